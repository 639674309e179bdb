"""The pair-wise loss's two matrix products on the split bf16-MFMA core (csrc/pairwise_split.hip, include/skd_pairwise_split.h)
on the GPU: skd_pairwise_split_gram_loss and skd_pairwise_split_backward beside their fp32 twins of skd.h on the same buffers.

Accuracy contract (the one every split kernel here was accepted under): the error of G and of dpooled against float64 is at most
FOUR times the fp32 twin's own error measured in the same test on the same inputs, and never more than the tolerance
tests/test_kernels_gpu.py::test_pairwise_stages holds the fp32 kernels to (G 2e-5 against a floor of 1.0, dpooled 5e-5 of
max |want|).  The loss is a sum of M^2 squares whose error is summation noise in both kernels: 1e-5 relative, floor 1e-6.
The figures of both kernels are printed per case (profiles/r29_pairwise_split_accuracy.md records them).

The entries are called unconditionally: a library without them fails these tests, it does not skip them.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import bounds_cases as BC
from structure_knowledge_distillation_amd import _lib, functional as SF

pytestmark = pytest.mark.gpu

DEV = "cuda"
RATIO = 4.0
CAP_G, CAP_DP, TOL_LOSS, FLOOR_LOSS = 2e-5, 5e-5, 1e-5, 1e-6
GL = 0.5                      # the upstream gradient handed to the backward entries

# (B, Cs, Ct, M)
SHAPES = [
    (2, 12, 20, 65),          # first size past the small path, one ragged tile, K tails
    (3, 8, 8, 128),           # exact tile, odd batch
    (2, 12, 20, 129),         # two tiles, the ragged one off the diagonal, mirror
    (2, 130, 70, 289),        # K tails, two (three: 64-row) channel tiles in the backward
    (1, 128, 512, 1089),      # the step's channel counts, nine tiles
]
GUARDED = [(2, 12, 20, 129), (2, 130, 70, 289)]
MANY = (1, 16, 16, 4225)      # the 34 x 34 triangular schedule, B = 1, the backward's longest K


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def hip():
    return _lib.load()


def pooled(shape):
    B, Cs, Ct, M = shape
    g = torch.Generator().manual_seed(M + Cs)
    return torch.randn(B, Cs, M, generator=g), torch.randn(B, Ct, M, generator=g)


def normalise(hip, shape, ps, pt):
    """(fhat_s, fhat_t, norm_s, ldm) on the GPU from the project's own normalise kernel, the buffers pre-filled with 9."""
    B, Cs, Ct, M = shape
    ldm = hip.skd_pairwise_ldm(M)
    fs, ft = torch.full((B, Cs, ldm), 9.0, device=DEV), torch.full((B, Ct, ldm), 9.0, device=DEV)
    nrm = torch.empty(B, M, device=DEV)
    assert hip.skd_channel_l2_normalise(B, Cs, M, P(ps.to(DEV)), P(fs), ldm, None, 0, P(nrm), None)
    assert hip.skd_channel_l2_normalise(B, Ct, M, P(pt.to(DEV)), P(ft), ldm, None, 0, None, None)
    return fs, ft, nrm, ldm


def gram(hip, split, shape, ldm, fs, ft, want_g=True):
    B, Cs, Ct, M = shape
    G = torch.full((B, ldm, ldm), 9.0, device=DEV) if want_g else None
    loss = torch.full((1,), 9.0, device=DEV)
    if split:
        ws = torch.full((max(1, hip.skd_pairwise_split_workspace_floats(B, Cs, Ct, M)),), float("nan"), device=DEV)
        assert hip.skd_pairwise_split_gram_loss(B, Cs, Ct, M, ldm, P(fs), P(ft), P(G), P(loss), P(ws), None) == 1
    else:
        ws = torch.empty(max(1, hip.skd_pairwise_workspace_floats(B, M)), device=DEV)
        assert hip.skd_pairwise_gram_loss(B, Cs, Ct, M, ldm, P(fs), P(ft), P(G), P(loss), P(ws), None) == 1
    return G, loss


def backward(hip, split, shape, ldm, fs, G, nrm, gl=GL):
    B, Cs, _, M = shape
    dp = torch.full((B, Cs, ldm), 9.0, device=DEV)
    glt = torch.tensor([gl], device=DEV)
    if split:
        ws = torch.full((max(1, hip.skd_pairwise_split_backward_workspace_floats(B, Cs, M)),), float("nan"), device=DEV)
        assert hip.skd_pairwise_split_backward(B, Cs, M, ldm, P(fs), P(G), P(nrm), P(glt), P(dp), P(ws), None) == 1
    else:
        ws = torch.empty(max(1, hip.skd_pairwise_backward_workspace_floats(B, Cs, M)), device=DEV)
        assert hip.skd_pairwise_backward(B, Cs, M, ldm, P(fs), P(G), P(nrm), P(glt), P(dp), P(ws), None) == 1
    return dp


def truth64(shape, ps, pt):
    """(G, loss, dpooled for an upstream gradient of GL) of the reference formula (utils.py:170-183) in float64 on the CPU."""
    B, _, _, M = shape
    x = ps.double().requires_grad_(True)
    fh = x / ((x ** 2).sum(1, keepdim=True).sqrt() + 1e-8).detach()
    th = pt.double() / ((pt.double() ** 2).sum(1, keepdim=True).sqrt() + 1e-8)
    G = torch.einsum("icm,icn->imn", th, th) - torch.einsum("icm,icn->imn", fh, fh)
    L = (G ** 2).sum() / M ** 2 / B
    L.backward()
    return G.detach(), L.detach(), GL * x.grad


def err_g(got, want):
    got = got.detach().cpu().double()
    assert bool(torch.isfinite(got).all())
    return float((got - want.cpu()).abs().max()) / max(float(want.abs().max()), 1.0)


def err_dp(got, want):
    got = got.detach().cpu().double()
    assert bool(torch.isfinite(got).all())
    return float((got - want.cpu()).abs().max()) / max(float(want.abs().max()), 1e-30)


def err_loss(got, want):
    return abs(float(got) - float(want)) / max(abs(float(want)), FLOOR_LOSS)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


_RUNS = {}


def run(hip, shape):
    """Everything one shape needs, computed once and shared (never modified): the float64 truth and both kernels' outputs on the
    same normalised buffers, the backward entries on the SAME G (the fp32 twin's)."""
    if shape not in _RUNS:
        ps, pt = pooled(shape)
        fs, ft, nrm, ldm = normalise(hip, shape, ps, pt)
        G0, l0 = gram(hip, False, shape, ldm, fs, ft)
        G1, l1 = gram(hip, True, shape, ldm, fs, ft)
        _RUNS[shape] = dict(ldm=ldm, fs=fs, ft=ft, nrm=nrm, want=truth64(shape, ps, pt), G0=G0, l0=l0, G1=G1, l1=l1,
                            dp0=backward(hip, False, shape, ldm, fs, G0, nrm), dp1=backward(hip, True, shape, ldm, fs, G0, nrm))
    return _RUNS[shape]


def check_bound(what, shape, new, parent, cap):
    bound = min(RATIO * parent, cap)
    print("%s %s: split %.3e  fp32 twin %.3e  bound %.3e" % (what, shape, new, parent, bound))
    assert new <= bound, "%s %s: err %.3e > %.3e (fp32 twin: %.3e, cap %.1e)" % (what, shape, new, bound, parent, cap)


# ---- 1. accuracy against float64, beside the fp32 twin ------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_gram_vs_float64(hip, shape):
    M = shape[3]
    r = run(hip, shape)
    G64, L64, _ = r["want"]
    check_bound("G", shape, err_g(r["G1"][:, :M, :M], G64), err_g(r["G0"][:, :M, :M], G64), CAP_G)
    e1, e0 = err_loss(r["l1"], L64), err_loss(r["l0"], L64)
    print("loss %s: split %.3e  fp32 twin %.3e  bound %.1e" % (shape, e1, e0, TOL_LOSS))
    assert e1 <= TOL_LOSS, "loss %s: %.3e > %.1e" % (shape, e1, TOL_LOSS)


@pytest.mark.parametrize("shape", SHAPES)
def test_backward_vs_float64(hip, shape):
    M = shape[3]
    r = run(hip, shape)
    want = r["want"][2]
    check_bound("dpooled", shape, err_dp(r["dp1"][..., :M], want), err_dp(r["dp0"][..., :M], want), CAP_DP)


# ---- 2. structure ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_structure(hip, shape):
    B, Cs, Ct, M = shape
    r = run(hip, shape)
    ldm, G, dp = r["ldm"], r["G1"], r["dp1"]
    assert torch.equal(bits(G), bits(G.transpose(1, 2))), "G is not bit-for-bit symmetric"
    if ldm > M:
        assert bool((bits(G[:, M:, :]) == 0).all()) and bool((bits(G[:, :, M:]) == 0).all()), "rows / columns >= M of G are not +0.0"
        assert bool((bits(dp[:, :, M:]) == 0).all()), "columns >= M of dpooled are not +0.0"
    # the same bits on a second call; the loss alone (G = NULL) has the same bits
    G2, l2 = gram(hip, True, shape, ldm, r["fs"], r["ft"])
    assert torch.equal(bits(G2), bits(G)) and torch.equal(bits(l2), bits(r["l1"]))
    _, l3 = gram(hip, True, shape, ldm, r["fs"], r["ft"], want_g=False)
    assert torch.equal(bits(l3), bits(r["l1"]))
    assert torch.equal(bits(backward(hip, True, shape, ldm, r["fs"], r["G0"], r["nrm"])), bits(dp))


# ---- 3. integers are exact -------------------------------------------------------------------------------------------------------

def int_panel(gen, B, C, M, ldm):
    t = torch.zeros(B, C, ldm)
    t[:, :, :M] = torch.randint(-2, 3, (B, C, M), generator=gen).float()
    return t


@pytest.mark.parametrize("shape", [(2, 32, 48, 128), (2, 12, 20, 129)])
def test_gram_integers_bit_exact(hip, shape):
    B, Cs, Ct, M = shape
    ldm = hip.skd_pairwise_ldm(M)
    gen = torch.Generator().manual_seed(7 * M + Cs)
    fs, ft = int_panel(gen, B, Cs, M, ldm), int_panel(gen, B, Ct, M, ldm)
    want = (torch.einsum("icm,icn->imn", ft.long(), ft.long()) - torch.einsum("icm,icn->imn", fs.long(), fs.long()))
    assert int(want.abs().max()) > 20
    G0, _ = gram(hip, False, shape, ldm, fs.to(DEV), ft.to(DEV))
    G1, l1 = gram(hip, True, shape, ldm, fs.to(DEV), ft.to(DEV))
    assert torch.equal(G1.cpu().double(), want.double()), "%d entries differ from the int64 Gram" % int((G1.cpu().double() != want.double()).sum())
    assert torch.equal(bits(G1), bits(G0))
    L = float((want.double() ** 2).sum()) / M ** 2 / B
    assert abs(float(l1) - L) <= TOL_LOSS * L


@pytest.mark.parametrize("B,Cs,M", [(2, 32, 128), (1, 32, 256)])
def test_backward_integers_bit_exact(hip, B, Cs, M):
    """Integer Fh_S and G, norm 1, upstream gradient 1: coef = -4 / (M^2 B) is a power of two, every product and sum is exact."""
    ldm = hip.skd_pairwise_ldm(M)
    assert ldm == M
    gen = torch.Generator().manual_seed(11 * M + B)
    fs = int_panel(gen, B, Cs, M, ldm)
    G = torch.randint(-2, 3, (B, M, M), generator=gen)
    G = (torch.triu(G) + torch.triu(G, 1).transpose(1, 2)).float()
    assert torch.equal(G, G.transpose(1, 2))
    shape = (B, Cs, 0, M)
    nrm = torch.ones(B, M, device=DEV)
    dp0 = backward(hip, False, shape, ldm, fs.to(DEV), G.to(DEV), nrm, gl=1.0)
    dp1 = backward(hip, True, shape, ldm, fs.to(DEV), G.to(DEV), nrm, gl=1.0)
    want = torch.einsum("bcn,bmn->bcm", fs.double(), G.double()) * (-4.0 / (M * M * B))
    assert float(want.abs().max()) > 0
    assert torch.equal(dp1.cpu().double(), want), "%d entries differ from the exact product" % int((dp1.cpu().double() != want).sum())
    assert torch.equal(bits(dp1), bits(dp0))


# ---- 4. many tiles ---------------------------------------------------------------------------------------------------------------

def test_many_tiles_on_the_gpu_only(hip):
    """34 x 34 tiles, 1156 + 34 work items of the triangular schedule, B = 1, the backward's longest K.  No CPU float64 work: the
    float64 expectation is torch's on the GPU, from the very fp32 buffers both kernels read, so the figures hold the kernels'
    own rounding alone."""
    shape = MANY
    B, Cs, Ct, M = shape
    ps, pt = pooled(shape)
    fs, ft, nrm, ldm = normalise(hip, shape, ps, pt)
    G0, l0 = gram(hip, False, shape, ldm, fs, ft)
    G1, l1 = gram(hip, True, shape, ldm, fs, ft)
    fs64, ft64 = fs.double(), ft.double()
    G64 = torch.bmm(ft64.transpose(1, 2), ft64) - torch.bmm(fs64.transpose(1, 2), fs64)
    scale = max(float(G64.abs().max()), 1.0)
    e0, e1 = float((G0.double() - G64).abs().max()) / scale, float((G1.double() - G64).abs().max()) / scale
    check_bound("G", shape, e1, e0, CAP_G)
    L64 = float((G64 ** 2).sum()) / M ** 2 / B
    assert err_loss(l1, L64) <= TOL_LOSS
    assert torch.equal(G1.view(torch.int32), G1.transpose(1, 2).contiguous().view(torch.int32))
    assert bool((G1[:, M:, :].contiguous().view(torch.int32) == 0).all()) and bool((G1[:, :, M:].contiguous().view(torch.int32) == 0).all())
    del G64, ft64
    dp0, dp1 = backward(hip, False, shape, ldm, fs, G0, nrm), backward(hip, True, shape, ldm, fs, G0, nrm)
    coef = -4.0 / (float(M) * M * B) * GL
    want = coef * torch.bmm(fs64, G0.double())[:, :, :M] / nrm.double()[:, None, :]
    scale = float(want.abs().max())
    e0, e1 = float((dp0[..., :M].double() - want).abs().max()) / scale, float((dp1[..., :M].double() - want).abs().max()) / scale
    check_bound("dpooled", shape, e1, e0, CAP_DP)
    assert bool((dp1[:, :, M:].contiguous().view(torch.int32) == 0).all())


# ---- 5. guard bands ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", GUARDED)
def test_guard_bands(hip, shape):
    """Every input, output and workspace at exact size between 0xFF guards, the workspaces never initialised, each entry called
    twice on the same buffers: the same bits, every output element written, the guards intact."""
    B, Cs, Ct, M = shape
    r = run(hip, shape)
    ldm = r["ldm"]
    A = BC.Arena(DEV)
    fs, ft = A.inp("fhat_s", r["fs"].cpu()), A.inp("fhat_t", r["ft"].cpu())
    G, loss = A.out("G", (B, ldm, ldm)), A.out("loss", (1,))
    ws = A.ws("workspace", hip.skd_pairwise_split_workspace_floats(B, Cs, Ct, M))
    seen = []
    for k in range(2):
        if k:
            A.reset()
        assert hip.skd_pairwise_split_gram_loss(B, Cs, Ct, M, ldm, P(fs), P(ft), P(G), P(loss), P(ws), None) == 1
        A.check()
        seen.append((G.cpu().clone(), loss.cpu().clone()))
    assert BC.same_bits(seen[0][0], seen[1][0]) and BC.same_bits(seen[0][1], seen[1][1])
    assert BC.same_bits(seen[0][0], r["G1"].cpu()) and BC.same_bits(seen[0][1], r["l1"].cpu())

    A = BC.Arena(DEV)
    fs, Gi, nrm = A.inp("fhat_s", r["fs"].cpu()), A.inp("G", r["G0"].cpu()), A.inp("norm_s", r["nrm"].cpu())
    gl, dp = A.inp("grad_loss", torch.tensor([GL])), A.out("dpooled", (B, Cs, ldm))
    ws = A.ws("workspace", hip.skd_pairwise_split_backward_workspace_floats(B, Cs, M))
    seen = []
    for k in range(2):
        if k:
            A.reset()
        assert hip.skd_pairwise_split_backward(B, Cs, M, ldm, P(fs), P(Gi), P(nrm), P(gl), P(dp), P(ws), None) == 1
        A.check()
        seen.append(dp.cpu().clone())
    assert bool(torch.isfinite(seen[0]).all()), "an element of dpooled was not written"
    assert BC.same_bits(seen[0], seen[1]) and BC.same_bits(seen[0], r["dp1"].cpu())


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals(hip):
    shape = (2, 12, 20, 129)
    B, Cs, Ct, M = shape
    r = run(hip, shape)
    ldm, fs, ft, nrm, G0 = r["ldm"], r["fs"], r["ft"], r["nrm"], r["G0"]
    G, loss = torch.full((B * ldm * ldm + 4,), 7.0, device=DEV), torch.full((1,), 7.0, device=DEV)
    ws = torch.full((hip.skd_pairwise_split_workspace_floats(B, Cs, Ct, M) + 4,), 7.0, device=DEV)
    off = lambda t: ctypes.c_void_p(t.data_ptr() + 4)          # 4 bytes past a 16-byte boundary
    good = [B, Cs, Ct, M, ldm, P(fs), P(ft), P(G), P(loss), P(ws), None]
    bad = []
    for i in (5, 6, 8, 9):                                      # a NULL pointer (G may be NULL)
        bad.append(good[:i] + [None] + good[i + 1:])
    bad.append(good[:4] + [ldm + 128] + good[5:])               # ldm != skd_pairwise_ldm(M)
    bad.append(good[:4] + [M] + good[5:])
    bad.append(good[:5] + [off(fs)] + good[6:])                 # misaligned buffers
    bad.append(good[:6] + [off(ft)] + good[7:])
    bad.append(good[:7] + [off(G)] + good[8:])
    bad.append(good[:9] + [off(ws)] + good[10:])
    bad.append([65536] + good[1:])                              # B > 65535
    for args in bad:
        assert hip.skd_pairwise_split_gram_loss(*args) == 0, args[:5]
    torch.cuda.synchronize()
    assert float(G.min()) == 7.0 == float(G.max()) and float(loss) == 7.0 and float(ws.min()) == 7.0 == float(ws.max())

    dp, gl = torch.full((B * Cs * ldm + 4,), 7.0, device=DEV), torch.tensor([GL], device=DEV)
    ws = torch.full((hip.skd_pairwise_split_backward_workspace_floats(B, Cs, M) + 4,), 7.0, device=DEV)
    good = [B, Cs, M, ldm, P(fs), P(G0), P(nrm), P(gl), P(dp), P(ws), None]
    bad = [good[:i] + [None] + good[i + 1:] for i in (4, 5, 6, 7, 8, 9)]
    bad.append(good[:3] + [ldm + 128] + good[4:])
    bad.append(good[:3] + [M] + good[4:])
    bad.append(good[:4] + [off(fs)] + good[5:])
    bad.append(good[:5] + [off(G0)] + good[6:])
    bad.append(good[:8] + [off(dp)] + good[9:])
    bad.append(good[:9] + [off(ws)] + good[10:])
    bad.append([65536] + good[1:])
    for args in bad:
        assert hip.skd_pairwise_split_backward(*args) == 0, args[:4]
    torch.cuda.synchronize()
    assert float(dp.min()) == 7.0 == float(dp.max()) and float(ws.min()) == 7.0 == float(ws.max())


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------------

def features(nhwc):
    g = torch.Generator().manual_seed(33)
    fs, ft = torch.randn(2, 128, 33, 33, generator=g), torch.randn(2, 512, 33, 33, generator=g)
    if nhwc:
        fs, ft = fs.contiguous(memory_format=torch.channels_last), ft.contiguous(memory_format=torch.channels_last)
    return fs, ft


_E2E = {}


def e2e_truth(k):
    """float64 loss and gradient of criterion.py:236-245 on the CPU for kernel ``k`` (the layout does not change them)."""
    if k not in _E2E:
        fs, ft = features(False)
        x = fs.double().requires_grad_(True)
        ps, pt = F.max_pool2d(x, k, k, 0, ceil_mode=True), F.max_pool2d(ft.double(), k, k, 0, ceil_mode=True)
        B, M = ps.shape[0], ps.shape[2] * ps.shape[3]
        ps, pt = ps.reshape(B, -1, M), pt.reshape(B, -1, M)
        fh = ps / ((ps ** 2).sum(1, keepdim=True).sqrt() + 1e-8).detach()
        th = pt / ((pt ** 2).sum(1, keepdim=True).sqrt() + 1e-8)
        L = ((torch.einsum("icm,icn->imn", th, th) - torch.einsum("icm,icn->imn", fh, fh)) ** 2).sum() / M ** 2 / B
        L.backward()
        _E2E[k] = (L.detach(), x.grad)
    return _E2E[k]


def loss_and_grad(fs, ft, k, split):
    x = fs.to(DEV).requires_grad_(True)
    loss = SF.pair_wise_loss(x, ft.to(DEV), k, k, split=split)
    loss.backward()
    return loss.detach(), x.grad


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "channels_last"])
@pytest.mark.parametrize("k,M", [(1, 1089), (2, 289)])
def test_end_to_end(monkeypatch, nhwc, k, M):
    monkeypatch.setattr(SF, "PAIRWISE_SPLIT_ROUTING_EXCLUDED", frozenset())      # whatever the measured set holds: the split path
    assert SF.pairwise_split_supported()
    fs, ft = features(nhwc)
    l0, g0 = loss_and_grad(fs, ft, k, False)
    names = ("skd_pairwise_gram_loss", "skd_pairwise_backward", "skd_pairwise_split_gram_loss", "skd_pairwise_split_backward")
    _lib.enable_kernel_timing(names)
    try:
        l1, g1 = loss_and_grad(fs, ft, k, True)
    finally:
        calls = _lib.disable_kernel_timing()
    assert [len(calls[n]) for n in names] == [0, 0, 1, 1], "split=True did not take the split entries"
    assert g1.shape == g0.shape and g1.stride() == g0.stride()
    assert abs(float(l1) - float(l0)) <= 1e-5 * abs(float(l0))
    L64, grad64 = e2e_truth(k)
    assert err_loss(l1, L64) <= TOL_LOSS
    check_bound("feature gradient", (2, 128, 512, M), err_dp(g1, grad64), err_dp(g0, grad64), CAP_DP)


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "channels_last"])
def test_small_graphs_are_untouched(monkeypatch, nhwc):
    monkeypatch.setattr(SF, "PAIRWISE_SPLIT_ROUTING_EXCLUDED", frozenset())
    fs, ft = features(nhwc)
    l0, g0 = loss_and_grad(fs, ft, 11, False)                   # 3 x 3 = 9 nodes: skd_pairwise_small
    l1, g1 = loss_and_grad(fs, ft, 11, True)
    assert torch.equal(bits(l0), bits(l1)) and torch.equal(g0.view(torch.int32), g1.view(torch.int32))
