"""tools/timeline.py on a synthetic rocprofv3 kernel trace: the step cutting (end of the D queue's last kernel), the per-stream busy /
idle accounting, main-stream gaps and the exposed D tail -- the arithmetic DESIGN.md section 9.5's critical-path statement rests on."""
import csv
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _trace(path, steps=6):
    """Per step (1 ms apart, times in ns): main queue 1: teacher 0-300 us, pixel-wise loss 300-310, backward 310-700 with a 40 us hole
    at 500; D queue 4: sn_bwd + conv 350-650 (overlapping the backward) and a tail 700-760 after the main stream's last kernel."""
    rows = []
    for k in range(steps):
        t = k * 1_000_000
        rows += [(1, "igemm_fwd_teacher", t + 0, t + 300_000), (1, "void skd::(anonymous namespace)::pixelwise_kernel(float const*)", t + 300_000, t + 310_000),
                 (1, "igemm_bwd_a", t + 310_000, t + 500_000), (1, "igemm_wrw_b", t + 540_000, t + 700_000),
                 (4, "skd::(anonymous namespace)::sn_bwd_dot_multi_kernel(skd::SnBatch)", t + 350_000, t + 400_000), (4, "igemm_fwd_d", t + 400_000, t + 650_000),
                 (4, "void at::native::(anonymous namespace)::multi_tensor_apply_kernel<x>", t + 700_000, t + 760_000)]
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["Kind", "Queue_Id", "Stream_Id", "Kernel_Name", "Start_Timestamp", "End_Timestamp"])
        for q, n, s, e in rows:
            w.writerow(["KERNEL_DISPATCH", q, 0, n, s, e])


def test_timeline_cuts_steps_and_accounts_streams(tmp_path):
    src, dst = tmp_path / "bench_kernel_trace.csv", tmp_path / "timeline.md"
    _trace(str(src))
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "timeline.py"), str(src), str(dst), "1", "4"], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    text = dst.read_text()
    assert "`q1` (**main**)" in text and "`q4` (**D step**)" in text
    mean = [l for l in text.splitlines() if l.startswith("| **mean**")][0].split("|")
    wall, main_busy, main_idle, d_busy, both, idle, tail = [float(x) for x in mean[2:9]]
    assert abs(wall - 1.0) < 1e-6                                     # a step = the interval between two ends of the D queue
    assert abs(main_busy - 0.66) < 1e-6 and abs(main_idle - 0.34) < 1e-6
    assert abs(d_busy - 0.36) < 1e-6 and abs(both - 0.26) < 1e-6      # 350-500 and 540-650 overlap the backward
    assert abs(tail - 0.06) < 1e-6                                    # the D stream's last 60 us are exposed
    assert abs(idle - 0.24) < 1e-6                                    # the 240 us between the steps (the 40 us hole of the main stream is covered by the D stream)
    gaps = [l for l in text.splitlines() if l.startswith("| 40 |") or l.startswith("| 240 |")]
    assert any("igemm_bwd_a" in g and "igemm_wrw_b" in g for g in gaps), text      # the 40 us hole, with its neighbours named


# ---- tools/kernel_coverage.py: the name normalisation and the set difference, on trace lines written here ------------------------
# The two demangled spellings are rocprofv3's own, as committed in profiles/r01g_abn_microbench_kernel_stats.csv (a template
# kernel carries `void `, a plain one does not); the mangled ones are the same two kernels as the compiler's resource remarks and
# a tracer without demangling name them, once with the `.kd` suffix of the kernel descriptor.
_GRAD_DX = ("void skd::(anonymous namespace)::abn_grad_dx_kernel<0>(float const*, float const*, float const*, float const*, float const*, "
            "float const*, float const*, float*, float*, float*, float, float, int, int, int, skd::(anonymous namespace)::Plan, int, int)")
_GRAD_DX_MANGLED = "_ZN3skd12_GLOBAL__N_118abn_grad_dx_kernelILi0EEEvPKfS3_S3_S3_S3_S3_S3_PfS4_S4_ffiiiNS0_4PlanEii"
_STATS = "skd::(anonymous namespace)::abn_stats_partial_kernel(float const*, float*, int, int, int, skd::(anonymous namespace)::Plan)"
_STATS_MANGLED_KD = "_ZN3skd12_GLOBAL__N_124abn_stats_partial_kernelEPKfPfiiiNS0_4PlanE.kd"
_CE = ("void skd::(anonymous namespace)::ce_cells_kernel<19, true, true>(float const*, float const*, long const*, float*, float*, int, int, int, int, "
       "int, int, int, float, float, int, int, float const*, unsigned char*)")
_FOREIGN = ("igemm_fwd_gtcx35_nhwc_fp32_bx0_ex1_bt128x64x32_wt32x32x2_ws1x1_wr1x2_ta1x16x1x1_1x2x4x32_tb1x4x2x1_1x8x1x32_pta_gkgs",
            "void at::native::vectorized_elementwise_kernel<4, at::native::neg_kernel_cuda(at::TensorIteratorBase&)::{lambda()#2}>(int)",
            "__amd_rocclr_copyBuffer")


def _coverage_tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_coverage
    finally:
        sys.path.pop(0)
    return kernel_coverage


def test_kernel_coverage_normalises_mangled_and_demangled_spellings_alike():
    K = _coverage_tool()
    got = K.normalise([_GRAD_DX, _GRAD_DX_MANGLED, _STATS, _STATS_MANGLED_KD, _CE, '"%s"' % _STATS, _STATS + ".kd"])
    assert got == ["abn_grad_dx_kernel<0>", "abn_grad_dx_kernel<0>", "abn_stats_partial_kernel", "abn_stats_partial_kernel",
                   "ce_cells_kernel<19, true, true>", "abn_stats_partial_kernel", "abn_stats_partial_kernel"]
    static = {"abn_grad_dx_kernel<0>", "abn_grad_dx_kernel<1>", "abn_stats_partial_kernel", "ce_cells_kernel<19, true, true>", "ce_cells_kernel<64, true, true>"}
    assert not set(K.normalise(list(_FOREIGN))) & static                # a name that is not the library's matches nothing


def test_kernel_coverage_set_difference_and_launch_counts(tmp_path):
    """One run with a stats file (counts), one with a trace file (a row per launch) and a stats file beside it that is not added
    again; the library's never-launched kernels are the set difference, foreign names are dropped."""
    K = _coverage_tool()
    a, b = tmp_path / "a" / "host", tmp_path / "b"
    a.mkdir(parents=True)
    b.mkdir()
    with open(a / "test_x_gpu_kernel_stats.csv", "w", newline="") as fh:
        w = csv.writer(fh, quoting=csv.QUOTE_NONNUMERIC)
        w.writerow(["Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage", "MinNs", "MaxNs", "StdDev"])
        w.writerow([_GRAD_DX, 117, 7527016, 64333.47, 14.9, 10960, 162520, 49280.5])
        w.writerow([_STATS_MANGLED_KD, 3, 300, 100.0, 0.1, 90, 110, 1.0])
        w.writerow([_FOREIGN[0], 232, 151136662, 651451.1, 22.94, 167162, 10798617, 1673807.8])
    with open(b / "test_y_gpu_kernel_trace.csv", "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["Kind", "Agent_Id", "Queue_Id", "Kernel_Id", "Kernel_Name", "Correlation_Id", "Start_Timestamp", "End_Timestamp"])
        for k, n in enumerate((_STATS, _STATS, _CE, _FOREIGN[1], _GRAD_DX_MANGLED)):
            w.writerow(["KERNEL_DISPATCH", 4, 1, k, n, k, 1000 * k, 1000 * k + 500])
    with open(b / "test_y_gpu_kernel_stats.csv", "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["Name", "Calls"])
        w.writerow([_STATS, 2])
    static = {"abn_grad_dx_kernel<0>": "abn.hip", "abn_grad_dx_kernel<1>": "abn.hip", "abn_stats_partial_kernel": "abn.hip",
              "ce_cells_kernel<19, true, true>": "ce_ohem.hip", "ce_cells_kernel<64, true, true>": "ce_ohem.hip"}
    launched = K.launches([str(tmp_path / "a"), str(b)])
    hit, never = K.coverage(static, launched)
    assert never == ["abn_grad_dx_kernel<1>", "ce_cells_kernel<64, true, true>"]
    assert hit == {"abn_grad_dx_kernel<0>": {"test_x_gpu": 117, "test_y_gpu": 1}, "abn_stats_partial_kernel": {"test_x_gpu": 3, "test_y_gpu": 2},
                   "ce_cells_kernel<19, true, true>": {"test_y_gpu": 1}}
    text = K.report(static, launched, "t")
    assert "5 kernels (template instantiations counted), 3 launched, 2 never launched." in text
    assert "| `abn_grad_dx_kernel<0>` | 118 | test_x_gpu test_y_gpu |" in text and "| `ce_cells_kernel<64, true, true>` | **never** |  |" in text
    assert "## ce_ohem.hip: 1 of 2 launched" in text and "* `abn_grad_dx_kernel<1>` (abn.hip)" in text and "igemm" not in text
