"""MI355X-native distillation hot path of irfanICMLL/structure_knowledge_distillation.

Sub-packages mirror the reference's import surface for this path so that its
``train_and_eval.py`` loop runs unchanged after the aliasing shown in INTEGRATION.md:

    libs      -> InPlaceABN / InPlaceABNSync            (reference: libs/)
    networks  -> kd_model.NetModel, pspnet_combine, sagan_models, spectral
    utils     -> criterion (the six loss classes), utils (sim_dis_compute ...), parallel shims

All device work goes through ``libskd_hip.so`` (hand-written gfx950 kernels behind the C ABI of
include/skd.h) or MIOpen/rocBLAS via PyTorch-ROCm for the convolutions.  There is no CPU path.
"""
__version__ = "0.1.0"

import os as _os

# MIOpen user find-db + kernel cache tuned for this step's convolution shapes on gfx950 (made by
# tools/miopen_tune.py with MIOpen's own tuner; the ROCm image ships no gfx950 database).  Must be in
# the environment before the first convolution initialises MIOpen.
#
# MIOpen treats the user db / cache directories as WRITABLE (an unseen problem appends to them), so the shipped
# database is never handed over directly: it is copied once into a per-user, per-rank cache directory
# (SKD_MIOPEN_CACHE, default ~/.cache/skd_amd, /tmp as a last resort) and MIOpen is pointed at the copy -- eight ranks
# never append to the same git-tracked files, and a read-only install still works.
MIOPEN_DB_DIR = _os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "miopen_db")
MIOPEN_DB_VERSION = None       # (major, minor, patch) of the MIOpen build the shipped find-db was recorded with


def _miopen_db_version():
    import re
    for f in sorted(_os.listdir(MIOPEN_DB_DIR)):
        m = re.search(r"\.HIP\.(\d+)_(\d+)_(\d+)_", f)
        if m:
            return tuple(int(x) for x in m.groups())
    return None


def _private_miopen_db():
    """Copy of the shipped db in a per-user directory keyed by the db's content hash, the rank and the job (MASTER_PORT when
    torchrun set one): two jobs on one host, or eight ranks of one job, never append to the same files.  Other copies
    (superseded databases, finished jobs) that have not been touched for a week are pruned when a new copy is made."""
    import hashlib
    import shutil
    import tempfile
    import time
    tag = hashlib.sha1()
    for root, _, files in sorted(_os.walk(MIOPEN_DB_DIR)):
        for f in sorted(files):
            tag.update(f.encode())
            with open(_os.path.join(root, f), "rb") as fh:
                tag.update(fh.read())
    digest = tag.hexdigest()[:12]
    job = _os.environ.get("MASTER_PORT")
    name = "miopen_db_%s_r%s%s" % (digest, _os.environ.get("LOCAL_RANK", "0"), "_j" + job if job else "")
    bases = [_os.environ.get("SKD_MIOPEN_CACHE"), _os.path.join(_os.path.expanduser("~"), ".cache", "skd_amd"),
             _os.path.join(tempfile.gettempdir(), "skd_amd_%d" % _os.getuid())]
    for base in bases:
        if not base:
            continue
        dst = _os.path.join(base, name)
        try:
            if not _os.path.isdir(dst):
                _os.makedirs(base, exist_ok=True)
                tmp = tempfile.mkdtemp(prefix=name + ".", dir=base)
                _copy_writable(MIOPEN_DB_DIR, _os.path.join(tmp, "db"))
                try:
                    _os.rename(_os.path.join(tmp, "db"), dst)      # atomic: concurrent ranks race harmlessly
                except OSError:
                    pass
                shutil.rmtree(tmp, ignore_errors=True)
                for other in _os.listdir(base):                    # garbage-collect copies of superseded databases
                    path = _os.path.join(base, other)
                    if other.startswith("miopen_db_") and path != dst and _os.path.isdir(path) and _idle_for(path) > 7 * 86400:
                        shutil.rmtree(path, ignore_errors=True)
            if _os.path.isdir(dst) and _writable(dst):
                try:
                    _os.utime(dst, None)       # "in use now": a directory's own mtime does not move when MIOpen appends to the files inside
                except OSError:
                    pass
                return dst
        except OSError:
            continue
    return None


def _copy_writable(src, dst):
    """shutil.copytree WITHOUT the source's permission bits: the shipped files may be read-only (a read-only checkout or
    install), and MIOpen must be able to append to its copy -- a read-only user db / kernel cache fails the first convolution
    with miopenStatusInternalError."""
    import shutil
    for root, _, files in _os.walk(src):
        out = _os.path.join(dst, _os.path.relpath(root, src))
        _os.makedirs(out, exist_ok=True)
        for f in files:
            shutil.copyfile(_os.path.join(root, f), _os.path.join(out, f))
    _writable(dst)


def _writable(path):
    """Give the owner write access to everything under ``path`` (a private copy: ours; older versions of this package copied the
    shipped permission bits); False when that is not possible."""
    import stat
    try:
        for root, dirs, files in _os.walk(path):
            for p, extra in [(root, stat.S_IRWXU)] + [(_os.path.join(root, f), stat.S_IRUSR | stat.S_IWUSR) for f in files]:
                mode = _os.stat(p).st_mode
                if mode & extra != extra:
                    _os.chmod(p, mode | extra)
        return all(_os.access(_os.path.join(r, n), _os.W_OK) for r, _, fs in _os.walk(path) for n in fs + [""])
    except OSError:
        return False


def _idle_for(path):
    """Seconds since anything in a private database copy was used: the newest mtime of the directory itself (touched by every
    process that selects it, see above) and of the files MIOpen writes inside it (the db files, cache/) -- a job that runs for
    more than a week keeps its live MIOPEN_USER_DB_PATH."""
    import time
    newest = 0.0
    try:
        newest = _os.path.getmtime(path)
        for root, _, files in _os.walk(path):
            for f in files:
                try:
                    newest = max(newest, _os.path.getmtime(_os.path.join(root, f)))
                except OSError:
                    pass
    except OSError:
        return 0.0
    return time.time() - newest


def check_miopen_db(warn=True):
    """True when the running MIOpen matches the build the shipped find-db was tuned on.  A mismatch means MIOpen
    silently ignores the database (its file names carry the version) and falls back to untuned immediate-mode
    heuristics -- 58-70 instead of 107-137 TFLOP/s on the dilated 3x3 convolutions of this step -- so it WARNS loudly;
    re-run tools/miopen_tune.py on the new build."""
    configure_miopen()
    if MIOPEN_DB_VERSION is None:
        return True
    try:
        import torch
        v = torch.backends.cudnn.version()
    except Exception:
        return True
    if not v:
        return True
    have = (v // 1000000, (v // 1000) % 1000, v % 1000)
    if have != MIOPEN_DB_VERSION and warn:
        import warnings
        warnings.warn("structure_knowledge_distillation_amd: the shipped MIOpen find-db was tuned on MIOpen %d.%d.%d but this "
                      "process runs MIOpen %d.%d.%d: the tuned convolution kernels will NOT be used (expect ~40 %% lower "
                      "convolution throughput); re-run tools/miopen_tune.py" % (MIOPEN_DB_VERSION + have), RuntimeWarning)
    return have == MIOPEN_DB_VERSION


_configured = False


def configure_miopen(force=False):
    """Point MIOpen at (a private copy of) the shipped find-db / kernel cache and switch its fp32 Winograd solvers off.
    Process-wide, therefore EXPLICIT: importing the package changes nothing; ``NetModel.__init__``, ``bench.py``, the tools
    and tests/conftest.py call this before their first convolution (MIOpen reads the variables when its handle is created,
    so call it before running any convolution in the process; variables the user already set are left alone).

    Winograd: MIOpen's fp32 Winograd solvers lose about three decimal digits (measured on MI355X,
    tests/diagnostics/diag_dstep.py: 2.6e-4 relative error on the discriminator's backward-data convolutions with them,
    6e-7 without; the same kernels put 1.8e-3 on the student's DSN weight gradient at 256 x 256), which the WGAN critic's
    cancelling gradients amplify to per cent, they are NCHW-only (each call is wrapped in layout transposes), and whether
    immediate mode picks them varied between otherwise identical runs.  The step is not slower without them (76.9 vs
    77.1 ms).  MIOpen's own variable wins: MIOPEN_DEBUG_CONV_WINOGRAD=1 in the environment leaves its choice alone."""
    global _configured, MIOPEN_DB_VERSION
    if _configured and not force:
        return _os.environ.get("MIOPEN_USER_DB_PATH")
    _configured = True
    _os.environ.setdefault("MIOPEN_DEBUG_CONV_WINOGRAD", "0")
    if _os.path.isdir(MIOPEN_DB_DIR):
        MIOPEN_DB_VERSION = _miopen_db_version()
        if "MIOPEN_USER_DB_PATH" not in _os.environ:
            dst = _private_miopen_db() or MIOPEN_DB_DIR
            _os.environ["MIOPEN_USER_DB_PATH"] = dst
            _os.environ.setdefault("MIOPEN_CUSTOM_CACHE_DIR", _os.path.join(dst, "cache"))
    return _os.environ.get("MIOPEN_USER_DB_PATH")
