"""Which gfx950 kernels of libskd_hip.so (template instantiations counted) has a traced run launched?  A measurement, not a test:
it compares kernel NAMES and launch counts, nothing else -- a launched kernel can still be wrong, and a kernel that switches form
inside (a loop trip, a staged / un-staged path) shows one name for all of them; tests/regime_cases.py is the table for those.

  * static side: the kernel list of tools/kernel_resources.py (hipcc's kernel-resource-usage remarks, no GPU needed);
  * dynamic side: the "Name" / "Kernel_Name" column of every ``*kernel_stats.csv`` and ``*kernel_trace.csv`` under the directories
    given, as written by one rocprofv3 run per test file:

        rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python -m pytest tests/FILE.py -m gpu -q

    (each run under its own ``timeout``, the runs chained with ``&&``; no ``--pmc``: counters are collected in runs of their own);
  * both sides are normalised the same way (``normalise``): a trailing ``.kd`` dropped, mangled names demangled, then ``short()`` of
    tools/kernel_resources.py: ``void ``, the argument list, ``(anonymous namespace)::`` and ``skd::`` stripped.  Names of the trace
    that are not the library's (MIOpen, rocBLAS, Composable Kernel, torch) match nothing and are ignored.

    python tools/kernel_coverage.py DIR [DIR ...] [-o out.md]       (default: markdown to stdout)

Output: per source file a table of its kernels with the launch count and the runs that launched them, and the never-launched ones.
"""
import argparse
import csv
import os
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import demangle, one, short  # noqa: E402

NAME_COLUMNS = ("Name", "Kernel_Name", "KernelName")
COUNT_COLUMNS = ("Calls", "Count")


def normalise(names):
    """[spelling of the tracer or the compiler] -> [the library's short name]; one demangler call for the whole list."""
    names = [n.strip().strip('"') for n in names]
    names = [n[:-3] if n.endswith(".kd") else n for n in names]
    mangled = [i for i, n in enumerate(names) if n.startswith("_Z")]
    for i, d in zip(mangled, demangle([names[i] for i in mangled])):
        names[i] = d
    return [short(n) for n in names]


def static_kernels():
    """{short name: source file} of every kernel the library's sources compile to."""
    from structure_knowledge_distillation_amd import build as B
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(8) as ex:
        rows = [r for rs in ex.map(lambda s: one(s, tmp), B.sources()) for r in rs]
    return {n: r["file"] for r, n in zip(rows, normalise([r["name"] for r in rows]))}


def read_csv(path):
    """[(name as spelt, launches)] of one rocprofv3 CSV: a stats file has a count column, a trace file one row per launch."""
    with open(path, newline="") as f:
        rd = csv.DictReader(f)
        col = next((c for c in NAME_COLUMNS if c in (rd.fieldnames or ())), None)
        cnt = next((c for c in COUNT_COLUMNS if c in (rd.fieldnames or ())), None)
        if col is None:
            return []
        return [(r[col], int(r[cnt]) if cnt else 1) for r in rd if r.get(col)]


def launches(dirs):
    """{short name: {run: launches}} over every *kernel_stats.csv / *kernel_trace.csv under ``dirs``.  A run is the file's name up
    to ``_kernel_``; where a run has both files the trace (one row per launch) is authoritative and the stats file is not added."""
    per_run = {}
    for d in dirs:
        for base, _, files in os.walk(d):
            for f in sorted(files):
                for kind in ("kernel_trace.csv", "kernel_stats.csv"):
                    if f.endswith(kind):
                        run = f[:-len(kind)].rstrip("_") or os.path.basename(base)
                        per_run.setdefault(run, {})[kind] = os.path.join(base, f)
    out = {}
    for run, files in sorted(per_run.items()):
        rows = read_csv(files.get("kernel_trace.csv") or files["kernel_stats.csv"])
        for n, (_, c) in zip(normalise([r[0] for r in rows]), rows):
            out.setdefault(n, {}).setdefault(run, 0)
            out[n][run] += c
    return out


def coverage(static, launched):
    """(launched: {kernel: {run: count}}, never launched: sorted list) of the library's kernels; foreign names are dropped."""
    hit = {k: launched[k] for k in static if k in launched}
    return hit, sorted(k for k in static if k not in launched)


def report(static, launched, title):
    hit, never = coverage(static, launched)
    lines = ["# " + title, "", "%d kernels (template instantiations counted), %d launched, %d never launched." % (len(static), len(hit), len(never)), ""]
    for src in sorted(set(static.values())):
        mine = sorted(k for k, f in static.items() if f == src)
        miss = [k for k in mine if k not in hit]
        lines += ["## %s: %d of %d launched" % (src, len(mine) - len(miss), len(mine)), "", "| kernel | launches | runs |", "|---|---|---|"]
        for k in mine:
            runs = hit.get(k, {})
            lines.append("| `%s` | %s | %s |" % (k, sum(runs.values()) if runs else "**never**", " ".join(sorted(runs))))
        lines.append("")
    lines += ["## Never launched", ""] + ["* `%s` (%s)" % (k, static[k]) for k in never] + [""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("dirs", nargs="+")
    ap.add_argument("-o", "--out")
    ap.add_argument("--title", default="Kernel launch coverage of the GPU suite (tools/kernel_coverage.py)")
    a = ap.parse_args()
    text = report(static_kernels(), launches(a.dirs), a.title)
    if a.out:
        open(a.out, "w").write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
