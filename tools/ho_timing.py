"""Timing of the high-order elevation (k_ho_elevate, K13) beside the export transpose (k_soa_planes, K8), which moves the same 32 B per
node (16 read, 16 written).

Workload: one resident 4097^2 block (4096 cells per direction: orders 2, 4 and 8 divide it), three relaxation sweeps; in one run, per order
p = 2, 4, 8 and per distribution (Gauss-Lobatto, equidistant) tm_smoother_elevate with both planes and the scaled Jacobians, and
tm_smoother_export_soa with x and y only.  Event pairs around the calls, 7 repeats after one warm-up call, median and min-max.  A call
ends in the copy of its two planes to the host (268 MB, the same for K13 and K8), which the event pair includes and which outweighs
either kernel: the KERNEL times, and with them the ratio the aim is about, come from one separate profiler run with kernel tracing and
statistics only, whose per-dispatch trace --report turns into microseconds, TB/s and the K13 / K8 ratio per byte:

    python tools/ho_timing.py [--out profiles/ho_timing.txt]                                               (needs the MI355X)
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o ho -- python tools/ho_timing.py --repeats 3   (needs the MI355X)
    python tools/ho_timing.py --report <dir>/.../ho_kernel_trace.csv [--out ...]     (no GPU: reads the CSV, appends to --out)

Aim: K13 at most 1.5 x K8 per byte at p <= 4 (the margin is for the seam nodes read twice and for the record); at p = 8 the ratio is
only reported: 5(p+1) un-fused multiply-adds per component and node approach the fp64 issue time there."""
import argparse
import csv
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, REPEATS, ORDERS, DISTRIBUTIONS = 4097, 7, (2, 4, 8), ("gauss_lobatto", "equidistant")


def fmt(t):
    return f"median {statistics.median(t):9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}"


def timed(fn, repeats):
    import torch

    fn()   # warm-up: code objects, buffers
    t = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        t.append(e0.elapsed_time(e1))
    return t


def workload(n, repeats, out):
    import numpy as np
    import torch  # noqa: F401  (the events; also loads the HIP runtime the library shares)

    from turbomesh_amd import _capi, configs, highorder
    from turbomesh_amd.smoothing import smooth, solver

    lines = [f"high-order elevation of one resident {n}^2 block (tm_smoother_elevate: K13 + finalize + both planes and the element pairs to the host) beside "
             f"tm_smoother_export_soa (K8 + the same two planes to the host); event pairs around the calls, {repeats} repeats after a warm-up call "
             "(tools/ho_timing.py).  The copies of the planes dominate both: kernel times below, from the profiler run"]
    with smooth.Smoother(configs.single_block(n, n, perturb=0.25), solver.Option.hip(inner=solver.Inner.relax)) as sm:
        sm.iterate(3)
        x, y = np.empty(n * n), np.empty(n * n)
        for p in ORDERS:
            for dist in DISTRIBUTIONS:
                el = highorder.Elevation(p, dist)
                q = sm.elevate(el, 0)[2]
                t = timed(lambda: sm.elevate(el, 0), repeats)
                lines.append(f"  K13 p {p} {dist:13s} {fmt(t)}   elements {q.elements} invalid {q.invalid} min scaled jacobian {q.min_scaled_jacobian:.4f}")
        t = timed(lambda: _capi.check(_capi.lib().tm_smoother_export_soa(sm._h, 0, _capi.f64ptr(x), _capi.f64ptr(y), None, None)), repeats)
        lines.append(f"  K8  x and y only        {fmt(t)}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


def report(trace_csv, out, n):
    """Per-dispatch rows in launch order: for every order the first half of the k_ho_elevate<p> dispatches are Gauss-Lobatto, the second
    half equidistant (the order of workload()); the first dispatch of each group is the warm-up and is left out."""
    by_name = {}
    with open(trace_csv) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        by_name.setdefault(r["Kernel_Name"], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)   # microseconds

    def group(pattern):
        hits = [v for k, v in by_name.items() if re.search(pattern, k)]
        if len(hits) != 1:
            sys.exit(f"{trace_csv}: {len(hits)} kernels match {pattern}")
        return hits[0]

    k8 = group(r"\bk_soa_planes\(")
    k8 = k8[1:] if len(k8) > 1 else k8
    k8_med = statistics.median(k8)
    nodes = float(n) * n
    lines = [f"kernel times of one rocprofv3 --kernel-trace --stats run of tools/ho_timing.py (no counters), {n}^2 nodes, per dispatch, warm-up dispatches left out; "
             "both kernels move 32 B per node (K13 reads the nodes on tile seams twice on top)",
             f"  K8  k_soa_planes             {len(k8):2d} dispatches  median {k8_med:8.1f} us  min {min(k8):8.1f}  max {max(k8):8.1f}   {32 * nodes / k8_med / 1e6:.2f} TB/s"]
    for p in ORDERS:
        d = group(rf"\bk_ho_elevate<{p}>")
        half = len(d) // 2
        for dist, part in (("gauss_lobatto", d[:half]), ("equidistant", d[half:])):
            part = part[2:] if len(part) > 2 else part   # the call that fetched the record and timed()'s warm-up
            med = statistics.median(part)
            ratio = med / k8_med
            verdict = "reported only" if p > 4 else ("HIT" if ratio <= 1.5 else "MISSED")
            lines.append(f"  K13 p {p} {dist:13s}      {len(part):2d} dispatches  median {med:8.1f} us  min {min(part):8.1f}  max {max(part):8.1f}   {32 * nodes / med / 1e6:.2f} TB/s   "
                         f"{ratio:.2f} x K8 per byte (aim at p <= 4: at most 1.5) -- {verdict}")
    for label, pattern in (("k_ho_reduce   (records, first stage)", r"\bk_ho_reduce\("), ("k_ho_finalize (records -> tm_ho_quality)", r"\bk_ho_finalize\(")):
        hits = [v for k, v in by_name.items() if re.search(pattern, k)]
        if hits:
            lines.append(f"  {label:42s} {len(hits[0]):3d} dispatches  median {statistics.median(hits[0]):8.1f} us  min {min(hits[0]):8.1f}  max {max(hits[0]):8.1f}   (behind every K13 launch)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "a") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--report", metavar="KERNEL_TRACE_CSV")
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", type=int, default=N)
    ap.add_argument("--repeats", type=int, default=REPEATS)
    args = ap.parse_args()
    if args.report:
        report(args.report, args.out, args.size)
    else:
        workload(args.size, args.repeats, args.out)


if __name__ == "__main__":
    main()
