"""Timing of the surface stage K15: the stacking kernel (k_stack_planes, K11) and the 3-D quality kernel (k_stack_quality, K12) with the
revolution mapping beside their cylindrical instantiations, in the same run.

Workload: 8 resident cuts of 2048^2 (config 5: amplitude 0.05 + 0.001 c, one handle per cut), cubic over the span, 16 layers, one
tm_stack_smoothers[_surf] call per window of k_count = 4, one tm_stack_smoothers_quality[_surf] call per round; the revolution mapping
with natural-spline tables of 65 knots per cut.  Kernel times come from ONE profiler run of this tool with kernel tracing and statistics
only (no counters in that run):

    rocprofv3 --kernel-trace --stats -d <dir> -o surf -- python tools/stack_surface_timing.py            (needs the MI355X)
    python tools/stack_surface_timing.py --report <dir>/.../surf_kernel_stats.csv [--out profiles/stack_surface_timing.txt]   (no GPU)

Both mappings move the same 16 K + 24 k_count = 224 B per node in K11; the revolution mapping adds per node and cut a search of
ceil(log2 64) = 6 steps in LDS, a gather of 64 B of coefficients and 14 flops.  Aim: a revolution launch of K11 takes <= 1.5 x a
cylindrical launch (reported as met or missed; K12 has no aim)."""
import argparse
import csv
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, CUTS, LAYERS, WINDOW, KNOTS, REPEATS = 2048, 8, 16, 4, 65, 3
AIM = 1.5


def workload(n, repeats):
    import numpy as np

    from turbomesh_amd import configs, stack
    from turbomesh_amd.smoothing import smooth, solver

    handles = [smooth.Smoother(configs.single_block(n, n, amplitude=0.05 + 0.001 * c), solver.Option.hip(inner=solver.Inner.relax)) for c in range(CUTS)]
    try:
        for h in handles:
            h.iterate(3)
        radii = 1.0 + 0.25 * np.arange(CUTS, dtype=np.float64)
        layers = stack.layers_from(radii, LAYERS)
        u = [np.linspace(-0.1, 1.1, KNOTS) for _ in range(CUTS)]
        x = [a + 0.02 * (c + 1) * np.sin(3 * a) for c, a in enumerate(u)]
        r = [radii[c] * (1 + 0.2 * np.tanh(2 * (a - 0.5))) for c, a in enumerate(u)]
        stacks = {"cylindrical": stack.Stack(radii, layers, "cubic", "cylindrical"),
                  "revolution": stack.Stack(radii, layers, "cubic", "revolution", surfaces=stack.Surfaces(u, x, r))}
        t0 = time.perf_counter()
        for _ in range(repeats + 1):   # the first round warms the code objects
            for st in stacks.values():
                for k in range(0, LAYERS, WINDOW):
                    st.block(handles, 0, k, WINDOW)
                st.quality(handles)
        outside = stacks["revolution"].block(handles, 0, 0, 1, return_outside=True)[3]
        print(f"stack_surface_timing: {repeats + 1} rounds of {LAYERS // WINDOW} windows of {WINDOW} layers and one quality report per mapping from {CUTS} cuts of "
              f"{n}^2, {time.perf_counter() - t0:.2f} s wall (device-to-host copies of the planes included); extrapolated nodes per cut {outside.tolist()}")
    finally:
        for h in handles:
            h.close()


def report(stats_csv, out, n):
    rows = {}
    with open(stats_csv) as f:
        for r in csv.DictReader(f):
            m = re.search(r"(k_stack_planes|k_stack_quality)<\s*(\d+)\s*,\s*(\d+)\s*>", r["Name"])
            if m and int(m.group(2)) == CUTS:
                rows[(m.group(1), int(m.group(3)))] = r
    need = [(k, m) for k in ("k_stack_planes", "k_stack_quality") for m in (1, 2)]
    if any(k not in rows for k in need):
        sys.exit(f"{stats_csv}: rows missing: {[k for k in need if k not in rows]}")
    nodes = float(n) * n
    us = lambda r, col: float(r[col]) / 1e3   # noqa: E731
    lines = [f"K15: the revolution mapping beside the cylindrical one on {n}^2 blocks: {CUTS} resident cuts, cubic over the span, {LAYERS} layers, windows of {WINDOW}; "
             f"tables of {KNOTS} knots per cut, natural splines; kernel times of one rocprofv3 --kernel-trace --stats run of tools/stack_surface_timing.py (no counters), "
             "every launch of the run averaged, the warm-up round included"]
    ratios = {}
    for key, what, bytes_per_node in (("k_stack_planes", "K11", 16 * CUTS + 24 * WINDOW), ("k_stack_quality", "K12", 16 * CUTS)):
        for m, name in ((1, "cylindrical"), (2, "revolution")):
            r = rows[(key, m)]
            rate = bytes_per_node * nodes / (us(r, "AverageNs") * 1e-6) / 1e12
            lines.append(f"  {what} {key:15s} {name:11s} {int(r['Calls']):3d} calls  average {us(r, 'AverageNs'):9.1f} us  min {us(r, 'MinNs'):9.1f}  max {us(r, 'MaxNs'):9.1f}   "
                         f"{rate:.3f} TB/s of {bytes_per_node} B/node")
        ratios[key] = us(rows[(key, 2)], "AverageNs") / us(rows[(key, 1)], "AverageNs")
    r11 = ratios["k_stack_planes"]
    lines.append(f"  K11 revolution / cylindrical = {r11:.2f} per launch (aim <= {AIM}): {'met' if r11 <= AIM else 'missed'}")
    lines.append(f"  K12 revolution / cylindrical = {ratios['k_stack_quality']:.2f} per launch (no aim; K12 marches all {LAYERS} layers in one launch)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--report", metavar="KERNEL_STATS_CSV")
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", type=int, default=N)
    ap.add_argument("--repeats", type=int, default=REPEATS)
    args = ap.parse_args()
    if args.report:
        report(args.report, args.out, args.size)
    else:
        workload(args.size, args.repeats)


if __name__ == "__main__":
    main()
