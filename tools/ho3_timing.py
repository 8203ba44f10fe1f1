"""Timing of the high-order hexahedra of stacked blocks (k_stack_elevate, K16) beside the two kernels it is measured against: K11
(k_stack_planes), which writes the same node layers, and K12 (k_stack_quality), which judges the same layers as linear hexahedra.

Workload: 8 resident cuts of 2049^2 nodes (2048^2 cells, so that the orders 2 and 4 divide them; config 5: amplitude 0.05 + 0.001 c, one
handle per cut), cubic, planar, 33 layers.  In one run, each call 1 + REPEATS times:
  for p in (2, 4), nodes in (gauss_lobatto, equidistant):   tm_stack_smoothers_elevate with planes and report, then the report alone;
  tm_stack_smoothers, all 33 layers (K11: the same 24 B per node and layer as the copy path of K16);
  tm_stack_smoothers_quality (K12 over the same layers).
Every call ends in a stream synchronise inside the library, so the printed times are host-clock times around whole calls (they include the
3.3 GB of planes crossing to the host where planes are asked for).  Kernel times come from ONE separate profiler run with kernel tracing
and statistics only (no counters in that run); the tool finds its own launches in the trace by their order:

    python tools/ho3_timing.py [--out profiles/ho3_timing.txt]                                                     (needs the MI355X)
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o ho3 -- python tools/ho3_timing.py --repeats 2  (needs the MI355X)
    python tools/ho3_timing.py --report <dir>/.../ho3_kernel_trace.csv --repeats 2 [--out ...]     (no GPU: reads the CSV, appends to --out)

Yardsticks: the copy path against K11 per byte written -- the traffic is the same, the Jacobian arithmetic comes
on top; the report alone against K12 per evaluated corner -- K12 evaluates 8 corners per cell, K16 (p+1)^3 nodes per element."""
import argparse
import csv
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, CUTS, LAYERS, REPEATS = 2049, 8, 33, 5
CONFIGS = [(p, d) for p in (2, 4) for d in ("gauss_lobatto", "equidistant")]


def timed(fn, repeats):
    fn()   # warm-up: code objects, buffers
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return statistics.median(t), min(t), max(t)


def fmt(t):
    return f"{t[0] * 1e3:9.3f} ms ({t[1] * 1e3:.3f}-{t[2] * 1e3:.3f})"


def workload(n, repeats, out):
    import numpy as np

    from turbomesh_amd import configs, highorder, stack
    from turbomesh_amd.smoothing import smooth, solver

    handles = [smooth.Smoother(configs.single_block(n, n, amplitude=0.05 + 0.001 * c), solver.Option.hip(inner=solver.Inner.relax)) for c in range(CUTS)]
    lines = [f"high-order hexahedra of {CUTS} resident cuts of {n}^2 nodes, cubic, planar, {LAYERS} layers; host clock around calls that end in a stream "
             f"synchronise, {repeats} repeats after a warm-up call: median (min-max)"]
    try:
        for h in handles:
            h.iterate(3)
        z = np.arange(CUTS, dtype=np.float64)
        st = stack.Stack(z, stack.layers_from(z, LAYERS), "cubic", "planar")
        for p, dist in CONFIGS:
            el = highorder.Elevation(p, dist)
            q = st.elevate(handles, el, 0, planes=False)[3]
            t = timed(lambda: st.elevate(handles, el, 0), repeats)
            lines.append(f"  K16 p {p} {dist:13s} planes + report ({q.elements} hexahedra, {q.invalid} invalid)   {fmt(t)}")
            t = timed(lambda: st.elevate(handles, el, 0, planes=False), repeats)
            lines.append(f"  K16 p {p} {dist:13s} report alone                                        {fmt(t)}")
        t = timed(lambda: st.block(handles, 0), repeats)
        lines.append(f"  K11 tm_stack_smoothers, all {LAYERS} layers ({3 * 8 * n * n * LAYERS / 1e9:.2f} GB of planes to the host)              {fmt(t)}")
        t = timed(lambda: st.quality(handles), repeats)
        lines.append(f"  K12 tm_stack_smoothers_quality ({(n - 1) ** 2 * (LAYERS - 1)} hexahedra)                          {fmt(t)}")
    finally:
        for h in handles:
            h.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out:
        with open(out, "w") as f:
            f.write(text)


def report(path, n, repeats, out):
    """Kernel times of the run above from rocprofv3's kernel trace: the launches are told apart by their order."""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    k16 = [d for _, d, name in rows if "k_stack_elevate" in name]
    k11 = [d for _, d, name in rows if "k_stack_planes" in name]
    k12 = [d for _, d, name in rows if "k_stack_quality<" in name or "k_stack_qualityI" in name]
    per = 1 + (1 + repeats) * 2   # per configuration: one report to print the counts, then planes + report and the report alone, warm-up included
    assert len(k16) == per * len(CONFIGS) and len(k11) == 1 + repeats and len(k12) == 1 + repeats, (len(k16), len(k11), len(k12))
    med = lambda v: statistics.median(v) * 1e-9   # noqa: E731
    nodes, cells = n * n * LAYERS, (n - 1) ** 2 * (LAYERS - 1)
    t11, t12 = med(k11[1:]), med(k12[1:])
    b11 = 24 * nodes
    lines = [f"kernel times of that run (rocprofv3 --kernel-trace, medians without the warm-up launch), {n}^2 nodes, {LAYERS} layers:",
             f"  K11 k_stack_planes   {t11 * 1e3:9.3f} ms   {b11 / t11 / 1e12:.3f} TB/s written   {t11 / b11 * 1e12:.3f} ps per byte written",
             f"  K12 k_stack_quality  {t12 * 1e3:9.3f} ms   {t12 / (8 * cells) * 1e12:.2f} ps per corner ({8 * cells} corners)"]
    for c, (p, dist) in enumerate(CONFIGS):
        mine = k16[c * per:(c + 1) * per]
        full, alone = med(mine[2:2 + repeats]), med(mine[3 + repeats:])
        corners = cells // p ** 3 * (p + 1) ** 3
        lines.append(f"  K16 p {p} {dist:13s} planes + report {full * 1e3:9.3f} ms   {full / b11 * 1e12:.3f} ps per byte written = {full / t11:.2f} x K11"
                     f"   | report alone {alone * 1e3:9.3f} ms   {alone / corners * 1e12:.2f} ps per node ({corners} nodes) = {alone / corners / (t12 / (8 * cells)):.2f} x K12 per corner")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out:
        with open(out, "a") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=N, help="nodes per direction of every cut (n - 1 a multiple of 4)")
    ap.add_argument("--repeats", type=int, default=REPEATS)
    ap.add_argument("--out", help="write (or, with --report, append) the lines to this file")
    ap.add_argument("--report", metavar="KERNEL_TRACE_CSV", help="no GPU: kernel times from the trace of a profiler run with the same --n and --repeats")
    args = ap.parse_args()
    if args.report:
        report(args.report, args.n, args.repeats, args.out)
    else:
        workload(args.n, args.repeats, args.out)


if __name__ == "__main__":
    main()
