"""Timing of the 3-D quality report of stacked blocks (k_stack_quality, K12) beside what a user did before it existed and beside the 2-D
report (k_quality, K9).

Workload: 8 resident cuts of 2048^2 (config 5: amplitude 0.05 + 0.001 c, one handle per cut), cubic, planar, 33 layers.  In one run:
  1. tm_stack_smoothers_quality: the report straight from the cuts;
  2. the same answer the old way: tm_stack_smoothers for all layers in windows of 4 (K11 writes the block, 24 B per node and layer, which
     then crosses to the host) plus tm_quality3d_planes_host on the result (--host: evaluated once, it takes the CPU many seconds);
  3. tm_smoother_quality (K9) on one of the handles.
Every call ends in a stream synchronise inside the library, so the times are host-clock times around whole calls: 7 repeats after one
warm-up call, median and min-max.  Kernel times come from ONE separate profiler run with kernel tracing and statistics only:

    python tools/stack_quality_timing.py [--host] [--out profiles/stack_quality_timing.txt]                     (needs the MI355X)
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o sq -- python tools/stack_quality_timing.py --repeats 3          (needs the MI355X)
    python tools/stack_quality_timing.py --report <dir>/.../sq_kernel_stats.csv [--out ...]   (no GPU: reads the CSV, appends to --out)

Counted per hexahedron (K12, from the shapes): 16 K B read per node (x 1.14 for the tile seams), 4 K - 2 multiply-adds of the node position,
about 280 further fp64 additions and multiplications (12 edge vectors, 3 edge lengths, eight 3 x 3 determinants, the volume's three), 10
IEEE divisions (8 corners, volume, aspect) and 3 square roots (each edge once)."""
import argparse
import csv
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, CUTS, LAYERS, WINDOW, REPEATS = 2048, 8, 33, 4, 7
FLOPS_PER_CELL = 280 + 4 * CUTS - 2          # additions and multiplications, none fused
DIVS_PER_CELL, ROOTS_PER_CELL = 10, 3
FP64_VECTOR_OPS = 256 * 4 * 16 * 2.4e9       # MI355X: 256 CUs x 4 SIMDs x 16 fp64 lanes per clock x 2.4 GHz = 39.3e12 un-fused operations/s
HBM_PEAK = 8.0e12


def timed(fn, repeats):
    fn()   # warm-up: code objects, buffers
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return statistics.median(t), min(t), max(t)


def fmt(t):
    return f"{t[0] * 1e3:.3f} ms ({t[1] * 1e3:.3f}-{t[2] * 1e3:.3f})"


def workload(n, repeats, host, out):
    import numpy as np

    from turbomesh_amd import configs, stack
    from turbomesh_amd.smoothing import smooth, solver

    handles = [smooth.Smoother(configs.single_block(n, n, amplitude=0.05 + 0.001 * c), solver.Option.hip(inner=solver.Inner.relax)) for c in range(CUTS)]
    lines = [f"3-D quality report of {CUTS} resident cuts of {n}^2, cubic, planar, {LAYERS} layers ({(n - 1) ** 2 * (LAYERS - 1)} hexahedra); host clock around "
             f"calls that end in a stream synchronise, {repeats} repeats after a warm-up call: median (min-max)"]
    try:
        for h in handles:
            h.iterate(3)
        z = np.arange(CUTS, dtype=np.float64)
        st = stack.Stack(z, stack.layers_from(z, LAYERS), "cubic", "planar")
        windows = [(k, min(WINDOW, LAYERS - k)) for k in range(0, LAYERS, WINDOW)]
        q = st.quality(handles)[0][0]
        t1 = timed(lambda: st.quality(handles), repeats)
        lines.append(f"  1. tm_stack_smoothers_quality (K12 + finalize, one 192 B record to the host)          {fmt(t1)}")
        t2 = timed(lambda: [st.block(handles, 0, k, c) for k, c in windows], repeats)
        lines.append(f"  2. tm_stack_smoothers, {len(windows)} windows of up to {WINDOW} layers (K11 + the planes to the host)      {fmt(t2)}")
        if host:
            planes = [np.concatenate(p) for p in zip(*[st.block(handles, 0, k, c) for k, c in windows])]
            t0 = time.perf_counter()
            hq = stack.quality_of_planes(*planes)
            th = time.perf_counter() - t0
            same = all(getattr(hq, f) == getattr(q, f) for f in ("cells", "inverted", "degenerate", "orientation", "min_scaled_jacobian", "worst_i", "worst_j",
                                                                 "worst_k", "max_aspect", "max_growth_k", "min_volume", "max_volume", "hist"))
            lines.append(f"     + tm_quality3d_planes_host on the {3 * planes[0].nbytes / 1e9:.2f} GB it returned (one CPU thread, once)   {th:.2f} s; "
                         f"every field but total_volume equal to the device's: {'yes' if same else 'NO'}")
        t3 = timed(lambda: handles[0].quality(), repeats)
        lines.append(f"  3. tm_smoother_quality of one cut (K9 + finalize)                                        {fmt(t3)}")
        lines.append(f"  record: inverted {q.inverted} degenerate {q.degenerate} min scaled jacobian {q.min_scaled_jacobian:.4f} max aspect {q.max_aspect:.2f} "
                     f"max growth k {q.max_growth_k:.4f}")
    finally:
        for h in handles:
            h.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


def report(stats_csv, out, n):
    pats = {"K12": re.compile(r"\bk_stack_quality<"), "K11": re.compile(r"\bk_stack_planes<"), "K9": re.compile(r"\bk_quality\(")}
    rows = {}
    with open(stats_csv) as f:
        for r in csv.DictReader(f):
            for key, pat in pats.items():
                if pat.search(r["Name"]):
                    rows[key] = r
    missing = [k for k in pats if k not in rows]
    if missing:
        sys.exit(f"{stats_csv}: no kernel rows for {missing}")
    avg = {k: float(r["AverageNs"]) * 1e-9 for k, r in rows.items()}
    span = {k: (float(r["MinNs"]) * 1e-6, float(r["MaxNs"]) * 1e-6, int(r["Calls"])) for k, r in rows.items()}
    cells3 = float(n - 1) ** 2 * (LAYERS - 1)
    cells2 = float(n - 1) ** 2
    nwin = (LAYERS + WINDOW - 1) // WINDOW
    k11_all = avg["K11"] * nwin
    per_corner_12, per_corner_9 = avg["K12"] / (8 * cells3), avg["K9"] / (4 * cells2)
    bytes12 = 16.0 * CUTS * n * n * (16.0 / 15.0) ** 2
    t_ops = cells3 * (FLOPS_PER_CELL + DIVS_PER_CELL + ROOTS_PER_CELL) / FP64_VECTOR_OPS   # a division or root counted as ONE operation: a floor
    t_bytes = bytes12 / HBM_PEAK
    lines = [
        f"kernel times of one rocprofv3 --kernel-trace --stats run of tools/stack_quality_timing.py (no counters), every launch of the run averaged, {n}^2, {CUTS} cuts, {LAYERS} layers",
        *[f"  {k:4s} {rows[k]['Name'][:60]:60s} {span[k][2]:3d} calls  average {avg[k] * 1e3:9.3f} ms  min {span[k][0]:9.3f}  max {span[k][1]:9.3f}" for k in ("K12", "K11", "K9")],
        f"  K12 against the K11 launches that write the block it describes ({nwin} windows): {avg['K12'] * 1e3:.3f} ms against {k11_all * 1e3:.3f} ms = "
        f"{avg['K12'] / k11_all:.2f} x (aim: below 1) -- {'HIT' if avg['K12'] < k11_all else 'MISSED'}",
        f"  per corner: K12 {per_corner_12 * 1e12:.2f} ps per hexahedron corner, K9 {per_corner_9 * 1e12:.2f} ps per quadrilateral corner: ratio {per_corner_12 / per_corner_9:.2f}",
        f"  bounds of K12 from the shapes: {FLOPS_PER_CELL} additions and multiplications + {DIVS_PER_CELL} divisions + {ROOTS_PER_CELL} square roots per hexahedron, "
        f"each counted as one fp64 vector operation, over 39.3e12 operations/s = {t_ops * 1e3:.3f} ms; {bytes12 / 1e6:.0f} MB over the 8 TB/s HBM peak = {t_bytes * 1e3:.3f} ms; "
        f"the kernel takes {avg['K12'] / t_ops:.1f} x the operation floor and {avg['K12'] / t_bytes:.1f} x the byte floor: the {'operation' if t_ops > t_bytes else 'byte'} "
        f"floor is the larger one (an IEEE division or square root is a sequence of a dozen operations, counted here as one); {bytes12 / avg['K12'] / 1e12:.2f} TB/s of reads",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "a") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--report", metavar="KERNEL_STATS_CSV")
    ap.add_argument("--out", default=None)
    ap.add_argument("--host", action="store_true", help="also evaluate the block K11 wrote on the CPU (tm_quality3d_planes_host), once")
    ap.add_argument("--size", type=int, default=N)
    ap.add_argument("--repeats", type=int, default=REPEATS)
    args = ap.parse_args()
    if args.report:
        report(args.report, args.out, args.size)
    else:
        workload(args.size, args.repeats, args.host, args.out)


if __name__ == "__main__":
    main()
