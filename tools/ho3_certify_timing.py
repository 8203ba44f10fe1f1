"""Timing of the certificate of high-order hexahedra (k_ho3_certify, K17) beside K16's report-only launch (k_stack_elevate without
planes), which the certificate runs first anyway, and beside the K11 window launches (k_stack_planes) that write the fine planes it reads.

Workload: 8 resident cuts of 2049^2 nodes, three relaxation sweeps each, cubic, planar, 33 layers; per order p = 2, 4
tm_stack_smoothers_certify at depth 2 (K16's report, then per window of span elements K11 and K17, the finalize, status and bounds to the
host) and tm_stack_smoothers_elevate without planes (K16's report + its pairs to the host).  Every element is proven at depth 0.  Host
clock around calls that end in a stream synchronise.  The KERNEL times, and with them the ratio K17 : K16-report the aim is about, come
from one profiler run with kernel tracing and statistics only, whose per-dispatch trace --report turns into times and the ratio:

    python tools/ho3_certify_timing.py [--out profiles/ho3_certify_timing.txt]                                          (needs the MI355X)
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o h3 -- python tools/ho3_certify_timing.py --repeats 2  (needs the MI355X)
    python tools/ho3_certify_timing.py --report <dir>/.../h3_kernel_trace.csv [--out ...]      (no GPU: reads the CSV, appends to --out)
    python tools/ho3_certify_timing.py --rough [--out ...]                                     (needs the MI355X: appends to --out)

--rough certifies one seeded block of 65 x 65 nodes and 17 layers from 3 cuts of 0.05-cells with uncorrelated node noise (0.3 cells at
order 2, 0.12 at order 4) at depths 0 .. 3: the case where subdivision matters, with the host clock around the calls.

Aim: where everything is decided at depth 0 (the smooth workload), K17 within the cost of K16's own report: ratio <= 1, the aim the 2-D
certificate had (and missed).  Nothing is asserted: the lines say HIT or MISSED and by how much."""
import argparse
import csv
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, CUTS, LAYERS, REPEATS, ORDERS, DEPTH = 2049, 8, 33, 3, (2, 4), 2


def timed(fn, repeats):
    fn()   # warm-up: code objects, buffers
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return f"median {statistics.median(t) * 1e3:9.3f} ms  min {min(t) * 1e3:9.3f}  max {max(t) * 1e3:9.3f}"


def emit(lines, out, mode):
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, mode) as f:
            f.write(text)


def workload(n, repeats, out):
    import numpy as np

    from turbomesh_amd import configs, highorder, stack
    from turbomesh_amd.smoothing import smooth, solver

    handles = [smooth.Smoother(configs.single_block(n, n, amplitude=0.05 + 0.001 * c), solver.Option.hip(inner=solver.Inner.relax)) for c in range(CUTS)]
    lines = [f"certificate of the hexahedra of {CUTS} resident cuts of {n}^2 nodes, cubic, planar, {LAYERS} layers, depth {DEPTH} (tm_stack_smoothers_certify: K16's "
             f"report, per window K11 and K17, the finalize, status and bounds to the host) beside K16's report alone (tm_stack_smoothers_elevate without planes); "
             f"host clock around the calls, {repeats} repeats after a warm-up call (tools/ho3_certify_timing.py).  Kernel times below, from the profiler run"]
    try:
        for h in handles:
            h.iterate(3)
        z = np.arange(CUTS, dtype=np.float64)
        st = stack.Stack(z, stack.layers_from(z, LAYERS), "cubic", "planar")
        for p in ORDERS:
            el = highorder.Elevation(p, "equidistant")
            lines.append(f"  K16 report   p {p}  {timed(lambda: st.elevate(handles, el, 0, planes=False), repeats)}")
            c = st.certify(handles, el, 0, max_depth=DEPTH)[0]
            lines.append(f"  certify      p {p}  {timed(lambda: st.certify(handles, el, 0, max_depth=DEPTH), repeats)}   {c.line('block')}")
    finally:
        for h in handles:
            h.close()
    emit(lines, out, "w")


def report(trace_csv, out, n):
    """Per-dispatch rows.  Per order: the k_ho3_certify<p> dispatches of one call summed (one per window of span elements) against one
    report-only k_stack_elevate<p, ...> dispatch, and the k_stack_planes dispatches of one certify call summed.  The dispatches of the
    first two calls of each kind (the call that fetched the record, and the warm-up) are left out."""
    with open(trace_csv) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3   # noqa: E731
    lines = [f"kernel times of one rocprofv3 --kernel-trace --stats run of tools/ho3_certify_timing.py (no counters), {CUTS} cuts of {n}^2 nodes, {LAYERS} layers; "
             "a certify call launches one K11 and one K17 per window of span elements: their dispatches are summed per call; warm-up calls left out"]
    for p in ORDERS:
        Eg = (LAYERS - 1) // p
        elements = ((n - 1) // p) ** 2 * Eg
        k16 = [us(r) for r in rows if re.search(rf"\bk_stack_elevate<{p},", r["Kernel_Name"])]
        k17 = [us(r) for r in rows if re.search(rf"\bk_ho3_certify<{p}>", r["Kernel_Name"])]
        if not k16 or not k17:
            sys.exit(f"{trace_csv}: no dispatches of order {p}")
        windows = None
        # the windows of a call: K17 dispatches come in runs between two k_stack_elevate dispatches of that order
        runs, cur, planes, cur_planes = [], [], [], []
        for r in rows:
            name = r["Kernel_Name"]
            if re.search(rf"\bk_ho3_certify<{p}>", name):
                cur.append(us(r))
            elif "k_stack_planes" in name and cur_planes is not None:
                cur_planes.append((us(r), int(r["Start_Timestamp"])))
            elif re.search(r"\bk_h3_finalize", name) and cur:
                runs.append(sum(cur))
                windows = len(cur)
                planes.append(sum(t for t, _ in cur_planes[-len(cur):]))
                cur, cur_planes = [], []
        runs, planes = (runs[2:], planes[2:]) if len(runs) > 2 else (runs, planes)
        # K16 dispatches: every certify call and every report call launches one; they cost the same, take them all but the first two
        k16 = k16[2:] if len(k16) > 2 else k16
        m16, m17, m11 = statistics.median(k16), statistics.median(runs), statistics.median(planes)
        ratio = m17 / m16
        lines.append(f"  p {p}  K16 report            {len(k16):2d} dispatches  median {m16 * 1e-3:9.3f} ms  min {min(k16) * 1e-3:9.3f}  max {max(k16) * 1e-3:9.3f}")
        lines.append(f"  p {p}  K11 windows ({windows:2d} per call) {len(planes):2d} calls  median {m11 * 1e-3:9.3f} ms  min {min(planes) * 1e-3:9.3f}  max {max(planes) * 1e-3:9.3f}")
        lines.append(f"  p {p}  K17 ({windows:2d} per call)         {len(runs):2d} calls  median {m17 * 1e-3:9.3f} ms  min {min(runs) * 1e-3:9.3f}  max {max(runs) * 1e-3:9.3f}   "
                     f"{m17 * 1e3 / elements:.2f} ns per element   K17 : K16-report = {ratio:.2f} (aim: at most 1) -- {'HIT' if ratio <= 1.0 else f'MISSED by {ratio:.1f} x'}")
    for label, pattern in (("k_hc_reduce   (records, first stage)", r"\bk_hc_reduce\("), ("k_h3_finalize (records -> tm_ho3_certificate)", r"\bk_h3_finalize\(")):
        hits = [us(r) for r in rows if re.search(pattern, r["Kernel_Name"])]
        if hits:
            lines.append(f"  {label:46s} {len(hits):3d} dispatches  median {statistics.median(hits):8.1f} us  min {min(hits):8.1f}  max {max(hits):8.1f}")
    emit(lines, out, "a")


def rough(out):
    import numpy as np

    from turbomesh_amd import configs, highorder, stack
    from turbomesh_amd.discrete import Mesh

    ni = nj = 65
    K, nk = 3, 17
    lines = [f"seeded rough block: {K} cuts of {ni} x {nj} nodes (0.05-cells, uniform node noise, numpy default_rng(2026 + cut)), cubic, planar, {nk} evenly spaced "
             "layers, certified on the device from host cuts (tm_stack_certify), host clock around the call after a warm-up call"]
    i, j = np.meshgrid(np.arange(ni, dtype=np.float64), np.arange(nj, dtype=np.float64), indexing="ij")
    z = np.arange(K, dtype=np.float64)
    st = stack.Stack(z, stack.layers_from(z, nk), "cubic", "planar")
    for p, amp in ((2, 0.3), (4, 0.12)):
        cuts = []
        for c in range(K):
            m = Mesh()
            m.addBlock("noise", configs.block_from_array(np.ascontiguousarray(0.05 * (np.stack([i, j], axis=-1) + np.random.default_rng(2026 + c).uniform(-amp, amp, (ni, nj, 2))))))
            cuts.append(m)
        el = highorder.Elevation(p, "equidistant")
        for depth in range(4):
            c = st.certify(cuts, el, 0, max_depth=depth)[0]
            share = "/".join(f"{100.0 * d / c.elements:.2f}" for d in c.decided_at)
            lines.append(f"  noise {amp} order {p} depth {depth}: {timed(lambda: st.certify(cuts, el, 0, max_depth=depth), 3)}   elements {c.elements} proven {c.proven} invalid "
                         f"{c.invalid} hidden invalid {c.hidden_invalid} undecided {c.undecided} ({100.0 * c.undecided / c.elements:.2f} %); decided at {share} %")
    emit(lines, out, "a")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--report", metavar="KERNEL_TRACE_CSV")
    ap.add_argument("--rough", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", type=int, default=N)
    ap.add_argument("--repeats", type=int, default=REPEATS)
    args = ap.parse_args()
    if args.report:
        report(args.report, args.out, args.size)
    elif args.rough:
        rough(args.out)
    else:
        workload(args.size, args.repeats, args.out)


if __name__ == "__main__":
    main()
