"""Timing of the high-order certificate (k_ho_certify, K14) beside K13's report-only launch (k_ho_elevate without planes), which the
certificate runs first anyway, and the share of elements decided per subdivision level on the example meshes.

Workload: one resident 4097^2 smooth block (4096 cells per direction: orders 2, 4 and 8 divide it), three relaxation sweeps; in one run,
per order p = 2, 4, 8, tm_smoother_certify (K13's report + K14 + finalize + status and bounds to the host) and tm_smoother_elevate without
planes (K13's report + its pairs to the host).  Event pairs around the calls, 7 repeats after one warm-up call, median and min-max.  The
KERNEL times, and with them the ratio K14 : K13-report the aim is about, come from one separate profiler run with kernel tracing and
statistics only, whose per-dispatch trace --report turns into microseconds and the ratio:

    python tools/ho_certify_timing.py [--out profiles/ho_certify_timing.txt]                                        (needs the MI355X)
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o hc -- python tools/ho_certify_timing.py --repeats 3   (needs the MI355X)
    python tools/ho_certify_timing.py --report <dir>/.../hc_kernel_trace.csv [--out ...]      (no GPU: reads the CSV, appends to --out)
    python tools/ho_certify_timing.py --examples tests/golden [--out ...]                     (needs the MI355X: appends to --out)

--examples also certifies a seeded 257^2 block of unit cells with uniform node noise of 0.35 cells (every coordinate a multiple of
1/256) at orders 2 and 4: the case where subdivision matters, and what the default depth 3 rests on.

The per-call lines are NOT comparable with each other: K13's report call copies one (Jmin, Jmax) pair per element into a fresh host
vector and divides them into the scaled Jacobians on the CPU (64 MB and 4 M divisions at p = 2), the certify call copies 17 B per
element into the caller's arrays.  Only the kernel times say what the kernels cost.

Aim: where nearly all elements are decided at depth 0 (this block), K14 within the cost of K13's own report: ratio <= 1.  Nothing is
asserted: the lines say HIT or MISSED and by how much."""
import argparse
import csv
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, REPEATS, ORDERS = 4097, 7, (2, 4, 8)


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


def emit(lines, out, mode):
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, mode) as f:
            f.write(text)


def workload(n, repeats, out):
    import torch  # noqa: F401  (the events; also loads the HIP runtime the library shares)

    from turbomesh_amd import configs, highorder
    from turbomesh_amd.smoothing import smooth, solver

    lines = [f"certificate of one resident {n}^2 smooth block (tm_smoother_certify: K13's report, K14, the finalizes, status and bounds to the host) beside "
             f"K13's report alone (tm_smoother_elevate without planes); event pairs around the calls, {repeats} repeats after a warm-up call "
             "(tools/ho_certify_timing.py).  The two lines of an order are not comparable: the K13 call forms one scaled Jacobian per element on the CPU from "
             "pairs copied into a fresh host vector, which outweighs its kernel; kernel times below, from the profiler run"]
    with smooth.Smoother(configs.single_block(n, n), solver.Option.hip(inner=solver.Inner.relax)) as sm:
        sm.iterate(3)
        for p in ORDERS:
            el = highorder.Elevation(p, "equidistant")
            t13 = timed(lambda: el.block(sm, 0, planes=False), repeats)
            c = sm.certify(el, 0)[0]
            t14 = timed(lambda: sm.certify(el, 0), repeats)
            lines.append(f"  K13 report   p {p}  {fmt(t13)}")
            lines.append(f"  certify      p {p}  {fmt(t14)}   {c.line('block')}")
    emit(lines, out, "w")


def report(trace_csv, out, n):
    """Per-dispatch rows: per order the k_ho_certify<p> dispatches against the k_ho_elevate<p> ones (all report-only in this workload);
    the first two dispatches of each are the call that fetched the record and timed()'s warm-up and are left out."""
    by_name = {}
    with open(trace_csv) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        by_name.setdefault(r["Kernel_Name"], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)   # microseconds

    def group(pattern):
        hits = [v for k, v in by_name.items() if re.search(pattern, k)]
        if len(hits) != 1:
            sys.exit(f"{trace_csv}: {len(hits)} kernels match {pattern}")
        return hits[0][2:] if len(hits[0]) > 2 else hits[0]

    lines = [f"kernel times of one rocprofv3 --kernel-trace --stats run of tools/ho_certify_timing.py (no counters), {n}^2 nodes, per dispatch, warm-up dispatches left out"]
    for p in ORDERS:
        k13, k14 = group(rf"\bk_ho_elevate<{p}>"), group(rf"\bk_ho_certify<{p}>")
        m13, m14 = statistics.median(k13), statistics.median(k14)
        elements = ((n - 1) // p) ** 2
        ratio = m14 / m13
        lines.append(f"  p {p}  K13 report {len(k13):2d} dispatches  median {m13:9.1f} us  min {min(k13):9.1f}  max {max(k13):9.1f}")
        lines.append(f"  p {p}  K14        {len(k14):2d} dispatches  median {m14:9.1f} us  min {min(k14):9.1f}  max {max(k14):9.1f}   {m14 * 1e3 / elements:.2f} ns per element   "
                     f"K14 : K13-report = {ratio:.2f} (aim: at most 1) -- {'HIT' if ratio <= 1.0 else f'MISSED by {ratio:.1f} x'}")
    for label, pattern in (("k_hc_reduce   (records, first stage)", r"\bk_hc_reduce\("), ("k_hc_finalize (records -> tm_ho_certificate)", r"\bk_hc_finalize\(")):
        hits = [v for k, v in by_name.items() if re.search(pattern, k)]
        if hits:
            lines.append(f"  {label:46s} {len(hits[0]):3d} dispatches  median {statistics.median(hits[0]):8.1f} us  min {min(hits[0]):8.1f}  max {max(hits[0]):8.1f}")
    emit(lines, out, "a")


def examples(root, out):
    """T106 and LS89 as their input files say, smoothed with the hip solver; the certificate at orders 2 and 5 and depths 3 and 4."""
    from turbomesh_amd import highorder
    from turbomesh_amd.input import Input
    from turbomesh_amd.smoothing import smooth, solver

    lines = ["example meshes, smoothed as their input files say (hip solver, inner strategy auto): elements decided per subdivision level (0/1/2/3/4), per cent of all"]
    for name in ("T106", "LS89"):
        cwd = os.getcwd()
        os.chdir(root)   # profile files are named relative to the working directory
        try:
            inp = Input.parse(open(os.path.join("examples", name, name + ".json")).read())
            mesh = inp.template.run(inp.geometry(os.getcwd()))
        except Exception as e:
            lines.append(f"  {name}: not built here: {e}")
            continue
        finally:
            os.chdir(cwd)
        with smooth.Smoother(mesh, solver.Option.hip()) as sm:
            sm.iterate(inp.iterations)
            for p in (2, 5):
                el = highorder.Elevation(p, "equidistant")
                try:
                    el.check(mesh)
                except Exception as e:   # the order does not divide a block of this example
                    lines.append(f"  {name} order {p}: {e}")
                    continue
                nodal = el.mesh(sm).total
                for depth in (3, 4):
                    c = sm.certify(el, max_depth=depth)[0]
                    share = "/".join(f"{100.0 * d / c.elements:.2f}" for d in c.decided_at)
                    lines.append(f"  {name} order {p} depth {depth}: elements {c.elements} nodal invalid {nodal.invalid} proven {c.proven} invalid {c.invalid} hidden invalid "
                                 f"{c.hidden_invalid} undecided {c.undecided}; decided at {share} %; min scaled bound {c.min_scaled_bound:.4f} "
                                 f"(nodal min scaled jacobian {nodal.min_scaled_jacobian:.4f})")
    import numpy as np

    from turbomesh_amd import configs
    from turbomesh_amd.discrete import Mesh

    n = 257
    rng = np.random.default_rng(2025)
    i, j = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    X = np.round((np.stack([i, j], axis=-1) + rng.uniform(-0.35, 0.35, (n, n, 2))) * 256) / 256
    noisy = Mesh()
    noisy.addBlock("noise", configs.block_from_array(np.ascontiguousarray(X)))
    lines.append(f"seeded {n}^2 block of unit cells, uniform node noise of 0.35 cells (numpy default_rng(2025), multiples of 1/256), certified on the device (tm_ho_certify)")
    for p in (2, 4):
        el = highorder.Elevation(p, "equidistant")
        for depth in (3, 4):
            c = el.certify(noisy, 0, max_depth=depth)[0]
            share = "/".join(f"{100.0 * d / c.elements:.2f}" for d in c.decided_at)
            lines.append(f"  noise order {p} depth {depth}: elements {c.elements} proven {c.proven} invalid {c.invalid} hidden invalid {c.hidden_invalid} "
                         f"undecided {c.undecided} ({100.0 * c.undecided / c.elements:.2f} %); decided at {share} %")
    emit(lines, out, "a")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--report", metavar="KERNEL_TRACE_CSV")
    ap.add_argument("--examples", metavar="GOLDEN_DIR")
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", type=int, default=N)
    ap.add_argument("--repeats", type=int, default=REPEATS)
    args = ap.parse_args()
    if args.report:
        report(args.report, args.out, args.size)
    elif args.examples:
        examples(args.examples, args.out)
    else:
        workload(args.size, args.repeats, args.out)


if __name__ == "__main__":
    main()
