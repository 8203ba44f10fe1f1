"""Timing of the weld (K18: link, number, points, cells) beside the export transpose (k_soa_planes, K8), which moves the same coordinates.

Workload: configs.strip(8, 2048, 2048) resident in one handle (33.5 M nodes, 7 interfaces of 2048 pairs), three relaxation sweeps; in one
run tm_smoother_weld (link + number + points of the resident coordinates, X and Y to the host), tm_smoother_export_soa of the eight blocks
(K8, x and y to the host), tm_weld_cells at order 1 (map up, 134 M ids down) and the host definition (tm_weld_map_host, tm_weld_points_host on
the downloaded planes).  Event pairs around the calls, 7 repeats after one warm-up call, median and min-max; the calls end in copies to the
host that outweigh the kernels, so the KERNEL times come from one separate profiler run with kernel tracing and statistics only:

    python tools/weld_timing.py [--out profiles/weld_timing.txt]                                               (needs the MI355X)
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o weld -- python tools/weld_timing.py --repeats 3   (needs the MI355X)
    python tools/weld_timing.py --report <dir>/.../weld_kernel_trace.csv [--out ...]     (no GPU: reads the CSV, appends to --out)
    python tools/weld_timing.py --parity [--out profiles/weld_parity.txt]     max_gap of the example meshes as written (needs the MI355X)

Algorithmic bytes per node: number 4 (map written; the flags are computed, not stored), points 16 read + 16 written + 4 of map read,
K8 16 + 16; cells 4 (p+1)^2 per cell written.  Aim: the points gather at parity with K8 per byte."""
import argparse
import csv
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NBLOCKS, N, REPEATS = 8, 2048, 7


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


def workload(nb, n, repeats, out):
    import ctypes as C

    import numpy as np
    import torch  # noqa: F401  (the events; also loads the HIP runtime the library shares)

    from turbomesh_amd import _capi, configs, weld
    from turbomesh_amd.smoothing import smooth, solver

    L = _capi.lib()
    mesh = configs.strip(nb, n, n)
    nodes = nb * n * n
    lines = [f"weld of configs.strip({nb}, {n}, {n}) resident in one handle, {nodes} nodes (tools/weld_timing.py); event pairs around the calls, {repeats} repeats "
             "after a warm-up call.  Every call ends in copies to the host, which dominate: kernel times below, from the profiler run"]
    with smooth.Smoother(mesh, solver.Option.hip(inner=solver.Inner.relax)) as sm:
        sm.iterate(3)
        X, Y, rec = np.empty(nodes), np.empty(nodes), _capi.tm_weld_info()
        t = timed(lambda: _capi.check(L.tm_smoother_weld(sm._h, None, _capi.f64ptr(X), _capi.f64ptr(Y), C.byref(rec))), repeats)
        info = weld.WeldInfo.from_struct(rec)
        lines.append(f"  tm_smoother_weld (K18 link + number + points, X and Y to the host)   {fmt(t)}   {info.nodes_in} -> {info.nodes_out} nodes, "
                     f"{info.classes_2} classes of 2, max_gap {info.max_gap:.3e}")
        x, y = np.empty(n * n), np.empty(n * n)

        def export():
            for b in range(nb):
                _capi.check(L.tm_smoother_export_soa(sm._h, b, _capi.f64ptr(x), _capi.f64ptr(y), None, None))

        t = timed(export, repeats)
        lines.append(f"  tm_smoother_export_soa of the {nb} blocks (K8, x and y to the host)        {fmt(t)}")
        sm.download()
    w = weld.Weld(mesh)
    t = timed(lambda: w.cells(1), max(1, repeats // 2))
    lines.append(f"  tm_weld_cells order 1 (map up, {4 * nb * (n - 1) ** 2} ids to the host)               {fmt(t)}")
    t0 = time.perf_counter()
    wh = weld.Weld(mesh, host=True)
    t1 = time.perf_counter()
    ph = wh.points(mesh)
    t2 = time.perf_counter()
    same = np.array_equal(wh.map, w.map) and np.array_equal(ph[:, 0], X[:wh.nodes]) and np.array_equal(ph[:, 1], Y[:wh.nodes])
    lines.append(f"  host definition: tm_weld_map_host {1e3 * (t1 - t0):9.1f} ms, tm_weld_points_host {1e3 * (t2 - t1):9.1f} ms (one run, wall clock, with the "
                 f"transposes to planes in numpy); equal to the device: {'yes' if same else 'NO'}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


STAGES = (
    ("link", (("k_weld_init", 1), ("k_weld_hook", 1), ("k_weld_compress", 1), ("k_weld_classes", 1))),
    ("number", (("k_weld_count", 1), ("k_weld_psum", 1), ("k_weld_pscan", 2), ("k_weld_number", 1), ("k_weld_slaves", 1))),
    ("points", (("k_weld_gather_resident", 0), ("k_weld_gap", 1), ("k_weld_gap_final", 1))),
    ("cells", (("k_weld_cells", 0),)),
)


def report(trace_csv, out, nb, n):
    """Per-dispatch rows: per kernel the median of its dispatches times the dispatches of one call (the per-block kernels run once per
    block, the blocks are of one size)."""
    by_name = {}
    with open(trace_csv) as f:
        for r in csv.DictReader(f):
            name = re.sub(r"\(.*", "", r["Kernel_Name"]).split("::")[-1].split(" ")[-1]
            by_name.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)   # microseconds
    nodes = float(nb) * n * n
    cells = float(nb) * (n - 1) ** 2
    k8 = by_name.get("k_soa_planes", [])
    if not k8:
        sys.exit(f"{trace_csv}: no k_soa_planes dispatch")
    k8_call = statistics.median(k8) * nb
    lines = [f"kernel times of one rocprofv3 --kernel-trace --stats run of tools/weld_timing.py (no counters), strip({nb}, {n}, {n}): per kernel the median "
             "dispatch x its dispatches per call",
             f"  K8  k_soa_planes x {nb}: {k8_call:9.1f} us per mesh   {32 * nodes / k8_call / 1e6:.2f} TB/s (32 B per node)"]
    for stage, kernels in STAGES:
        total = 0.0
        for name, per_call in kernels:
            per_call = per_call or nb   # 0: once per block
            d = by_name.get(name, [])
            if not d:
                continue
            t = statistics.median(d) * per_call
            total += t
            lines.append(f"    {stage:6s} {name:24s} {len(d):4d} dispatches  median {statistics.median(d):9.1f} us  min {min(d):9.1f}  max {max(d):9.1f}   x {per_call} = {t:9.1f} us")
        if stage == "number":
            lines.append(f"  K18 number: {total:9.1f} us   {4 * nodes / total / 1e6:.2f} TB/s (4 B per node written)")
        elif stage == "points":
            g = statistics.median(by_name["k_weld_gather_resident"]) * nb
            ratio = (g / 36.0) / (k8_call / 32.0)
            lines.append(f"  K18 points: {total:9.1f} us, the gather {g:9.1f} us   {36 * nodes / g / 1e6:.2f} TB/s (36 B per node)   {ratio:.2f} x K8 per byte "
                         f"(aim: parity) -- {'HIT' if ratio <= 1.05 else 'MISSED'}")
        elif stage == "cells":
            lines.append(f"  K18 cells order 1: {total:9.1f} us   {16 * cells / total / 1e6:.2f} TB/s (16 B per cell written)")
        else:
            lines.append(f"  K18 {stage}: {total:9.1f} us")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "a") as f:
            f.write(text)


def parity(out):
    """max_gap of the example meshes as their files write them: linear, and at orders 2 and 5 with both node distributions."""
    from turbomesh_amd import _capi, highorder, weld
    from turbomesh_amd.input import Input
    from turbomesh_amd.smoothing import smooth, solver

    gold = os.path.join(ROOT, "tests", "golden")
    lines = ["max_gap (largest distance of a welded node's copies from its owner) of the example meshes smoothed as their files say (--hip: the device "
             "solver, the file's iterations and control function), from the coordinates resident in the handle (tools/weld_timing.py --parity)"]
    for name in ("T106", "LS89"):
        inp = Input.parse(open(os.path.join(gold, "examples", name, name + ".json")).read())
        inp.solver = solver.Option.hip(inner=solver.Inner.auto)
        mesh = inp.template.run(inp.geometry(gold))
        w = weld.Weld(mesh)
        with smooth.Smoother(mesh, inp.solver, inp.wall_control_function) as sm:
            sm.iterate(inp.iterations)
            w.points(sm)
            lines.append(f"  {name}: {w.info.nodes_in} -> {w.info.nodes_out} nodes, {inp.iterations} iterations; linear: max_gap {w.info.max_gap:.3e} at node "
                         f"{w.info.gap_node}, periodic_gap {w.info.periodic_gap:.3e}")
            for p in (2, 5):
                for dist in ("equidistant", "gauss_lobatto"):
                    try:
                        hom = highorder.Elevation(p, dist).mesh(sm)
                    except _capi.TmError as e:
                        lines.append(f"    order {p} {dist:13s}: {e.name} (the blocks are not on the element grid of this order)")
                        continue
                    w.points(hom)
                    lines.append(f"    order {p} {dist:13s}: max_gap {w.info.max_gap:.3e} at node {w.info.gap_node}, periodic_gap {w.info.periodic_gap:.3e}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--report", metavar="KERNEL_TRACE_CSV")
    ap.add_argument("--parity", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--blocks", type=int, default=NBLOCKS)
    ap.add_argument("--size", type=int, default=N)
    ap.add_argument("--repeats", type=int, default=REPEATS)
    args = ap.parse_args()
    if args.report:
        report(args.report, args.out, args.blocks, args.size)
    elif args.parity:
        parity(args.out)
    else:
        workload(args.blocks, args.size, args.repeats, args.out)


if __name__ == "__main__":
    main()
