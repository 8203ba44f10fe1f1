"""Timing of the boundary of the welded mesh (K19: k_weld_faces_lateral, k_weld_faces_caps, k_weld_faces_measure, k_weld_faces_final) beside
the K18 kernels with the same access patterns: k_weld_cells (the caps' store pattern) and k_weld_gather (a gather through the map).

Workload: configs.strip(8, 2048, 2048) welded (33.5 M nodes), its order-1 cells (k_weld_cells), its welded points from host planes
(k_weld_gather), then the boundary across 33 layers at order 1 -- 2 x 33.5 M cap faces and the perimeter times 32 lateral faces
(tm_weld_boundary_faces) -- and its measures on the planar stack of the welded plane (tm_weld_faces_measure).  The calls end in copies to
and from the host that outweigh the kernels (wall clock, one run each), so the KERNEL times come from one separate profiler run with kernel
tracing and statistics only, no counters:

    python tools/weld_boundary_timing.py [--out profiles/weld_boundary_timing.txt]                                     (needs the MI355X)
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o wb -- python tools/weld_boundary_timing.py        (needs the MI355X)
    python tools/weld_boundary_timing.py --report <dir>/.../wb_kernel_trace.csv [--out ...]   (no GPU: reads the CSV, appends to --out)

Algorithmic bytes: k_weld_cells and k_weld_faces_caps write 16 B per quadrilateral (the caps two per plane element); k_weld_gather reads
16 B of coordinates and 4 B of map per node; k_weld_faces_measure reads per face 16 B of ids, 4 B of patch and four corners of 24 B.
Aims: the caps per byte written within 1.25 x k_weld_cells; the measure is held against k_weld_gather per byte read, the ratio written down."""
import argparse
import csv
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NBLOCKS, N, LAYERS = 8, 2048, 33


def workload(nb, n, nk, out):
    import numpy as np
    import torch  # noqa: F401  (loads the HIP runtime the library shares)

    from turbomesh_amd import configs, weld

    def clock(fn):
        t0 = time.perf_counter()
        r = fn()
        return r, 1e3 * (time.perf_counter() - t0)

    mesh = configs.strip(nb, n, n)
    w, t_map = clock(lambda: weld.Weld(mesh))
    lines = [f"boundary of the welded configs.strip({nb}, {n}, {n}) across {nk} layers at order 1 (tools/weld_boundary_timing.py): wall clock of one call each, "
             "copies to and from the host included -- they dominate; kernel times below, from the profiler run",
             f"  tm_weld_map                          {t_map:10.1f} ms   {w.info.nodes_in} -> {w.nodes} nodes"]
    pts, t = clock(lambda: w.points(mesh))
    lines.append(f"  tm_weld_points (k_weld_gather)       {t:10.1f} ms")
    cells, t = clock(lambda: w.cells(1))
    lines.append(f"  tm_weld_cells order 1                {t:10.1f} ms   {len(cells)} quadrilaterals")
    del cells
    b, t = clock(lambda: w.boundary(1, layers=nk))
    i = b.info
    lines.append(f"  tm_weld_boundary_faces               {t:10.1f} ms   {i.faces} faces: {i.lateral_faces} lateral, {i.cap_faces} on the caps, {i.patches} patches")
    p3 = [np.tile(pts[:, 0], nk), np.tile(pts[:, 1], nk), np.repeat(0.01 * np.arange(nk), w.nodes)]   # the planar stack of the welded plane, as planes
    patches, t = clock(lambda: b.measure(p3))
    lines.append(f"  tm_weld_faces_measure                {t:10.1f} ms")
    again = b.measure(p3)
    lines.append(f"  a second call gives the same bits: {'yes' if again == patches else 'NO'}")
    for q, r in enumerate(patches):
        lines.append(f"    patch {q} {r.name:10s} {r.faces:9d} faces  measure {r.measure:.15e}  normal ({r.normal[0]:+.3e}, {r.normal[1]:+.3e}, {r.normal[2]:+.3e})  moment {r.moment:+.15e}")
    lines.append(f"  sum of the normals ({sum(r.normal[0] for r in patches):+.3e}, {sum(r.normal[1] for r in patches):+.3e}, {sum(r.normal[2] for r in patches):+.3e}), "
                 f"sum of the moments / 3 = {sum(r.moment for r in patches) / 3:.15e} (the strip is {nb} x 1 x {0.01 * (nk - 1):g})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


def report(trace_csv, out, nb, n, nk):
    by_name = {}
    with open(trace_csv) as f:
        for r in csv.DictReader(f):
            name = re.sub(r"\(.*", "", r["Kernel_Name"]).split("::")[-1].split(" ")[-1]
            by_name.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)   # microseconds
    need = ("k_weld_cells", "k_weld_gather", "k_weld_faces_caps", "k_weld_faces_lateral", "k_weld_faces_measure", "k_weld_faces_final")
    missing = [k for k in need if k not in by_name]
    if missing:
        sys.exit(f"{trace_csv}: no dispatch of {missing}")
    nodes, cells = float(nb) * n * n, float(nb) * (n - 1) ** 2
    lateral = (2.0 * (n - 1) + 2.0 * nb * (n - 1)) * (nk - 1)
    faces = 2 * cells + lateral
    med = {k: statistics.median(v) for k, v in by_name.items()}
    lines = [f"kernel times of one rocprofv3 --kernel-trace --stats run of tools/weld_boundary_timing.py (no counters), strip({nb}, {n}, {n}) x {nk} layers, order 1: "
             "per kernel the median dispatch (per-block kernels: x the blocks)"]
    for k in need:
        d = by_name[k]
        lines.append(f"    {k:24s} {len(d):4d} dispatches  median {med[k]:10.1f} us  min {min(d):10.1f}  max {max(d):10.1f}")
    t_cells, t_caps = med["k_weld_cells"] * nb, med["k_weld_faces_caps"] * nb
    per_cells, per_caps = t_cells / (16 * cells), t_caps / (32 * cells)
    ratio = per_caps / per_cells
    lines.append(f"  K18 k_weld_cells x {nb}:      {t_cells:10.1f} us   {16 * cells / t_cells / 1e6:.2f} TB/s written (16 B per cell)")
    lines.append(f"  K19 k_weld_faces_caps x {nb}: {t_caps:10.1f} us   {32 * cells / t_caps / 1e6:.2f} TB/s written (2 x 16 B per plane element)   {ratio:.2f} x k_weld_cells per byte "
                 f"written (aim: <= 1.25) -- {'MET' if ratio <= 1.25 else 'MISSED'}")
    lines.append(f"  K19 k_weld_faces_lateral:    {med['k_weld_faces_lateral']:10.1f} us   {lateral:.0f} faces: perimeter-sized")
    # the gather of the profiler run is the one-layer call on the plane mesh: the largest dispatches of that name
    t_gather = max(by_name["k_weld_gather"])
    per_gather, per_measure = t_gather / (20 * nodes), med["k_weld_faces_measure"] / (116 * faces)
    lines.append(f"  K18 k_weld_gather:           {t_gather:10.1f} us   {20 * nodes / t_gather / 1e6:.2f} TB/s read (20 B per node)")
    lines.append(f"  K19 k_weld_faces_measure:    {med['k_weld_faces_measure']:10.1f} us   {116 * faces / med['k_weld_faces_measure'] / 1e6:.2f} TB/s requested (116 B per face; every "
                 f"point is asked for by four faces)   {per_measure / per_gather:.2f} x k_weld_gather per byte read (no ratio fixed in advance)")
    lines.append(f"  K19 k_weld_faces_final:      {med['k_weld_faces_final']:10.1f} us")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "a") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--report", metavar="KERNEL_TRACE_CSV")
    ap.add_argument("--out", default=None)
    ap.add_argument("--blocks", type=int, default=NBLOCKS)
    ap.add_argument("--size", type=int, default=N)
    ap.add_argument("--layers", type=int, default=LAYERS)
    args = ap.parse_args()
    if args.report:
        report(args.report, args.out, args.blocks, args.size, args.layers)
    else:
        workload(args.blocks, args.size, args.layers, args.out)


if __name__ == "__main__":
    main()
