"""Timing of the wall distance of the welded mesh (K20: table build, distance, record) beside its yardsticks, all measured in the same run.

Workloads: T106 as its file says (smoothed, 3 images, the blade = the unassigned patch); the O4H examples with every num_cells x 2
(as tools/dev/o4h_refined_probe.py builds them; the seeded mesh resident in a handle -- from x 3 on the template's tanh clustering of the
file's wall spacing has no solution, so the x 8 meshes cannot be built); one 4096 x 4096 block with its four sides as walls
(16 380 faces; a handle refuses listed wall conditions, so the two i-sides alone cannot be selected by kind); the same plane stacked to 5 layers with hub and shroud (--stacked; 83.9 M nodes, 67 M triangles).
Yardsticks: (a) the same launch with TM_WALL_NO_CULL and pairs_evaluated of both; (b) K9's quality report (tm_smoother_quality) on the
same handle, per node; (c) the host twin on one thread for T106.
Event pairs around the calls, 7 repeats after one warm-up call, median and min-max.  The calls end in copies to the host, so the KERNEL
times -- and the share of the table build against the distance launch -- come from one separate profiler run with kernel tracing and
statistics only (never combined with counters):

    python tools/wall_distance_timing.py [--out profiles/wall_distance_timing.txt] [--size 4096] [--stacked]            (needs the MI355X)
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o wd -- python tools/wall_distance_timing.py --repeats 2   (needs the MI355X)
    python tools/wall_distance_timing.py --report <dir>/.../wd_kernel_trace.csv [--out ...]      (no GPU: reads the CSV, appends to --out)"""
import argparse
import csv
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, REPEATS, FACTOR = 4096, 7, 2
GOLD = os.path.join(ROOT, "tests", "golden")


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


def example(name, factor):
    from turbomesh_amd.input import Input

    j = json.load(open(os.path.join(GOLD, "examples", name, name + ".json")))
    for k in j["template"]["O4H"]["num_cells"]:
        j["template"]["O4H"]["num_cells"][k] *= factor
    inp = Input.parse(json.dumps(j))
    return inp, inp.template.run(inp.geometry(GOLD))


def resident(lines, label, sm, repeats, kinds=None):
    """culled and not culled wall distance and the quality report of one handle"""
    res = {}
    o = [q.orientation for q in sm.quality()[0]]   # given, so that the call does not run the quality report itself
    tc = timed(lambda: res.__setitem__("c", sm.wall_distance(kinds, orientation=o)), repeats)
    tn = timed(lambda: res.__setitem__("n", sm.wall_distance(kinds, cull=False, orientation=o)), max(1, repeats // 2))
    tq = timed(lambda: sm.quality(), repeats)
    c, n = res["c"].info, res["n"].info
    same = (res["c"].distance == res["n"].distance).all() and (res["c"].face == res["n"].face).all() and (res["c"].image == res["n"].image).all()
    lines.append(f"  {label}: {c.points} nodes, {c.faces} faces, {c.primitives} primitives in {c.groups} groups, {c.images} image(s); on the wall {c.on_wall}, "
                 f"nearest to an image {c.nearest_via_image}, maximum {c.max_distance:.6e} at node {c.max_point}")
    lines.append(f"    tm_smoother_wall_distance, culled       {fmt(tc)}   pairs_evaluated {c.pairs_evaluated}")
    lines.append(f"    tm_smoother_wall_distance, NO_CULL      {fmt(tn)}   pairs_evaluated {n.pairs_evaluated}   "
                 f"(a) culling buys {statistics.median(tn) / statistics.median(tc):.2f} x in time, {n.pairs_evaluated / max(1, c.pairs_evaluated):.1f} x in pairs; equal results: "
                 f"{'yes' if same else 'NO'}")
    lines.append(f"    tm_smoother_quality (K9), same handle    {fmt(tq)}   (b) wall distance / quality per node, whole calls: "
                 f"{statistics.median(tc) / statistics.median(tq):.2f} x (the wall distance call also welds, lists the faces and copies three planes out)")
    return res["c"]


def workload(n, repeats, out, stacked):
    import numpy as np
    import torch  # noqa: F401  (the events; also loads the HIP runtime the library shares)

    from turbomesh_amd import configs, weld
    from turbomesh_amd.smoothing import smooth, solver

    lines = [f"wall distance of the welded mesh (tools/wall_distance_timing.py): event pairs around the calls, {repeats} repeats after a warm-up call.  The calls end in "
             "copies to the host; kernel times and the share of the table build are below, from the profiler run"]
    inp, mesh = example("T106", 1)
    with smooth.Smoother(mesh, solver.Option.hip(inner=solver.Inner.auto), inp.wall_control_function) as sm:
        sm.iterate(inp.iterations)
        got = resident(lines, f"T106 as its file says ({inp.iterations} iterations)", sm, repeats)
        w = weld.Weld(mesh)
        pts = w.points(sm)
        o = [q.orientation for q in sm.quality()[0]]
    t0 = time.perf_counter()
    host = weld.Weld(mesh, host=True).wall_distance(pts, w.boundary(1, orientation=o), host=True)
    t1 = time.perf_counter()
    same = np.array_equal(host.distance, got.distance) and np.array_equal(host.face, got.face) and np.array_equal(host.image, got.image)
    lines.append(f"    (c) host twin, one thread, all {host.info.pairs_evaluated} pairs: {1e3 * (t1 - t0):9.1f} ms (one run, wall clock); equal to the device: {'yes' if same else 'NO'}")
    for name in ("T106", "LS89"):
        inp, mesh = example(name, FACTOR)
        with smooth.Smoother(mesh, solver.Option.hip(inner=solver.Inner.relax)) as sm:
            resident(lines, f"{name} with every num_cells x {FACTOR} (seeded mesh)", sm, repeats)
    mesh = configs.single_block(n, n)   # a handle refuses listed wall conditions and the resident call selects by kind: all four sides are the wall
    with smooth.Smoother(mesh, solver.Option.hip(inner=solver.Inner.relax)) as sm:
        sm.iterate(3)
        resident(lines, f"single_block({n}, {n}), all four sides walls", sm, repeats)
        if stacked:
            w = weld.Weld(mesh)
            plane = w.points(sm)
            nk = 5
            pts = np.concatenate([np.concatenate([plane, np.full((len(plane), 1), 0.05 * k)], axis=1) for k in range(nk)])
            b = w.boundary(1, layers=nk)
            faces, index, images = b.wall_faces(("unassigned", "hub", "shroud"))
            res = {}
            tc = timed(lambda: res.__setitem__("c", weld.wall_distance_of(faces, pts, images)), max(1, repeats // 2))
            c = res["c"].info
            lines.append(f"  the same plane on {nk} layers, lateral faces, hub and shroud walls: {c.points} nodes, {c.faces} faces, {c.primitives} triangles in {c.groups} groups")
            lines.append(f"    tm_wall_distance, culled (faces and points up, three planes down)   {fmt(tc)}   pairs_evaluated {c.pairs_evaluated} of "
                         f"{c.points * c.primitives} (NO_CULL not run: {c.points * c.primitives:.2e} triangle tests)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


KERNELS = ("k_wall_table", "k_wall_chunks", "k_wall_distance", "k_wall_final", "k_quality", "k_quality_finalize")


def report(trace_csv, out):
    """Per dispatch of k_wall_distance (in launch order) the table build that precedes it: the share of the build against the distance launch."""
    rows = []
    with open(trace_csv) as f:
        for r in csv.DictReader(f):
            name = re.sub(r"[<(].*", "", r["Kernel_Name"]).split("::")[-1].split(" ")[-1]
            if name in KERNELS:
                rows.append((int(r["Start_Timestamp"]), name, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3, r.get("Grid_Size", r.get("Grid_Size_X", "?"))))
    rows.sort()
    lines = ["kernel times of one rocprofv3 --kernel-trace --stats run of tools/wall_distance_timing.py (no counters): per distinct launch shape the median over its "
             "dispatches, in microseconds; build = k_wall_table + k_wall_chunks before the distance launch"]
    shapes, build = {}, 0.0
    for _, name, us, grid in rows:
        if name in ("k_wall_table", "k_wall_chunks"):
            build += us
        elif name == "k_wall_distance":
            shapes.setdefault(("wall", grid, round(build, -1) if build > 100 else 0), []).append((build, us))
            build = 0.0
        elif name == "k_quality":
            shapes.setdefault(("quality", grid, 0), []).append((0.0, us))
    for (kind, grid, _), v in shapes.items():
        b, d = statistics.median(x[0] for x in v), statistics.median(x[1] for x in v)
        if kind == "wall":
            lines.append(f"  k_wall_distance grid {grid:>9s}: {len(v):3d} dispatches, median {d:12.1f} us (min {min(x[1] for x in v):12.1f}, max {max(x[1] for x in v):12.1f}); "
                         f"build {b:9.1f} us = {100.0 * b / (b + d):5.1f} % of build + distance")
        else:
            lines.append(f"  k_quality       grid {grid:>9s}: {len(v):3d} dispatches, median {d:12.1f} us")
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
    ap.add_argument("--stacked", action="store_true", help="also the 4096^2 plane on 5 layers with hub and shroud (about 20 GB on the device)")
    args = ap.parse_args()
    if args.report:
        report(args.report, args.out)
    else:
        workload(args.size, args.repeats, args.out, args.stacked)


if __name__ == "__main__":
    main()
