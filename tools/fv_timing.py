"""Timing of the face-based view and the finite-volume metrics of the welded mesh (K21) beside the kernels they are measured against: K18's
order-1 cells launch (k_weld_cells), the 2-D quality report K9 (k_quality) and the 3-D one K12 (k_stack_quality).

Workload: configs.strip(8, 2048, 2048), three relaxation sweeps; --layers 0: the plane mesh (33.5 M cells, 67 M faces), --layers 3: the
welded plane repeated on 3 layers (67 M hexahedra).  Event pairs around the calls, 7 repeats after one warm-up call, median and min-max;
the calls of the face lists end in copies to the host that outweigh the kernels, so the KERNEL times come from separate profiler runs with
kernel tracing and statistics only, one per layer count:

    python tools/fv_timing.py --layers 0 [--out profiles/fv_timing.txt]                                           (needs the MI355X)
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o fv -- python tools/fv_timing.py --layers 0 --repeats 2 --no-host
    python tools/fv_timing.py --report <dir>/.../fv_kernel_trace.csv --layers 0 [--out ...]    (no GPU: reads the CSV, appends to --out)
    python tools/fv_timing.py --parity [--out profiles/fv_parity.txt]     largest |host - longdouble| / bar of the CPU tests (no GPU)

Bytes written by the face-list launches: per cell 8 (count and first face), per interior face 4 npf + 4 + 4 + 8 (ring, owner, neighbour, two
cell_faces slots), per boundary face 4 npf + 4 + 4.  Aims, reported as ratios, none a merge condition: the face-list launches per byte
written against k_weld_cells (16 B per cell written); the metrics passes per cell against K9 (plane) and per hexahedron against K12."""
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
FACE_LIST = (("k_fv_count", 1), ("k_weld_psum", 0), ("k_weld_pscan", 0), ("k_fv_interior", 1), ("k_weld_faces_lateral", 1), ("k_weld_faces_caps", -1), ("k_fv_boundary", 1))
METRICS = (("k_fv_cells", 1), ("k_fv_faces", 1), ("k_fv_final", 1))


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


def counts(nb, n, layers):
    eg = layers - 1 if layers >= 2 else 1
    cells = nb * (n - 1) ** 2 * eg
    boundary = (2 * (n - 1) + 2 * nb * (n - 1)) * eg + (2 * nb * (n - 1) ** 2 if layers >= 2 else 0)
    fpc, npf = (6, 4) if layers >= 2 else (4, 2)
    internal = (fpc * cells - boundary) // 2
    written = 8 * cells + internal * (4 * npf + 16) + boundary * (4 * npf + 8)
    return cells, internal, boundary, written


def workload(nb, n, layers, repeats, out, host=True):
    import numpy as np
    import torch  # noqa: F401  (the events; also loads the HIP runtime the library shares)

    from turbomesh_amd import configs, stack, weld
    from turbomesh_amd.smoothing import smooth, solver

    mesh = configs.strip(nb, n, n)
    cells, internal, boundary, _ = counts(nb, n, layers)
    lines = [f"faces and finite-volume metrics of configs.strip({nb}, {n}, {n}){f' on {layers} layers' if layers >= 2 else ''}: {cells} cells, {internal} internal and "
             f"{boundary} boundary faces (tools/fv_timing.py); event pairs around the calls, {repeats} repeats after a warm-up call.  The list calls end in copies to "
             "the host, which dominate: kernel times below, from the profiler run"]
    w = weld.Weld(mesh)
    with smooth.Smoother(mesh, solver.Option.hip(inner=solver.Inner.relax)) as sm:
        sm.iterate(3)
        o = [q.orientation for q in sm.quality()[0]]
        if layers < 2:
            rep = sm.fv_report(o)
            t = timed(lambda: sm.fv_report(o), repeats)
            lines.append(f"  tm_smoother_fv_report (K18 weld + K21 lists + metrics, the record to the host)   {fmt(t)}   min cos {rep.min_cos:.6f}, max skewness "
                         f"{rep.max_skewness:.6f}, {rep.negative_cells} cells with V <= 0, max closedness {rep.max_closedness:.3e}")
            t = timed(lambda: sm.quality(), repeats)
            lines.append(f"  tm_smoother_quality (K9 + finalize, the records to the host)                     {fmt(t)}")
        else:
            try:
                z = np.array([0.0, 0.125 * (layers - 1)])
                st = stack.Stack(z, stack.layers_from(z, layers), "linear", "planar")
                t = timed(lambda: st.quality([sm, sm]), repeats)
                lines.append(f"  tm_stack_smoothers_quality of the same plane as both cuts (K12 + finalize)      {fmt(t)}")
            except Exception as e:   # the comparison is then missing from the report, and says so
                lines.append(f"  tm_stack_smoothers_quality (K12): not measured ({type(e).__name__}: {e})")
        pts = w.points(sm)
    if layers >= 2:
        pts = np.vstack([np.column_stack([pts, np.full(len(pts), 0.125 * k)]) for k in range(layers)])
    nk = layers if layers >= 2 else None
    f = w.faces(nk, o)
    t = timed(lambda: w.faces(nk, o), max(1, repeats // 2))
    lines.append(f"  tm_weld_faces (map up, {f.faces.size + f.owner.size + f.neighbour.size + f.cell_faces.size} ids to the host; with the boundary plan)   {fmt(t)}")
    rd = f.metrics(pts)
    t = timed(lambda: f.metrics(pts), max(1, repeats // 2))
    lines.append(f"  tm_fv_metrics (lists and points up, the record to the host)                      {fmt(t)}")
    if layers < 2:   # K18's cells launch, measured alongside
        t = timed(lambda: w.cells(1), max(1, repeats // 2))
        lines.append(f"  tm_weld_cells order 1 (map up, {4 * cells} ids to the host)                          {fmt(t)}")
    if not host:
        print("\n".join(lines))
        return
    t0 = time.perf_counter()
    fh = weld.Weld(mesh, host=True).faces(nk, o)
    t1 = time.perf_counter()
    rh = fh.metrics(pts)
    t2 = time.perf_counter()
    same = all(np.array_equal(getattr(f, k), getattr(fh, k)) for k in ("faces", "owner", "neighbour", "cell_faces"))
    same = same and all(getattr(rd, k) == getattr(rh, k) for k in ("min_volume", "max_volume", "min_volume_cell", "max_closedness", "min_cos", "min_cos_face", "max_skewness",
                                                                   "max_skewness_face", "negative_cells", "nonorthogonal_faces", "inverted_faces"))
    lines.append(f"  host definition: tm_weld_faces_host {1e3 * (t1 - t0):9.1f} ms, tm_fv_metrics_host {1e3 * (t2 - t1):9.1f} ms (one run, wall clock); equal to the device: "
                 f"{'yes' if same else 'NO'}; total_volume device - host {rd.total_volume - rh.total_volume:.3e}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "a") as fh_:
            fh_.write(text)


def report(trace_csv, out, nb, n, layers):
    """Per-dispatch rows: per kernel the median of its dispatches times the dispatches of one call."""
    by_name = {}
    with open(trace_csv) as f:
        for r in csv.DictReader(f):
            name = re.sub(r"[<(].*", "", r["Kernel_Name"]).split("::")[-1].split(" ")[-1]
            by_name.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)   # microseconds
    cells, internal, boundary, written = counts(nb, n, layers)
    med = lambda name: statistics.median(by_name[name]) if by_name.get(name) else None
    lines = [f"kernel times of one rocprofv3 --kernel-trace --stats run of tools/fv_timing.py --layers {layers} (no counters), strip({nb}, {n}, {n}): per kernel the median "
             "dispatch x its dispatches per call"]
    calls = max(1, len(by_name.get("k_fv_count", [])))
    total_lists = 0.0
    for name, per_call in FACE_LIST:
        d = by_name.get(name, [])
        if not d:
            continue
        if per_call == 0:   # the scan launches are K18's: ALL their dispatches of the run over the face-list calls, the few of K18's own numbering included
            t = sum(d) / calls
            lines.append(f"    lists   {name:22s} {len(d):4d} dispatches  sum {sum(d):9.1f} us over {calls} calls (K18's numbering included: an upper bound) = {t:9.1f} us")
        else:
            per_call = nb if per_call < 0 else per_call
            t = statistics.median(d) * per_call
            lines.append(f"    lists   {name:22s} {len(d):4d} dispatches  median {statistics.median(d):9.1f} us  min {min(d):9.1f}  max {max(d):9.1f}   x {per_call} = {t:9.1f} us")
        total_lists += t
    lines.append(f"  K21 face lists: {total_lists:9.1f} us   {written / total_lists / 1e6:.2f} TB/s ({written} B written)")
    kc = med("k_weld_cells")
    if kc and layers < 2:
        tc = kc * nb
        ratio = (total_lists / written) / (tc / (16.0 * cells))
        lines.append(f"  K18 k_weld_cells x {nb}: {tc:9.1f} us   {16.0 * cells / tc / 1e6:.2f} TB/s (16 B per cell written); face lists per byte written: {ratio:.2f} x K18 cells "
                     f"(aim: parity) -- {'HIT' if ratio <= 1.05 else 'MISSED'}")
    total_metrics = 0.0
    for name, per_call in METRICS:
        d = by_name.get(name, [])
        if not d:
            continue
        t = statistics.median(d) * per_call
        total_metrics += t
        lines.append(f"    metrics {name:22s} {len(d):4d} dispatches  median {statistics.median(d):9.1f} us  min {min(d):9.1f}  max {max(d):9.1f}   x {per_call} = {t:9.1f} us")
    lines.append(f"  K21 metrics: {total_metrics:9.1f} us   {1e3 * total_metrics / cells:.4f} ns per cell")
    other = "k_stack_quality" if layers >= 2 else "k_quality"
    ko = med(other)
    if ko:   # one dispatch per block
        to = ko * nb
        ratio = total_metrics / to
        lines.append(f"  {'K12' if layers >= 2 else 'K9'} {other} x {nb}: {to:9.1f} us   {1e3 * to / cells:.4f} ns per cell; metrics per cell: {ratio:.2f} x "
                     f"{'K12' if layers >= 2 else 'K9'} (aim: parity) -- {'HIT' if ratio <= 1.05 else 'MISSED'}")
    else:
        lines.append(f"  {other}: no dispatch in the trace -- the ratio is not reported")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "a") as f:
            f.write(text)


def parity(out):
    """The largest observed error over its bar of the CPU tests' comparisons of the host definition with longdouble."""
    from tests import test_fv_faces_cpu as T
    from turbomesh_amd import configs

    lines = ["largest |host definition - longdouble| / bar over every per-cell and per-face value (tests/fv_reference.py: running first-order error bound; "
             "tools/fv_timing.py --parity)"]
    for name in sorted(T.INTERIOR):
        mesh, w, pts, o, ref, f = T.plane_case(name)
        lines.append(f"  {name:18s} {f.ncells:6d} cells {f.ninternal:6d} internal faces: {T.against_longdouble(f.metrics(pts, fields=True), ref, pts):.3f}")
    for nk, planar in ((3, True), (9, True), (9, False)):
        mesh = configs.two_by_two(9, 9, tfi=T.oracle_tfi)
        w, pts, o = T.stacked(mesh, nk, planar)
        ref = T.F.faces(mesh, w.map, nk, o)
        f = w.faces(layers=nk, orientation=o)
        lines.append(f"  two_by_two x {nk} {'planar' if planar else 'warped':6s} {f.ncells:6d} cells {f.ninternal:6d} internal faces: "
                     f"{T.against_longdouble(f.metrics(pts, fields=True), ref, pts):.3f}")
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
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=REPEATS)
    ap.add_argument("--no-host", action="store_true", help="skip the host definition (the profiler run)")
    args = ap.parse_args()
    if args.report:
        report(args.report, args.out, args.blocks, args.size, args.layers)
    elif args.parity:
        parity(args.out)
    else:
        workload(args.blocks, args.size, args.layers, args.repeats, args.out, not args.no_host)


if __name__ == "__main__":
    main()
