"""CPU: the host definition of the face-based view of the welded mesh and of its finite-volume metrics (tm_weld_faces_plan,
tm_weld_faces_host, tm_fv_metrics_host; turbomesh_amd.weld with host=True) against tests/fv_reference.py -- faces, owner, neighbour and
cell_faces equal exactly, known interior counts, the reference-free properties of an upper-triangular face list, rings, partition
invariance, analytic grids, a fold, every value against longdouble, the polyMesh round trip, errors, struct sizes.

Every bar is the running first-order error bound of tests/fv_reference.py (class EV): the rounding of every
operation of the definition, propagated in its order.  No other tolerance appears."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests import fv_reference as F
from tests import test_weld_boundary_cpu as bcpu
from tests import test_weld_cpu as cpu
from tests import weld_boundary_reference as B
from tests.conftest import oracle_tfi
from turbomesh_amd import _capi, configs, output, stack, weld
from turbomesh_amd.discrete import Mesh

LD = np.longdouble
INTERIOR = {"T106": 47570, "LS89": 71375, "two_by_two": 418, "strip_reversed": 493, "periodic_channel": 172, "plate": 412, "cut": 1268, "polar_ring": 253}
VALID = ["cut", "strip_reversed", "plate", "two_by_two", "polar_ring"]
LISTS = ("faces", "owner", "neighbour", "cell_faces")


@functools.lru_cache(maxsize=None)
def plane_case(name):
    """(mesh, Weld(host), welded points, orientation, reference lists, host Faces) -- built once, never modified"""
    mesh, w, ref_map, _, _ = cpu.case(name)
    o = bcpu.orientation_of(name)
    return mesh, w, bcpu.plane_case(name)[2], o, F.faces(mesh, ref_map, 0, o), w.faces(orientation=o)


def same_lists(f, ref):
    for k in LISTS:
        got = getattr(f, k)
        assert got.dtype == np.int32 and got.shape == ref[k].shape and np.array_equal(got, ref[k]), k
    assert f.ninternal == ref["ninternal"] == len(f.neighbour)


def upper_triangular(f):
    """the properties a solver relies on, without the reference"""
    own, nb = f.owner[:f.ninternal].astype(np.int64), f.neighbour.astype(np.int64)
    assert (np.diff(own) >= 0).all() and (nb > own).all()
    same = np.diff(own) == 0
    assert (np.diff(nb)[same] >= 0).all()                      # inside one owner the neighbours ascend
    fpc = f.cell_faces.shape[1]
    assert np.array_equal(np.bincount(np.concatenate([f.owner, f.neighbour]), minlength=f.ncells), np.full(f.ncells, fpc))   # 4 (6) faces per cell
    cf = f.cell_faces.astype(np.int64)
    cell = np.arange(f.ncells)[:, None]
    other = np.concatenate([nb, np.full(len(f.faces) - f.ninternal, -1)])
    assert ((f.owner[cf] == cell) | (other[cf] == cell)).all()
    assert len(np.unique(cf)) == len(f.faces)                  # every face is named, an interior one twice
    assert (np.sort(cf[f.owner[cf] != cell]) == np.arange(f.ninternal)).all()
    for r in f.boundary.patches:
        assert f.ninternal + r.begin >= f.ninternal
    assert np.array_equal(f.faces[f.ninternal:], f.boundary.faces)


def ratio(got, ev):
    """largest |host - longdouble| / bar; a zero bar asks for equality"""
    err = np.abs(np.asarray(got, dtype=LD) - ev.v).astype(np.float64)
    bar = ev.bar()
    assert (err <= bar).all(), (float(err.max()), float(bar.max()))
    return float(np.max(np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), 0.0))) if err.size else 0.0


def against_longdouble(rep, ref, pts):
    """every per-cell and per-face value and every field of the record; -> the largest observed / bar"""
    M = F.metrics(ref, pts)
    dim = 2 if ref["faces"].shape[1] == 2 else 3
    worst = max(ratio(rep.volume, M["volume"]), ratio(rep.closedness, M["closedness"]), ratio(rep.cos, M["cos"]), ratio(rep.skewness, M["skewness"]))
    for c in range(dim):
        worst = max(worst, ratio(rep.centre[:, c], M["centre"][c]), ratio(rep.area[:, c], M["area"][c]), ratio(rep.face_centre[:, c], M["face_centre"][c]))
    ni = ref["ninternal"]
    assert (rep.cells, rep.internal_faces, rep.boundary_faces) == (len(ref["cell_faces"]), ni, len(ref["faces"]) - ni)
    # extremes: |min a - min b| <= max |a_i - b_i|, and the cell named holds the reference's extreme within its bar
    for value, index, ev, largest in ((rep.min_volume, rep.min_volume_cell, M["volume"], False), (rep.max_volume, rep.max_volume_cell, M["volume"], True),
                                      (rep.max_closedness, rep.max_closedness_cell, M["closedness"], True), (rep.min_cos, rep.min_cos_face, M["cos"], False),
                                      (rep.max_skewness, rep.max_skewness_face, M["skewness"], True)):
        want, _ = F.extreme(ev, largest)
        bar = float(np.nanmax(ev.bar()))
        assert abs(float(LD(value) - want)) <= bar and abs(float(ev.v[index] - want)) <= 2 * bar
    # counts: exact unless a value lies within its bar of the threshold
    def between(got, ev, limit, inclusive):
        lo = int(np.sum(ev.v + ev.bar() <= limit) if inclusive else np.sum(ev.v + ev.bar() < limit))
        hi = int(np.sum(ev.v - ev.bar() <= limit) if inclusive else np.sum(ev.v - ev.bar() < limit))
        assert lo <= got <= hi, (lo, got, hi)
    between(rep.negative_cells, M["volume"], 0.0, True)
    between(rep.inverted_faces, M["cos"], 0.0, True)
    between(rep.nonorthogonal_faces, M["cos"].take(np.arange(ni)), F.COS_70, False)
    if rep.negative_cells:
        sure = np.flatnonzero(M["volume"].v + M["volume"].bar() <= 0)
        maybe = np.flatnonzero(M["volume"].v - M["volume"].bar() <= 0)
        assert maybe[0] <= rep.first_negative_cell <= (sure[0] if len(sure) else maybe[-1])
    total, bar = F.total_volume(M["volume"])
    assert abs(float(LD(rep.total_volume) - total)) <= bar
    return worst


@pytest.mark.parametrize("name", sorted(cpu.TABLE))
def test_every_topology_of_the_table(name):
    mesh, w, pts, o, ref, f = plane_case(name)
    same_lists(f, ref)
    upper_triangular(f)
    assert f.ninternal == INTERIOR[name] and len(f.faces) - f.ninternal == bcpu.KNOWN[name][0]
    assert f.ninternal == (4 * f.ncells - bcpu.KNOWN[name][0]) // 2
    plan = _capi.tm_fv_plan()
    _capi.check(_capi.lib().tm_weld_faces_plan(w._md.ref(), 0, C.byref(plan)))
    assert (plan.cells, plan.internal_faces, plan.boundary_faces, plan.nodes_per_face, plan.faces_per_cell) == (f.ncells, f.ninternal, bcpu.KNOWN[name][0], 2, 4)
    worst = against_longdouble(f.metrics(pts, fields=True), ref, pts)
    print(f"{name}: {f.ninternal} interior faces, largest |host - longdouble| / bar = {worst:.3f}")


@pytest.mark.parametrize("name", VALID)
def test_normals_point_from_owner_to_neighbour_and_cells_close(name):
    mesh, w, pts, o, ref, f = plane_case(name)
    rep = f.metrics(pts, fields=True)
    d = rep.centre[f.neighbour] - rep.centre[f.owner[:f.ninternal]]
    assert (np.sum(rep.area[:f.ninternal] * d, axis=1) > 0).all()
    assert rep.negative_cells == 0 and rep.inverted_faces == 0 and rep.min_volume > 0
    M = F.metrics(ref, pts)
    assert (rep.closedness <= M["closedness"].v.astype(np.float64) + M["closedness"].bar()).all()
    # closed in exact arithmetic: the reference's value is its own 2^-64 rounding, 2^-11 of the fp64 bound, and the bar alone bounds the host's
    assert (M["closedness"].v.astype(np.float64) <= M["closedness"].bar() * 2.0 ** -10).all()
    assert rep.max_closedness <= float(M["closedness"].bar().max()) < 1e-15


def stacked(mesh, nk, planar=True):
    w = weld.Weld(mesh, host=True)
    if planar:
        blocks = bcpu.planar_blocks(mesh, nk)
    else:
        blocks = [tuple(np.stack([p * (1.0 + k / 17.0) if c < 2 else p + k / 7.0 + 0.01 * X * k for k in range(nk)]) for c, p in enumerate((X, Y, np.zeros_like(X))))
                  for X, Y in cpu.R.mesh_planes(mesh)]
    o = tuple(stack.quality_of_planes(*blk).orientation for blk in blocks)
    return w, w.points(blocks), o


@pytest.mark.parametrize("case", ["two_by_two_3", "two_by_two_9", "flipped_strip_3", "two_by_two_9_warped"])
def test_stacked_meshes(case):
    mesh = configs.strip(3, 9, 12, reverse_odd=True, tfi=oracle_tfi) if case.startswith("flipped") else configs.two_by_two(9, 9, tfi=oracle_tfi)
    nk, planar = int(case.split("_")[-2 if case.endswith("warped") else -1]), not case.endswith("warped")
    w, pts, o = stacked(mesh, nk, planar)
    if case.startswith("flipped"):
        assert sorted(set(o)) == [-1, 1]
    ref = F.faces(mesh, w.map, nk, o)
    f = w.faces(layers=nk, orientation=o)
    same_lists(f, ref)
    upper_triangular(f)
    assert f.faces.shape[1] == 4 and f.cell_faces.shape[1] == 6 and f.ncells == len(w.cells(1, layers=nk))
    assert f.ninternal == (6 * f.ncells - len(f.boundary.faces)) // 2
    rep = f.metrics(pts, fields=True)
    worst = against_longdouble(rep, ref, pts)
    print(f"{case}: {f.ninternal} interior faces, largest |host - longdouble| / bar = {worst:.3f}")
    d = rep.centre[f.neighbour] - rep.centre[f.owner[:f.ninternal]]
    assert (np.sum(rep.area[:f.ninternal] * d, axis=1) > 0).all() and rep.negative_cells == 0
    if not planar:
        return
    # planar faces: sum V = K19's sum of moments / 3 = area x span, each within the bars of its two sides
    M = F.metrics(ref, pts)
    total, bar = F.total_volume(M["volume"])
    sums, abss, mags, terms = B.measures(f.boundary.faces, f.boundary.face_patch, len(f.boundary.patches), pts, 1, True)
    kbar = B.bar_against_reference(terms, abss, mags, True)[:, 4].sum() / 3
    moments = B.values_of(f.boundary.measure(pts)).astype(LD)[:, 4].sum() / 3
    # the reference volumes against the reference moments: identical in exact arithmetic, 2^-64 roundings apart -- inside either bar
    assert abs(float(LD(rep.total_volume) - moments)) <= bar + kbar + abs(float(total - sums[:, 4].sum() / 3))
    assert abs(float(total - sums[:, 4].sum() / 3)) <= bar + kbar
    w2 = weld.Weld(mesh, host=True)
    pts2 = w2.points(mesh)
    o2 = tuple(q.orientation for q in mesh.quality(host=True)[0])
    area, area_mag = B.signed_cell_areas(mesh, w2.map, pts2, o2)
    span = LD(0.125) * (nk - 1)
    ref_bar = float(area_mag) * (4 * len(w2.cells(1)) + 4) * 2.0 ** -64 * float(span)
    assert abs(float(LD(rep.total_volume) - area * span)) <= bar + ref_bar + abs(float(total - area * span))
    assert abs(float(total - area * span)) <= bar + kbar + ref_bar


def test_a_ring_two_cells_around_keeps_both_faces_of_a_pair():
    mesh = cpu.polar_ring(7, 3)
    w = weld.Weld(mesh, host=True)
    for o in ((1,), (-1,)):
        # the two circumferential edges at one radius join the SAME two nodes, so node sets cannot tell the faces apart: this case is
        # checked by its properties and not against the reference
        f = w.faces(orientation=o)
        pairs = list(zip(f.owner[:f.ninternal].tolist(), f.neighbour.tolist()))
        twice = sorted({p for p in pairs if pairs.count(p) == 2})
        assert len(twice) == 6 and twice == [(e, e + 6) for e in range(6)]
        for own, nb in twice:   # ordered by the owner's side
            two = [t for t, p in enumerate(pairs) if p == (own, nb)]
            sides = [int(np.flatnonzero(f.cell_faces[own] == t)[0]) for t in two]
            assert two[1] == two[0] + 1 and sides == sorted(sides) == [0, 1]
        upper_triangular(f)


def test_a_ring_one_cell_around_is_refused():
    mesh = cpu.polar_ring(7, 2)
    w = weld.Weld(mesh, host=True)
    with pytest.raises(F.OwnNeighbour):
        F.faces(mesh, w.map, 0, (1,))
    with pytest.raises(_capi.TmError) as e:
        w.faces(orientation=(1,))
    assert e.value.code == _capi.TM_E_MISMATCH and "block 0, side" in str(e.value)


def test_partition_invariance_of_the_cut_grid():
    mesh, w, pts, o, ref, f = plane_case("cut")
    single = Mesh()
    single.addBlock("whole", configs.block_from_array(cpu.warped_grid(23, 31)))
    w1 = weld.Weld(single, host=True)
    pts1 = w1.points(single)
    f1 = w1.faces(orientation=(1,))
    assert f1.ninternal == f.ninternal == 1268

    def triples(ff, ww, p):
        cells = ww.cells(1)
        key = lambda ids: frozenset(map(tuple, p[np.asarray(ids)].tolist()))
        return {(key(cells[a]), key(cells[b]), key(row)) for a, b, row in zip(ff.owner[:ff.ninternal], ff.neighbour, ff.faces[:ff.ninternal])}

    def unordered(t):
        return {(frozenset((a, b)), r) for a, b, r in t}

    # owner and neighbour are cell NUMBERS, which the partition changes: the pair and the face are what is invariant
    assert unordered(triples(f, w, pts)) == unordered(triples(f1, w1, pts1))
    ra, rb = f.metrics(pts, fields=True), f1.metrics(pts1, fields=True)
    Ma, Mb = F.metrics(ref, pts), F.metrics(F.faces(single, w1.map, 0, (1,)), pts1)
    for name, key in (("min_cos", "cos"), ("max_skewness", "skewness")):
        assert abs(getattr(ra, name) - getattr(rb, name)) <= float(np.max(Ma[key].bar()) + np.max(Mb[key].bar()))
    assert abs(ra.total_volume - rb.total_volume) <= F.total_volume(Ma["volume"])[1] + F.total_volume(Mb["volume"])[1]


def grid_mesh(xy):
    m = Mesh()
    m.addBlock("b", configs.block_from_array(np.ascontiguousarray(xy)))
    return m


def test_sheared_grid_has_one_angle_no_skewness_and_equal_volumes():
    s, h, k = 0.5, 1.0 / 16, 1.0 / 8
    u, v = np.meshgrid(h * np.arange(13), k * np.arange(10), indexing="ij")   # multiples of 2^-4 and 2^-3: the nodes are exact
    mesh = grid_mesh(np.stack([u + s * v, v], axis=2))
    w = weld.Weld(mesh, host=True)
    pts = w.points(mesh)
    ref = F.faces(mesh, w.map, 0, (1,))
    f = w.faces(orientation=(1,))
    same_lists(f, ref)
    rep = f.metrics(pts, fields=True)
    M = F.metrics(ref, pts)
    ni = f.ninternal
    # faces across j (normal along the sheared direction) see the centres in line: cos = 1 / sqrt(1 + s^2); faces across i: cos = 1 / sqrt(1 + s^2) too
    want = 1 / np.sqrt(LD(1) + LD(s) * LD(s))
    assert (np.abs(rep.cos[:ni].astype(LD) - want).astype(np.float64) <= M["cos"].bar()[:ni] + np.abs(M["cos"].v[:ni] - want).astype(np.float64)).all()
    assert (np.abs(M["cos"].v[:ni] - want).astype(np.float64) <= M["cos"].bar()[:ni]).all()
    assert (rep.skewness <= M["skewness"].bar()).all() and (np.abs(M["skewness"].v).astype(np.float64) <= M["skewness"].bar()).all()
    assert (np.abs(rep.volume - h * k) <= M["volume"].bar()).all()
    assert rep.nonorthogonal_faces == 0 and rep.inverted_faces == 0


def test_a_fold_is_counted_and_named():
    xy = cpu.warped_grid(9, 11).copy()
    xy[4, 5] = xy[6, 5] + (xy[6, 5] - xy[5, 5]) * 0.5   # an interior node moved across its neighbour and beyond the next one
    mesh = grid_mesh(xy)
    w = weld.Weld(mesh, host=True)
    pts = w.points(mesh)
    ref = F.faces(mesh, w.map, 0, (1,))
    f = w.faces(orientation=(1,))
    same_lists(f, ref)
    rep = f.metrics(pts, fields=True)
    against_longdouble(rep, ref, pts)
    M = F.metrics(ref, pts)
    bad = np.flatnonzero(M["volume"].v <= 0)
    assert rep.negative_cells >= 1 and rep.negative_cells == len(bad) and rep.first_negative_cell == bad[0]
    assert rep.inverted_faces >= 1 and rep.inverted_faces == int(np.sum(M["cos"].v <= 0)) and rep.min_cos < 0


def test_polymesh_round_trip_and_cyclic_partners(tmp_path):
    mesh = cpu.case("periodic_channel")[0]
    w = weld.Weld(mesh, host=True)   # its own: points() updates info
    nk = 2
    blocks = bcpu.planar_blocks(mesh, nk, 1.0)
    o = tuple(stack.quality_of_planes(*blk).orientation for blk in blocks)
    pts = w.points(blocks)
    f = w.faces(layers=nk, orientation=o)
    d = str(tmp_path / "polyMesh")
    files = output.write_polymesh(d, pts, f, empty_caps=True)
    assert sorted(os.path.basename(p) for p in files) == ["boundary", "faces", "neighbour", "owner", "points"]
    got = output.read_polymesh(d)
    assert np.array_equal(got["points"], pts) and np.array_equal(got["faces"], f.faces)
    assert np.array_equal(got["owner"], f.owner) and np.array_equal(got["neighbour"], f.neighbour)
    at = f.ninternal
    names = [p["name"] for p in got["boundary"]]
    assert len(set(names)) == len(names) == len(f.boundary.patches)
    for p, r in zip(got["boundary"], f.boundary.patches):
        assert (p["startFace"], p["nFaces"], p["name"]) == (at, r.faces, r.name)   # contiguous from ninternal on
        at += p["nFaces"]
        assert p["type"] == output.polymesh_patch_type(r.kind, True)
    assert at == len(f.faces)
    assert [p["type"] for p in got["boundary"]].count("empty") == 2 and [p["type"] for p in got["boundary"]].count("cyclic") == 2
    by_name = {p["name"]: p for p in got["boundary"]}
    for p in got["boundary"]:
        if p["type"] != "cyclic":
            continue
        q = by_name[p["neighbourPatch"]]
        assert q["neighbourPatch"] == p["name"] and q["nFaces"] == p["nFaces"] and p["transform"] == "translational"
        sep = np.array(p["separationVector"])
        assert np.array_equal(sep, -np.array(q["separationVector"])) and sep.any()
        for t in range(p["nFaces"]):   # face t of one side + translation = face t of the other: node (a, c) is the image of node (1 - a, c),
            a = got["points"][got["faces"][p["startFace"] + t]] + sep           # within the gap the weld reports for the periodic pairs
            b = got["points"][got["faces"][q["startFace"] + t]][[1, 0, 3, 2]]
            assert np.abs(a - b).max() <= w.info.periodic_gap + 2.0 ** -53 * np.abs(b).max()   # + the rounding of this one addition
    with pytest.raises(ValueError):
        output.write_polymesh(d, w.points(mesh), w.faces(orientation=o))   # a plane mesh has edges, not quadrilaterals


def test_struct_sizes():
    assert (C.sizeof(_capi.tm_fv_plan), C.sizeof(_capi.tm_fv_info), C.sizeof(_capi.tm_fv_fields)) == (40, 144, 56)


def test_errors():
    L = _capi.lib()
    mesh, w, pts, o, ref, f = plane_case("two_by_two")
    md = w._md.ref()
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.tm_weld_faces_plan(md, 0, None) == _capi.TM_E_ARG
    for fn in (L.tm_weld_faces_host, L.tm_weld_faces):   # NULL pointers are refused before anything is read or launched
        assert fn(md, None, w.nodes, 0, None, i32(f.faces), i32(f.owner), i32(f.neighbour), None) == _capi.TM_E_ARG
        assert fn(md, i32(w.map), w.nodes, 0, None, None, i32(f.owner), i32(f.neighbour), None) == _capi.TM_E_ARG
        assert fn(md, None, 2 ** 31, 0, None, None, None, None, None) == _capi.TM_E_ARG
    planes = [np.ascontiguousarray(pts[:, c]) for c in range(2)]
    arr = (C.POINTER(C.c_double) * 2)(*[_capi.f64ptr(a) for a in planes])
    rec = _capi.tm_fv_info()
    args = lambda faces=f.faces, owner=f.owner, nb=f.neighbour, cf=f.cell_faces: (2, f.ncells, f.ninternal, len(f.faces) - f.ninternal, i32(faces), i32(owner), i32(nb),
                                                                                i32(cf), len(pts), arr, None, C.byref(rec))
    for fn in (L.tm_fv_metrics_host, L.tm_fv_metrics):   # all of these are refused by the host-side check, before any launch
        assert fn(*args()[:4], None, *args()[5:]) == _capi.TM_E_ARG
        assert fn(4, *args()[1:]) == _capi.TM_E_ARG
        bad = f.faces.copy()
        bad[17, 1] = len(pts)
        assert fn(*args(faces=bad)) == _capi.TM_E_ARG and b"point" in L.tm_last_error()
        bad = f.owner.copy()
        bad[[3, 4]] = bad[[4, 3]] if bad[3] != bad[4] else (bad[4] + 1, bad[3])
        bad[5], bad[6] = 9, 2
        assert fn(*args(owner=bad)) == _capi.TM_E_ARG
        bad = f.neighbour.copy()
        bad[0] = f.owner[0]
        assert fn(*args(nb=bad)) == _capi.TM_E_ARG
        bad = f.cell_faces.copy()
        bad[0, 0] = len(f.faces)
        assert fn(*args(cf=bad)) == _capi.TM_E_ARG
    assert L.tm_fv_metrics_host(*args()) == _capi.TM_OK and rec.cells == f.ncells


def test_polymesh_flags_that_do_not_go_together_are_errors(capsys):
    from turbomesh_amd.__main__ import main

    cfg = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "examples", "T106", "T106.json")
    for extra, word in ((["--weld", "--output", "t.vtk", "--polymesh", "d", "--order", "2"], "--order"), (["--polymesh", "d", "--output", "t.xyz"], "--weld"),
                        (["--fv-report"], "--weld"), (["--weld", "--output", "t.vtk", "--polymesh", "d", "--polymesh-thickness", "0"], "--polymesh-thickness")):
        with pytest.raises(SystemExit) as e:   # refused while the arguments are read: nothing is meshed
            main([cfg, "--hip"] + extra)
        assert e.value.code not in (0, None)
        assert word in capsys.readouterr().err
