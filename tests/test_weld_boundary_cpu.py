"""CPU: the host definition of the boundary of the welded mesh (tm_weld_boundary_plan, tm_weld_boundary_faces_host,
tm_weld_faces_measure_host; turbomesh_amd.weld with host=True) against tests/weld_boundary_reference.py -- known face counts, faces,
patches and origin equal exactly, the reference-free edge rule, orientation (closure of the normals, enclosed area and volume), matched
periodic faces, errors, the file round trip, the struct sizes.

The bar of every measured value: 2 (n - 1) 2^-53 sum |t| for the order of the sums, plus c 2^-53 sum M for the
rounding of a term, M the magnitude of the products a term is formed from and c counted from its operations
(weld_boundary_reference.C_PLANE / C_STACKED).  No other tolerance appears."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

from tests import test_weld_cpu as cpu
from tests import weld_boundary_reference as B
from tests.conftest import oracle_tfi
from turbomesh_amd import _capi, configs, output, stack, weld
from turbomesh_amd.boundary import Condition, ConditionTag, Range, Side

LD = np.longdouble

# name -> (faces, {kind: faces} or None for "all unassigned", loops)
KNOWN = {
    "T106": (860, {"unassigned": 340, "periodic": 300, "inlet": 90, "outlet": 130}, 2),
    "LS89": (1250, {"unassigned": 540, "periodic": 290, "inlet": 180, "outlet": 240}, 2),
    "two_by_two": (60, None, 1),
    "strip_reversed": (70, None, 1),
    "periodic_channel": (40, {"periodic": 24, "inlet": 8, "unassigned": 8}, 1),
    "plate": (72, None, 1),
    "cut": (104, None, 1),
    "polar_ring": (46, None, 2),
}
KIND_NAMES = {0: "wall", 1: "inlet", 2: "outlet", 16: "periodic", 17: "unassigned", 18: "hub", 19: "shroud"}


@functools.lru_cache(maxsize=None)
def orientation_of(name):
    """o_b of the quality report (host), per block"""
    return tuple(q.orientation for q in cpu.case(name)[0].quality(host=True)[0])


@functools.lru_cache(maxsize=None)
def plane_case(name, order=1):
    """(mesh, Weld(host), welded points, reference boundary, reference measures) -- built once, never modified."""
    mesh, w, ref_map, _, _ = cpu.case(name)
    o = orientation_of(name)
    pts = weld.Weld(mesh, host=True).points(mesh)
    ref = B.boundary(mesh, ref_map, order, 0, o)
    return mesh, w, pts, ref, B.measures(ref["faces"], ref["face_patch"], len(ref["patches"]), pts, order, False)


def same_patches(got, want):
    assert len(got) == len(want)
    for g, r in zip(got, want):
        assert (g.kind, g.source, g.partner, g.translation, g.begin, g.faces) == (r["kind"], r["source"], r["partner"], r["translation"], r["begin"], r["faces"])


def same_boundary(b, ref):
    assert b.faces.dtype == np.int32 and b.faces.shape == ref["faces"].shape and np.array_equal(b.faces, ref["faces"])
    assert np.array_equal(b.face_patch, ref["face_patch"]) and np.array_equal(b.origin, ref["origin"])
    same_patches(b.patches, ref["patches"])
    assert b.info.faces == len(ref["faces"]) and b.info.patches == len(ref["patches"])


def within(got, want, bar):
    err = np.abs(np.asarray(got, dtype=LD) - want).astype(np.float64)
    assert (err <= bar).all(), (err, bar)


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers_and_the_reference(name):
    mesh, w, pts, ref, _ = plane_case(name)
    faces, by_kind, loops = KNOWN[name]
    b = w.boundary(1, orientation=orientation_of(name))
    same_boundary(b, ref)
    assert (b.info.faces, b.info.nodes_per_face, b.info.lateral_faces, b.info.cap_faces) == (faces, 2, faces, 0) and b.cell_type == 3
    assert (b.info.loops, b.info.irregular_nodes) == (loops, 0) == (ref["loops"], ref["irregular"])
    got = {}
    for r in b.patches:
        got[KIND_NAMES[r.kind]] = got.get(KIND_NAMES[r.kind], 0) + r.faces
    assert {k: v for k, v in got.items() if v} == (by_kind or {"unassigned": faces})
    assert b.patches[-1].kind == _capi.TM_PATCH_UNASSIGNED
    # reference-free: the faces are the edges that lie in exactly one cell of the welded order-1 mesh
    assert {(min(a, c), max(a, c)) for a, c in b.faces.tolist()} == B.one_cell_edges(mesh, w.map) and len(b.faces) == len(B.one_cell_edges(mesh, w.map))


def test_t106_names_and_partners():
    _, w, _, _, _ = plane_case("T106")
    b = w.boundary(1)
    assert [r.name for r in b.patches] == ["inlet", "outlet", "periodic18a", "periodic18b", "periodic19a", "periodic19b", "periodic20a", "periodic20b", "unassigned"]
    for q, r in enumerate(b.patches):
        if r.kind == _capi.TM_PATCH_PERIODIC:
            o = b.patches[r.partner]
            assert o.partner == q and o.source == r.source and o.faces == r.faces and o.translation == (-r.translation[0], -r.translation[1])
    assert sum(len(a) for a, _, _ in b.periodic_faces()) == 150


def test_t106_at_order_5():
    mesh, w, pts, ref, ms = plane_case("T106", 5)
    b = w.boundary(5, orientation=orientation_of("T106"))
    assert b.faces.shape == (172, 6) and b.cell_type == 68
    same_boundary(b, ref)
    sums, abss, mags, terms = ms
    within(B.values_of(b.measure(pts)), sums, B.bar_against_reference(terms, abss, mags, False))
    assert int(terms.sum()) == 860   # the fine edges are those of order 1


def planar_blocks(mesh, nk, dz=0.125):
    return [tuple(np.stack([p if c < 2 else p + k * dz for k in range(nk)]) for c, p in enumerate((X, Y, np.zeros_like(X)))) for X, Y in cpu.R.mesh_planes(mesh)]


@functools.lru_cache(maxsize=None)
def stacked_case(order):
    """two_by_two(9, 9) x 9 layers, the layers scaled and lifted so that no face is degenerate: (mesh, Weld, blocks, points, orientation, ref, measures)"""
    mesh = configs.two_by_two(9, 9, tfi=oracle_tfi)
    w = weld.Weld(mesh, host=True)
    blocks = [tuple(np.stack([p * (1.0 + k / 17.0) if c < 2 else p + k / 7.0 + 0.01 * X * k for k in range(9)]) for c, p in enumerate((X, Y, np.zeros_like(X))))
              for X, Y in cpu.R.mesh_planes(mesh)]
    o = tuple(stack.quality_of_planes(*blk).orientation for blk in blocks)
    pts = w.points(blocks)
    ref = B.boundary(mesh, w.map, order, 9, o)
    return mesh, w, blocks, pts, o, ref, B.measures(ref["faces"], ref["face_patch"], len(ref["patches"]), pts, order, True)


@pytest.mark.parametrize("order", [1, 2, 4])
def test_stacked_two_by_two_on_nine_layers(order):
    mesh, w, blocks, pts, o, ref, (sums, abss, mags, terms) = stacked_case(order)
    b = w.boundary(order, layers=9, orientation=o)
    same_boundary(b, ref)
    E = 8 // order
    # 8 E segments x E span elements; 4 E^2 elements per cap
    assert b.info.lateral_faces == 8 * E * E and b.info.cap_faces == 2 * 4 * E * E and b.faces.shape[1] == (order + 1) ** 2
    if order == 2:
        assert (b.info.lateral_faces, b.info.cap_faces, b.faces.shape) == (128, 128, (256, 9))
    assert [r.kind for r in b.patches] == [_capi.TM_PATCH_UNASSIGNED, _capi.TM_PATCH_HUB, _capi.TM_PATCH_SHROUD]
    assert b.cell_type == (9 if order == 1 else 70)
    assert np.array_equal(np.unique(b.origin[:, 1]), np.arange(6))
    within(B.values_of(b.measure(pts)), sums, B.bar_against_reference(terms, abss, mags, True))
    # the boundary of the hexahedra: every face's corner ring is a face of exactly one cell
    cells = w.cells(1, layers=9)
    quads = {}
    for c in cells.tolist():
        for f in ((0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 5, 4), (1, 2, 6, 5), (2, 3, 7, 6), (3, 0, 4, 7)):
            k = tuple(sorted(c[i] for i in f))
            quads[k] = quads.get(k, 0) + 1
    if order == 1:
        assert {tuple(sorted(r)) for r in b.faces.tolist()} == {k for k, n in quads.items() if n == 1}


def closure(name, orientation, order=1):
    """(sum of the patch normals, sum of the moments / 2 - oriented cell areas, their bars) of the host definition, sums in longdouble"""
    mesh, w, pts, _, _ = plane_case(name)
    ref = B.boundary(mesh, w.map, order, 0, orientation)
    sums, abss, mags, terms = B.measures(ref["faces"], ref["face_patch"], len(ref["patches"]), pts, order, False)
    b = w.boundary(order, orientation=orientation)
    v = B.values_of(b.measure(pts)).astype(LD)
    bar = B.bar_against_reference(terms, abss, mags, False)
    area, area_mag = B.signed_cell_areas(mesh, w.map, pts, orientation_of(name))
    area_bar = 0.5 * bar[:, 4].sum() + float(area_mag) * (4 * len(w.cells(1)) + 4) * 2.0 ** -64   # the second term: the reference's own sum
    return v[:, 1:3].sum(axis=0), v[:, 4].sum() / 2 - area, bar[:, 1:3].sum(axis=0), area_bar


@pytest.mark.parametrize("name", ["cut", "strip_reversed", "T106", "LS89"])
def test_orientation_closes_the_boundary_and_encloses_the_cells(name):
    assert len(set(orientation_of(name))) == 2   # the blocks differ in handedness
    n_sum, area_gap, n_bar, area_bar = closure(name, orientation_of(name))
    print(f"{name}: sum n = ({float(n_sum[0]):.3e}, {float(n_sum[1]):.3e}) within ({n_bar[0]:.3e}, {n_bar[1]:.3e}); area gap {float(area_gap):.3e} within {area_bar:.3e}")
    assert (np.abs(n_sum).astype(np.float64) <= n_bar).all()
    assert abs(float(area_gap)) <= area_bar


def test_without_the_orientation_the_cut_does_not_close():
    n_sum, area_gap, n_bar, area_bar = closure("cut", (1,) * 9)
    assert (np.abs(n_sum).astype(np.float64) > n_bar).any() or abs(float(area_gap)) > area_bar
    assert abs(float(area_gap)) > 1e3 * area_bar   # by far: the flipped blocks run their sides the wrong way round


def test_planar_stack_of_identical_cuts_volume_and_caps():
    mesh, w, pts2, _, _ = plane_case("cut")
    nk, dz = 5, 0.125
    blocks = planar_blocks(mesh, nk, dz)
    o3 = tuple(stack.quality_of_planes(*blk).orientation for blk in blocks)
    assert o3 == orientation_of("cut")   # the span ascends: the hexahedra have the handedness of the cut
    pts = weld.Weld(mesh, host=True).points(blocks)
    ref = B.boundary(mesh, w.map, 1, nk, o3)
    sums, abss, mags, terms = B.measures(ref["faces"], ref["face_patch"], len(ref["patches"]), pts, 1, True)
    b = w.boundary(1, layers=nk, orientation=o3)
    same_boundary(b, ref)
    v = B.values_of(b.measure(pts)).astype(LD)
    bar = B.bar_against_reference(terms, abss, mags, True)
    within(v, sums, bar)
    area, area_mag = B.signed_cell_areas(mesh, w.map, pts2, orientation_of("cut"))
    ref_bar = float(area_mag) * (4 * len(w.cells(1)) + 4) * 2.0 ** -64
    span = LD(dz) * (nk - 1)
    assert abs(float(v[:, 4].sum() / 3 - area * span)) <= bar[:, 4].sum() / 3 + ref_bar * float(span)
    hub, shroud = v[-2], v[-1]
    assert abs(float(hub[3] + area)) <= bar[-2, 3] + ref_bar and abs(float(shroud[3] - area)) <= bar[-1, 3] + ref_bar   # -+ area z
    assert (np.abs(v[-2:, 1:3]).astype(np.float64) <= bar[-2:, 1:3]).all()
    assert (np.abs(v[:, 1:4].sum(axis=0)).astype(np.float64) <= bar[:, 1:4].sum(axis=0)).all()   # closed


@pytest.mark.parametrize("name,order", [("T106", 1), ("T106", 2), ("LS89", 1), ("periodic_channel", 1), ("periodic_channel", 2)])
def test_periodic_faces_match_under_their_translation(name, order):
    mesh, w, pts, _, _ = plane_case(name)
    b = w.boundary(order, orientation=orientation_of(name))
    pairs = set()
    for ids, _ in w.periodic_pairs():
        pairs |= {tuple(r) for r in ids.tolist()}
    gap = weld.Weld(mesh, host=True)
    gap.points(mesh)
    total = 0
    at = lambda a: 0 if a == 0 else 1 if a == order else a + 1
    for fa, fb, t in b.periodic_faces():
        assert len(fa) == len(fb) and len(fa) > 0
        total += len(fa)
        for a in range(order + 1):
            ia, ib = fa[:, at(a)], fb[:, at(order - a)]
            assert np.abs(pts[ia] + np.array(t) - pts[ib]).max() <= gap.info.periodic_gap
            assert {tuple(r) for r in np.stack([ia, ib], axis=1).tolist()} <= pairs
    assert total * order == {"T106": 150, "LS89": 145, "periodic_channel": 12}[name]


def test_periodic_lateral_faces_of_a_stacked_channel():
    mesh, w, _, _, _ = plane_case("periodic_channel")
    p, nk = 2, 5
    b = w.boundary(p, layers=nk, orientation=orientation_of("periodic_channel"))
    local = B.quad_order(p)
    where = {ab: k for k, ab in enumerate(local)}
    (fa, fb, t), = b.periodic_faces()
    assert fa.shape == (6 * 2, 9)
    pairs = {tuple(r) for r in w.periodic_pairs()[0][0].tolist()}
    for (a, c), k in where.items():   # node (a, c) of a face is the image of node (p - a, c) of its partner, in the same layer
        ia, ib = fa[:, k], fb[:, where[(p - a, c)]]
        assert np.array_equal(ia // w.nodes, ib // w.nodes)
        assert {tuple(r) for r in np.stack([ia % w.nodes, ib % w.nodes], axis=1).tolist()} <= pairs


def test_errors(capsys):
    L = _capi.lib()
    mesh = configs.periodic_channel(13, 9, tfi=oracle_tfi)
    mesh.boundary_conditions[0] = Condition(Range(0, Side.j_min, 0, 7), ConditionTag.inlet)   # ends inside the last segment of order 2
    w = weld.Weld(mesh, host=True)
    assert w.boundary(1).patches[0].faces == 7
    with pytest.raises(_capi.TmError) as e:
        w.boundary(2)
    assert e.value.code == _capi.TM_E_MISMATCH and "condition 0" in str(e.value)
    good = weld.Weld(configs.periodic_channel(13, 9, tfi=oracle_tfi), host=True)
    for order in (0, 9):
        with pytest.raises(_capi.TmError):
            good.boundary(order)
    md = _capi.MeshDesc(configs.two_by_two(8, 9, tfi=oracle_tfi), with_coordinates=False)
    for fn in (L.tm_weld_boundary_faces_host, L.tm_weld_boundary_faces):   # ids are int32: sizes only, nothing is read
        assert fn(md.ref(), None, 2 ** 29, 1, 4, None, None, None, None) == _capi.TM_E_ARG
    # the measure refuses what it cannot read safely
    pts = np.zeros((4, 2))
    faces = np.array([[0, 1], [1, 4]], dtype=np.int32)
    patch = np.zeros(2, dtype=np.int32)
    recs = (_capi.tm_weld_patch * 1)()
    dp = C.POINTER(C.c_double)
    planes = (dp * 2)(_capi.f64ptr(np.ascontiguousarray(pts[:, 0])), _capi.f64ptr(np.ascontiguousarray(pts[:, 1])))
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    for fn in (L.tm_weld_faces_measure_host, L.tm_weld_faces_measure):
        assert fn(2, 1, 2, i32(faces), i32(patch), 1, 4, 2, planes, recs) == _capi.TM_E_ARG            # point 4 of 4
        assert fn(2, 1, 1, i32(faces), i32(np.array([1], dtype=np.int32)), 1, 4, 2, planes, recs) == _capi.TM_E_ARG   # patch past the patches
        assert fn(4, 1, 1, i32(faces), i32(patch), 1, 4, 2, planes, recs) == _capi.TM_E_ARG
    from turbomesh_amd.__main__ import main

    cfg = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "examples", "T106", "T106.json")
    with pytest.raises(SystemExit) as ex:   # refused while the arguments are read: nothing is meshed
        main([cfg, "--hip", "--boundary", "--output", "t.vtk"])
    assert ex.value.code not in (0, None) and "--boundary" in capsys.readouterr().err


@pytest.mark.parametrize("kind", [3, 68, 9, 70])
def test_file_round_trip_bit_for_bit(kind, tmp_path):
    mesh, w0, _, _, _ = plane_case("periodic_channel")
    w = weld.Weld(mesh, host=True)
    order = 1 if kind in (3, 9) else 2
    o = orientation_of("periodic_channel")
    src = mesh if kind in (3, 68) else [tuple(np.stack([p * (1.0 + k / 3.0) if c < 2 else p + k / 7.0 for k in range(3)]) for c, p in enumerate((X, Y, np.zeros_like(X))))
                                        for X, Y in cpu.R.mesh_planes(mesh)]
    um = w.mesh(src, order, boundary=True, orientation=o)
    b = um.boundary
    assert b.cell_type == kind and any(r.measure > 0 for r in b.patches)
    f = str(tmp_path / "w.vtk")
    um.write(f)
    vtk, js = um.write_boundary(f)
    assert (vtk, js) == (str(tmp_path / "w.boundary.vtk"), str(tmp_path / "w.boundary.json"))
    pts, faces, types, patch, kinds = output.read_vtk_boundary(vtk)
    vol = output.read_vtk_lagrange(f)[0]
    assert np.array_equal(pts, vol)   # the same points as the volume file: ids are shared
    assert np.array_equal(pts[:, :um.points.shape[1]], um.points)
    assert np.array_equal(faces, b.faces) and np.all(types == kind) and np.array_equal(patch, b.face_patch)
    assert np.array_equal(kinds, np.array([b.patches[q].kind for q in b.face_patch]))
    table = json.load(open(js))
    assert table == json.loads(json.dumps(b.table())) and len(table["patches"]) == len(b.patches)
    for rec, r in zip(table["patches"], b.patches):
        assert (rec["name"], rec["kind"], rec["begin"], rec["faces"], rec["measure"], rec["moment"]) == (r.name, r.kind, r.begin, r.faces, r.measure, r.moment)
    um.distribution = "gauss_lobatto"
    if order > 1:
        with pytest.raises(ValueError):
            um.write_boundary(f)
    with pytest.raises(ValueError):
        w.mesh(mesh, 1).write_boundary(f)   # no boundary was asked for


def test_struct_sizes():
    assert C.sizeof(_capi.tm_weld_patch) == 88 and C.sizeof(_capi.tm_weld_boundary_info) == 56
