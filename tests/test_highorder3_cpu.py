"""CPU: high-order hexahedra of stacked blocks (include/tm_hip.h, "high-order hexahedra of stacked blocks") -- tm_ho3_planes_host,
tm_stack_elevate_host, tm_ho3_check and the Python layer against tests/ho3_reference.py (numpy longdouble, written from the definition)
and against pins that rest on no reading of the library.  No GPU: the device side is tests/test_gpu_highorder3.py."""
import ctypes as C

import numpy as np
import pytest

from tests import control_field_reference as cfr
from tests import ho3_reference as h3
from tests import ho_reference as hr
from tests import stack_reference as sr
from tests import stack_surface_reference as ssr
from tests.conftest import oracle_tfi
from turbomesh_amd import _capi, configs, highorder, output, quality, stack

LD = np.longdouble
DISTRIBUTIONS = ("equidistant", "gauss_lobatto", "prescribed")
ORDERS = (1, 2, 3, 4)
RECORD = ("elements", "invalid", "orientation", "order", "min_scaled_jacobian", "worst_block", "worst_e", "worst_f", "worst_g", "min_jacobian",
          "max_jacobian", "hist")


def elevation(p, dist):
    return highorder.Elevation(p, dist, hr.prescribed_nodes(p) if dist == "prescribed" else None)


def same_record(a, b):
    """Every field equal bit for bit (NaN equals NaN)."""
    return all(np.asarray(getattr(a, k)).tobytes() == np.asarray(getattr(b, k)).tobytes() for k in RECORD)


def cut_meshes(blocks):
    return [cfr.single_block_mesh(b) for b in blocks]


def bent_cuts(ni, nj, K):
    return [cfr.bent_clustered(ni, nj, seed=c) + 0.01 * c for c in range(K)]


# ------------------------------------------------------------------ the host definition against the reference
def blocks_for(p):
    """A multi-element bent block, and one block whose coordinates are of the size of its element (a single element around the origin):
    there the Jacobian bar is not loose by |coordinate| / element size."""
    s = np.linspace(-0.5, 0.5, p + 1)
    k, j, i = np.meshgrid(s, s, s, indexing="ij")
    small = (i + 0.08 * np.sin(2.0 * j) + 0.03 * k * k, j + 0.06 * i * i - 0.01, k + 0.05 * i * j)
    return [("bent", h3.bent_block(2 * p + 1, 3 * p + 1, 2 * p + 1, seed=p)), ("origin", small)]


@pytest.mark.parametrize("p", ORDERS)
def test_host_planes_against_the_reference(p):
    for dist in DISTRIBUTIONS:
        for name, (X, Y, Z) in blocks_for(p):
            ref = h3.Reference(X, Y, Z, p, dist, hr.prescribed_nodes(p) if dist == "prescribed" else None)
            x, y, z, q, sj = highorder.planes3d(X, Y, Z, elevation(p, dist))
            ratio = hr.worst_ratio(np.stack([x, y, z], axis=-1), ref.Y, ref.bar_Y)
            print(f"ho3_parity: host p {p} {dist} {name}: worst |Y - Y_ref| / bar {ratio:.3f}")
            assert ratio <= 1.0
            assert q.elements == ref.Ei * ref.Ej * ref.Eg == (2 * 3 * 2 if name == "bent" else 1) and q.order == p and q.orientation == ref.orientation == 1
            assert ref.decided().all() and q.invalid == ref.invalid == 0
            lo, hi = ref.sj_interval()
            assert sj.shape == (ref.Eg, ref.Ej, ref.Ei) and np.all((sj.T >= lo) & (sj.T <= hi)), (dist, name)
            d = ref.delta.max()
            jr = (abs(LD(q.min_jacobian) - ref.jmin.min()) / d, abs(LD(q.max_jacobian) - ref.jmax.max()) / d)
            print(f"ho3_parity: host p {p} {dist} {name}: worst |J - J_ref| / bar {float(max(jr)):.3f}")
            assert max(jr) <= 1.0
            g, f, e = np.unravel_index(np.nanargmin(sj), sj.shape)            # the first minimum in (g, f, e) order: the tie rule
            assert q.min_scaled_jacobian == np.nanmin(sj) and (q.worst_e, q.worst_f, q.worst_g) == (e, f, g)
            assert sum(q.hist) == q.elements - q.invalid
            assert np.array_equal(np.histogram(np.minimum(sj.ravel(), 0.95), bins=np.arange(11) / 10)[0], q.hist)
            rep = highorder.planes3d(X, Y, Z, elevation(p, dist), planes=False)   # a report alone
            assert rep[0] is None and same_record(rep[3], q) and rep[4].tobytes() == sj.tobytes()


@pytest.mark.parametrize("p", ORDERS)
def test_equidistant_and_order_one_copy_the_nodes(p):
    X, Y, Z = h3.bent_block(2 * p + 1, p + 1, 3 * p + 1, seed=7)
    Y[0, 0, 0] = -0.0                                                         # copied: the sign of a zero survives
    x, y, z, _, _ = highorder.planes3d(X, Y, Z, elevation(p, "equidistant"))
    assert x.tobytes() == X.tobytes() and y.tobytes() == Y.tobytes() and z.tobytes() == Z.tobytes()
    if p == 1:
        for dist in DISTRIBUTIONS:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(highorder.planes3d(X, Y, Z, elevation(1, dist))[:3], (X, Y, Z)))


@pytest.mark.parametrize("p", ORDERS)
def test_element_layers_equal_the_2d_elevation_of_that_layer(p):
    """Rows 0 and p of T are unit vectors: layer k = g*p of the output is K13's elevation of fine layer k, numerically equal."""
    X, Y, Z = h3.bent_block(3 * p + 1, 2 * p + 1, 2 * p + 1, seed=11)
    for dist in ("gauss_lobatto", "prescribed"):
        el = elevation(p, dist)
        x, y, z, _, _ = highorder.planes3d(X, Y, Z, el)
        for k in range(0, 2 * p + 1, p):
            for (a, b), (fa, fb) in (((x, y), (X, Y)), ((z, x), (Z, X))):     # any two components
                layer = np.ascontiguousarray(np.stack([fa[k].T, fb[k].T], axis=-1))
                xa, xb, _, _ = el.block(cfr.single_block_mesh(layer), 0, host=True)
                assert np.array_equal(a[k], xa) and np.array_equal(b[k], xb), (dist, k)
        # and faces, edges, corners are shared: the fine nodes at the element corners come back unchanged
        assert np.array_equal(x[::p, ::p, ::p], X[::p, ::p, ::p]) and np.array_equal(z[::p, ::p, ::p], Z[::p, ::p, ::p])


# ------------------------------------------------------------------ from the cuts: tm_stack_elevate_host
HOST_CASES = [(1, 3, 2, 2, "linear", "planar"), (2, 5, 7, 3, "cubic", "planar"), (3, 7, 4, 2, "cubic", "cylindrical"), (4, 9, 5, 5, "linear", "cylindrical"),
              (2, 5, 5, 3, "cubic", "revolution")]


def stack_for(K, nk, interpolation, mapping, seed):
    z = sr.spans(K, "uniform" if mapping != "planar" else "nonuniform")
    s = np.sort(sr.layers_with_cuts(z, nk, seed=seed))
    if mapping == "revolution":
        u, x, r, rr = ssr.tables(K, seed=seed)
        return stack.Stack(z, s, interpolation, mapping, surfaces=stack.Surfaces(u, x, r, rr))
    return stack.Stack(z, s, interpolation, mapping)


@pytest.mark.parametrize("case", HOST_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_host_from_cuts_equals_host_on_the_stacked_planes(case):
    p, ni, nj, K, interpolation, mapping = case
    Eg = 3
    st = stack_for(K, Eg * p + 1, interpolation, mapping, seed=ni)
    cuts = cut_meshes(bent_cuts(ni, nj, K))
    fine = st.block(cuts, 0, host=True)
    for dist in ("gauss_lobatto", "equidistant"):
        el = elevation(p, dist)
        want = highorder.planes3d(*fine, el)
        got = st.elevate(cuts, el, 0, host=True)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], want[:3])) and same_record(got[3], want[3]) and got[4].tobytes() == want[4].tobytes()
        # windows tile the block; the record and sj cover the whole block whatever the window
        parts = [st.elevate(cuts, el, 0, g, 1, host=True) for g in range(Eg)]
        for q in range(3):
            for g, part in enumerate(parts):
                assert part[q].tobytes() == want[q][g * p:(g + 1) * p + 1].tobytes()
        assert all(same_record(part[3], want[3]) and part[4].tobytes() == want[4].tobytes() for part in parts)
        rep = st.elevate(cuts, el, 0, host=True, planes=False)
        assert rep[0] is None and same_record(rep[3], want[3])
    if mapping == "revolution":
        outside = st.elevate(cuts, elevation(p, "equidistant"), 0, host=True, planes=False, return_outside=True)[5]
        assert np.array_equal(outside, st.block(cuts, 0, host=True, return_outside=True)[3])


def affine_cuts(ni, nj, K, shift):
    """K cuts that are one affine map of the lattice, shifted by c * shift from cut to cut; everything dyadic, so every node is exact."""
    M = np.array([[0.75, -0.25], [0.5, 1.25]])
    I, J = np.meshgrid(np.arange(ni) / 8.0, np.arange(nj) / 16.0, indexing="ij")
    base = np.stack([M[0, 0] * I + M[0, 1] * J + 0.5, M[1, 0] * I + M[1, 1] * J - 0.25], axis=-1)
    return [base + c * np.asarray(shift) for c in range(K)], (M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]) / 8.0 / 16.0


@pytest.mark.parametrize("p", ORDERS)
def test_affine_cuts_have_a_constant_jacobian(p):
    ni, nj, nk = 2 * p + 1, 3 * p + 1, 2 * p + 1
    blocks, det2 = affine_cuts(ni, nj, 3, (0.125, -0.0625))
    z = np.array([0.0, 1.0, 2.0])
    st = stack.Stack(z, np.arange(nk) / (nk - 1) * 2.0, "linear", "planar")     # uniform layers, dz/dw = 2/(nk-1) per index step
    cuts = cut_meshes(blocks)
    want = det2 * 2.0 / (nk - 1)
    for dist in DISTRIBUTIONS:
        X, Y, Z, q, sj = st.elevate(cuts, elevation(p, dist), 0, host=True)
        ref = h3.Reference(*st.block(cuts, 0, host=True), p, dist, hr.prescribed_nodes(p) if dist == "prescribed" else None)
        d = float(ref.delta.max())
        assert q.invalid == 0 and q.orientation == 1 and q.elements == 2 * 3 * 2
        assert abs(q.min_jacobian - want) <= d and abs(q.max_jacobian - want) <= d
        assert np.all(np.abs(sj - 1.0) <= 2 * d / want + 4 * np.finfo(float).eps)


def folded_stack():
    return stack.Stack([0.0, 1.0], [0.0, 0.6, 0.3, 0.8, 1.0], "linear", "planar")


def test_a_fold_in_span_is_found():
    """p = 2, layers 0, 0.6, 0.3 | 0.3, 0.8, 1.0: dz/dw is +1.05 / -0.75 at the ends of span element 0 and +0.65 / +0.05 in element 1."""
    ni, nj = 5, 7
    cuts = cut_meshes(bent_cuts(ni, nj, 2))
    for dist in ("equidistant", "gauss_lobatto"):
        _, _, Z, q, sj = folded_stack().elevate(cuts, elevation(2, dist), 0, host=True)
        Ei, Ej = 2, 3
        assert q.elements == 2 * Ei * Ej and q.invalid == Ei * Ej and q.orientation == 1
        assert np.isnan(sj[0]).all() and np.isfinite(sj[1]).all() and q.worst_g == 1
    D = hr.tables(2, "equidistant")[1]
    dz = [float(D[a] @ np.array(zs, dtype=LD)) for zs in ([0.0, 0.6, 0.3], [0.3, 0.8, 1.0]) for a in (0, 2)]
    assert np.allclose(dz, [1.05, -0.75, 0.65, 0.05], rtol=0, atol=1e-15)


def test_mirrored_cuts_have_the_other_handedness_and_the_same_bits():
    ni, nj, p = 7, 5, 2
    blocks = bent_cuts(ni, nj, 3)
    mirrored = [b * np.array([-1.0, 1.0]) for b in blocks]
    st = stack.Stack([0.0, 0.5, 1.0], np.linspace(0.0, 1.0, 5), "cubic", "planar")
    a = st.elevate(cut_meshes(blocks), elevation(p, "gauss_lobatto"), 0, host=True)
    b = st.elevate(cut_meshes(mirrored), elevation(p, "gauss_lobatto"), 0, host=True)
    assert a[3].orientation == 1 and b[3].orientation == -1 and a[3].invalid == b[3].invalid == 0
    assert a[4].tobytes() == b[4].tobytes()
    assert (a[3].min_scaled_jacobian, a[3].min_jacobian, a[3].max_jacobian, a[3].hist) == (b[3].min_scaled_jacobian, b[3].min_jacobian, b[3].max_jacobian, b[3].hist)
    assert np.array_equal(b[0], -a[0]) and b[1].tobytes() == a[1].tobytes()


def test_non_finite_coordinates_make_invalid_elements_and_nothing_else():
    X, Y, Z = h3.bent_block(5, 5, 5)
    X[1, 1, 1] = np.nan
    _, _, _, q, sj = highorder.planes3d(X, Y, Z, elevation(2, "gauss_lobatto"))
    assert q.invalid == 1 and np.isnan(sj[0, 0, 0]) and np.isfinite(sj[1, 1, 1]) and np.isfinite(q.min_scaled_jacobian)
    X[:] = np.nan
    _, _, _, q, sj = highorder.planes3d(X, Y, Z, elevation(2, "gauss_lobatto"))
    assert q.invalid == q.elements == 8 and np.isnan(q.min_scaled_jacobian) and (q.worst_block, q.worst_e, q.worst_f, q.worst_g) == (0, 0, 0, 0)
    assert np.isnan(q.min_jacobian) and np.isnan(q.max_jacobian) and sum(q.hist) == 0 and np.isnan(sj).all()


def test_total_of_block_records():
    a = highorder.planes3d(*h3.bent_block(5, 5, 5), elevation(2, "gauss_lobatto"))[3]
    X, Y, Z = h3.bent_block(5, 7, 5, seed=2)
    X[1, 1, 1] = np.nan
    b = highorder.planes3d(X, Y, Z, elevation(2, "gauss_lobatto"), block=1)[3]
    t = quality.total_ho3([a, b])
    assert t.elements == a.elements + b.elements and t.invalid == b.invalid == 1 and t.order == 2 and t.orientation == 1
    assert t.min_scaled_jacobian == min(a.min_scaled_jacobian, b.min_scaled_jacobian)
    worst = a if a.min_scaled_jacobian <= b.min_scaled_jacobian else b
    assert (t.worst_block, t.worst_e, t.worst_f, t.worst_g) == (worst.worst_block, worst.worst_e, worst.worst_f, worst.worst_g)
    assert t.min_jacobian == min(a.min_jacobian, b.min_jacobian) and t.max_jacobian == max(a.max_jacobian, b.max_jacobian)
    assert t.hist == tuple(x + y for x, y in zip(a.hist, b.hist))
    empty = quality.total_ho3([])
    assert empty.elements == 0 and np.isnan(empty.min_scaled_jacobian)


# ------------------------------------------------------------------ checks, arguments
def test_check_names_each_of_the_three_offenders():
    st = stack.Stack([0.0, 1.0], np.linspace(0.0, 1.0, 9))
    m = configs.strip(3, 9, 13, tfi=oracle_tfi)
    for p in (1, 2, 4):
        st.check_elevation(m, elevation(p, "gauss_lobatto"))
    with pytest.raises(_capi.TmError) as e:
        st.check_elevation(m, elevation(3, "gauss_lobatto"))                  # 8 cells along i
    assert e.value.code == _capi.TM_E_SIZE and "block 0" in str(e.value) and "order 3" in str(e.value)
    m.connections[1].ranges[0].start = 2                                      # off the element grid of order 4
    with pytest.raises(_capi.TmError) as e:
        st.check_elevation(m, elevation(4, "gauss_lobatto"))
    assert e.value.code == _capi.TM_E_SIZE and "connection 1" in str(e.value) and "block 1" in str(e.value)
    st.check_elevation(m, elevation(2, "gauss_lobatto"))
    m = configs.strip(3, 9, 13, tfi=oracle_tfi)
    for nk in (8, 10, 4):                                                     # 7 and 9 layer cells; fewer than p+1 layers
        with pytest.raises(_capi.TmError) as e:
            stack.Stack([0.0, 1.0], np.linspace(0.0, 1.0, nk)).check_elevation(m, elevation(4, "gauss_lobatto"))
        assert e.value.code == _capi.TM_E_SIZE and f"{nk} layers" in str(e.value) and "block" not in str(e.value)
    with pytest.raises(_capi.TmError) as e:
        st.check_elevation(m, elevation(5, "gauss_lobatto"))                  # the order itself
    assert e.value.code == _capi.TM_E_ARG and "TM_HO3_MAX_ORDER" in str(e.value)


def test_struct_size_and_arguments_of_the_host_calls():
    assert C.sizeof(_capi.tm_ho3_quality) == 160 and _capi.TM_HO3_MAX_ORDER == 4
    L = _capi.lib()
    X, Y, Z = h3.bent_block(5, 5, 5)
    out = [np.empty_like(X) for _ in range(3)]
    q = _capi.tm_ho3_quality()

    def rc(p, planes=(True, True, True), nk=5, src=True):
        opt = _capi.tm_ho_opt(p, _capi.TM_HO_GAUSS_LOBATTO, None)
        ptr = [_capi.f64ptr(o) if w else None for o, w in zip(out, planes)]
        return L.tm_ho3_planes_host(_capi.f64ptr(X) if src else None, _capi.f64ptr(Y), _capi.f64ptr(Z), 5, 5, nk, C.byref(opt), 0, *ptr, C.byref(q), None)

    assert rc(2) == _capi.TM_OK and q.elements == 8 and rc(4) == _capi.TM_OK and q.elements == 1 and rc(1) == _capi.TM_OK and q.elements == 64
    assert rc(2, (False, False, False)) == _capi.TM_OK
    assert rc(2, (True, False, True)) == _capi.TM_E_ARG and rc(2, src=False) == _capi.TM_E_ARG
    assert rc(3) == _capi.TM_E_SIZE and rc(2, nk=4) == _capi.TM_E_SIZE and rc(4, nk=3) == _capi.TM_E_SIZE and rc(2, nk=1) == _capi.TM_E_SIZE
    for p in (5, 6, 7, 8):
        assert rc(p) == _capi.TM_E_ARG                                        # 2-D orders that hexahedra do not take
    assert rc(0) == _capi.TM_E_ARG and rc(9) == _capi.TM_E_ARG
    # from the cuts: the window, and tables with the wrong mapping
    cuts = cut_meshes(bent_cuts(5, 5, 2))
    st = stack.Stack([0.0, 1.0], np.linspace(0.0, 1.0, 5), "linear")
    el = elevation(2, "gauss_lobatto")
    assert st.elevate(cuts, el, 0, 1, 1, host=True)[0].shape == (3, 5, 5)
    for g_begin, g_count in ((0, 3), (2, 1), (3, 0), (0, 0)):
        with pytest.raises(_capi.TmError) as e:
            st.elevate(cuts, el, 0, g_begin, g_count, host=True)
        assert e.value.code == _capi.TM_E_ARG
    with pytest.raises(_capi.TmError) as e:
        stack.Stack([0.0, 1.0], np.linspace(0.0, 1.0, 4), "linear").elevate(cuts, el, 0, host=True)
    assert e.value.code == _capi.TM_E_SIZE
    u, x, r, rr = ssr.tables(2, seed=1)
    st._opt.mapping = _capi.TM_STACK_REVOLUTION                               # revolution without tables
    with pytest.raises(_capi.TmError) as e:
        st.elevate(cuts, el, 0, host=True)
    assert e.value.code == _capi.TM_E_ARG


# ------------------------------------------------------------------ writer
def point_index_from_ijk(i, j, k, p):
    """vtkLagrangeHexahedron::PointIndexFromIJK of VTK 9 for one order p in all three directions, restated."""
    ibdy, jbdy, kbdy = i in (0, p), j in (0, p), k in (0, p)
    nbdy = ibdy + jbdy + kbdy
    if nbdy == 3:
        return (i and (2 if j else 1) or (3 if j else 0)) + (4 if k else 0)
    offset = 8
    if nbdy == 2:
        if not ibdy:
            return (i - 1) + ((p - 1) + (p - 1) if j else 0) + (2 * (p - 1 + p - 1) if k else 0) + offset
        if not jbdy:
            return (j - 1) + ((p - 1) if i else 2 * (p - 1) + (p - 1)) + (2 * (p - 1 + p - 1) if k else 0) + offset
        offset += 4 * (p - 1) + 4 * (p - 1)
        return (k - 1) + (p - 1) * (i and (2 if j else 1) or (3 if j else 0)) + offset     # VTK >= 9: the fourth edge is (0, p), not (p, p)
    offset += 4 * (p - 1 + p - 1 + p - 1)
    if nbdy == 1:
        if ibdy:
            return (j - 1) + (p - 1) * (k - 1) + ((p - 1) * (p - 1) if i else 0) + offset
        offset += 2 * (p - 1) * (p - 1)
        if jbdy:
            return (i - 1) + (p - 1) * (k - 1) + ((p - 1) * (p - 1) if j else 0) + offset
        offset += 2 * (p - 1) * (p - 1)
        return (i - 1) + (p - 1) * (j - 1) + ((p - 1) * (p - 1) if k else 0) + offset
    offset += 2 * 3 * (p - 1) * (p - 1)
    return offset + (i - 1) + (p - 1) * ((j - 1) + (p - 1) * (k - 1))


@pytest.mark.parametrize("p", ORDERS)
def test_vtk_round_trip_and_connectivity(p, tmp_path):
    local = highorder.lagrange_hex_order(p)
    assert len(local) == (p + 1) ** 3 and [point_index_from_ijk(a, b, c, p) for a, b, c in local] == list(range((p + 1) ** 3))
    if p > 2:
        return                                                                # the order is what differs between the orders; one file format
    K = 2
    st = stack.Stack([0.0, 1.0], np.linspace(0.0, 1.0, 2 * p + 1), "linear")
    A, B = bent_cuts(2 * p + 1, 3 * p + 1, K), bent_cuts(p + 1, 2 * p + 1, K)
    A[0][0, 0, 1] = -0.0
    cuts = []
    for c in range(K):
        m = cfr.single_block_mesh(A[c])
        m.addBlock("block_1", configs.block_from_array(B[c].copy()))
        cuts.append(m)
    hom = st.mesh3d_ho(cuts, elevation(p, "equidistant"), host=True)
    f = str(tmp_path / "curved.vtk")
    hom.write(f)
    points, cells, types = output.read_vtk_lagrange(f)
    want = np.concatenate([np.stack([a.reshape(-1) for a in xyz], axis=1) for xyz in hom.blocks])
    assert points.shape == want.shape and np.array_equal(points, want) and np.array_equal(np.signbit(points), np.signbit(want))
    assert np.all(types == 72) and cells.shape == (2 * 3 * 2 + 1 * 2 * 2, (p + 1) ** 3)
    n, offset = 0, 0
    for X, Y, Z in hom.blocks:
        nk, nj, ni = X.shape
        for g in range((nk - 1) // p):
            for f_ in range((nj - 1) // p):
                for e in range((ni - 1) // p):                                # elements with e fastest, like sj
                    for a in range(p + 1):
                        for b in range(p + 1):
                            for c in range(p + 1):
                                i, j, k = e * p + a, f_ * p + b, g * p + c
                                node = cells[n, point_index_from_ijk(a, b, c, p)]
                                assert node == offset + (k * nj + j) * ni + i
                                assert tuple(points[node]) == (X[k, j, i], Y[k, j, i], Z[k, j, i])
                    n += 1
        offset += ni * nj * nk
    with pytest.raises(ValueError):
        st.mesh3d_ho(cuts, elevation(p, "gauss_lobatto"), host=True).write(f)  # Lagrange cells assume equidistant nodes
    g = str(tmp_path / "curved.xyz")
    hom2 = st.mesh3d_ho(cuts, elevation(p, "gauss_lobatto"), host=True)
    hom2.write(g)
    back = output.read_plot3d_3d(g)
    assert [b[:3] for b in back] == hom2.sizes()
    assert all(b[3 + q].tobytes() == hom2.blocks[k][q].tobytes() for k, b in enumerate(back) for q in range(3))
    assert hom2.total.elements == 16 and same_record(hom2.total, quality.total_ho3(hom2.per_block))


def test_python_layer_refuses_what_it_cannot_serve():
    class FakeHandle:
        _h = 1
        _mesh = cfr.single_block_mesh(cfr.bent_clustered(5, 5))

    st = stack.Stack([0.0, 1.0], np.linspace(0.0, 1.0, 5))
    with pytest.raises(ValueError):
        st.elevate([FakeHandle(), FakeHandle()], elevation(2, "gauss_lobatto"), 0, host=True)
    with pytest.raises(ValueError):
        st.elevate(cut_meshes(bent_cuts(5, 5, 2)), elevation(2, "gauss_lobatto"), 0, host=True, return_outside=True)
    with pytest.raises(ValueError):
        highorder.planes3d(np.zeros((3, 3)), np.zeros((3, 3)), np.zeros((3, 3)), elevation(2, "gauss_lobatto"))
