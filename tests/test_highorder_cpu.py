"""CPU: high-order elevation (include/tm_hip.h, "high-order elements") -- tm_ho_tables, tm_ho_check, tm_ho_elevate_host and the
Python layer against tests/ho_reference.py (numpy longdouble, written from the definitions) and against analytic pins that rest on no
reading of the reference.  No GPU: the device side is tests/test_gpu_highorder.py."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import control_field_reference as cfr
from tests import ho_reference as hr
from tests.conftest import oracle_tfi
from turbomesh_amd import _capi, configs, highorder, output, quality

LD = np.longdouble
DISTRIBUTIONS = ("equidistant", "gauss_lobatto", "prescribed")
ORDERS = range(1, 9)


def elevation(p, dist):
    return highorder.Elevation(p, dist, hr.prescribed_nodes(p) if dist == "prescribed" else None)


def host_block(X, p, dist):
    """(Y (ni, nj, 2), HoQuality, sj (Ei, Ej)) of tm_ho_elevate_host on one block."""
    Xp, Yp, q, sj = elevation(p, dist).block(cfr.single_block_mesh(X), 0, host=True)
    return np.stack([Xp.T, Yp.T], axis=-1), q, sj.T


# ------------------------------------------------------------------ tables
@pytest.mark.parametrize("p", ORDERS)
def test_tables_equal_the_reference_after_one_rounding(p):
    for dist in DISTRIBUTIONS:
        pres = hr.prescribed_nodes(p) if dist == "prescribed" else None
        t, T, D = elevation(p, dist).tables()
        Tr, Dr = hr.tables(p, dist, pres)
        assert np.array_equal(t, hr.nodes(p, dist, pres)), dist
        assert np.array_equal(T, Tr.astype(np.float64)) and np.array_equal(D, Dr.astype(np.float64)), dist
        unit = np.eye(p + 1)
        assert np.array_equal(T[0], unit[0]) and np.array_equal(T[p], unit[p])
        assert t[0] == 0.0 and t[p] == 1.0 and np.all(np.diff(t) > 0)
        assert np.all(np.abs(D.sum(axis=1)) <= 64 * np.finfo(float).eps * np.abs(D).sum(axis=1))   # the derivative of a constant


@pytest.mark.parametrize("p", ORDERS)
def test_equidistant_is_the_identity(p):
    t, T, _ = elevation(p, "equidistant").tables()
    assert np.array_equal(T, np.eye(p + 1))
    assert np.array_equal(t, (np.arange(p + 1, dtype=LD) / p).astype(np.float64))


def test_gauss_lobatto_nodes():
    for p in ORDERS:
        t = elevation(p, "gauss_lobatto").tables()[0]
        assert np.all(np.abs((t + t[::-1]) - 1.0) <= np.spacing(1.0)), p      # symmetric to 1 ulp
    assert np.array_equal(elevation(1, "gauss_lobatto").tables()[0], [0.0, 1.0])
    assert np.array_equal(elevation(2, "gauss_lobatto").tables()[0], [0.0, 0.5, 1.0])
    t3 = elevation(3, "gauss_lobatto").tables()[0]
    known = [(1 - 1 / math.sqrt(5)) / 2, (1 + 1 / math.sqrt(5)) / 2]
    assert np.all(np.abs(t3[1:3] - known) <= np.spacing(1.0))
    # p = 4: x = 0, +-sqrt(3/7)
    t4 = elevation(4, "gauss_lobatto").tables()[0]
    assert t4[2] == 0.5 and abs(t4[3] - (1 + math.sqrt(3 / 7)) / 2) <= np.spacing(1.0)


def test_options_that_are_refused():
    L = _capi.lib()

    def rc(order, dist, nodes=None):
        n = None if nodes is None else np.asarray(nodes, dtype=np.float64)
        opt = _capi.tm_ho_opt(order, dist, _capi.f64ptr(n) if n is not None else None)
        return L.tm_ho_tables(C.byref(opt), None, None, None)

    assert rc(2, _capi.TM_HO_GAUSS_LOBATTO) == _capi.TM_OK          # every output may be NULL
    assert rc(0, 0) == _capi.TM_E_ARG and rc(9, 0) == _capi.TM_E_ARG and rc(2, 7) == _capi.TM_E_ARG
    assert L.tm_ho_tables(None, None, None, None) == _capi.TM_E_ARG
    P = _capi.TM_HO_PRESCRIBED
    assert rc(2, P) == _capi.TM_E_ARG                                # no nodes
    assert rc(2, P, [0.0, 0.3, 1.0]) == _capi.TM_OK
    assert rc(2, P, [0.0, 0.0, 1.0]) == _capi.TM_E_ARG               # not strictly increasing
    assert rc(2, P, [0.0, 1.2, 1.0]) == _capi.TM_E_ARG
    assert rc(2, P, [0.1, 0.5, 1.0]) == _capi.TM_E_ARG               # first not 0
    assert rc(2, P, [0.0, 0.5, 0.9]) == _capi.TM_E_ARG               # last not 1
    assert rc(2, P, [0.0, float("nan"), 1.0]) == _capi.TM_E_ARG
    assert rc(2, P, [0.0, float("inf"), 1.0]) == _capi.TM_E_ARG


# ------------------------------------------------------------------ host elevation against the reference
def blocks_for(p):
    """A multi-element bent block, and one block whose coordinates are of the size of its elements (a single element around the
    origin): there the Jacobian bar is not loose by |coordinate| / element size."""
    s = np.linspace(-0.5, 0.5, p + 1)
    small = np.stack([s[:, None] + 0.08 * np.sin(2.0 * s[None, :]), s[None, :] + 0.06 * s[:, None] ** 2 - 0.01], axis=-1)
    return [("bent", cfr.bent_clustered(3 * p + 1, 2 * p + 1)), ("origin", small)]


@pytest.mark.parametrize("p", ORDERS)
def test_host_elevation_against_the_reference(p):
    for dist in DISTRIBUTIONS:
        for name, X in blocks_for(p):
            ref = hr.Reference(X, p, dist, hr.prescribed_nodes(p) if dist == "prescribed" else None)
            Y, q, sj = host_block(X, p, dist)
            ratio = hr.worst_ratio(Y, ref.Y, ref.bar_Y)
            print(f"ho_parity: host p {p} {dist} {name}: worst |Y - Y_ref| / bar {ratio:.3f}")
            assert ratio <= 1.0
            # J through what the record exposes: per element Jmin / Jmax, per block the extremes
            assert q.elements == ref.Ei * ref.Ej and q.order == p and q.orientation == ref.orientation == 1
            assert ref.decided().all() and q.invalid == ref.invalid == 0
            lo, hi = ref.sj_interval()
            assert np.all((sj >= lo) & (sj <= hi)), (dist, name)
            d = ref.delta.max()
            jr = (abs(LD(q.min_jacobian) - ref.jmin.min()) / d, abs(LD(q.max_jacobian) - ref.jmax.max()) / d)
            print(f"ho_parity: host p {p} {dist} {name}: worst |J - J_ref| / bar {float(max(jr)):.3f}")
            assert max(jr) <= 1.0
            assert q.min_scaled_jacobian == np.nanmin(sj) and (q.worst_e, q.worst_f) == np.unravel_index(np.nanargmin(sj), sj.shape)
            assert sum(q.hist) == q.elements - q.invalid
            assert np.array_equal(np.histogram(np.minimum(sj.ravel(), 0.95), bins=np.arange(11) / 10)[0], q.hist)


@pytest.mark.parametrize("p", ORDERS)
def test_equidistant_and_order_one_copy_the_nodes(p):
    X = cfr.bent_clustered(2 * p + 1, 3 * p + 1)
    X[0, 0, 1] = -0.0                                                   # copied: the sign of a zero survives
    Y, _, _ = host_block(X, p, "equidistant")
    assert np.array_equal(Y, X) and np.signbit(Y[0, 0, 1])
    if p == 1:
        for dist in DISTRIBUTIONS:
            assert np.array_equal(host_block(X, 1, dist)[0], X)


# ------------------------------------------------------------------ analytic pins
def polynomial_map(u, v, p, seed):
    """A map of degree <= p per index direction, in longdouble."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.0, 1.0, size=(2, p + 1, p + 1)) / (1 + np.add.outer(np.arange(p + 1), np.arange(p + 1)))
    U, V = np.broadcast_arrays(np.asarray(u, dtype=LD), np.asarray(v, dtype=LD))
    out = np.zeros(U.shape + (2,), dtype=LD)
    for k in range(2):
        for a in range(p + 1):
            for b in range(p + 1):
                out[..., k] += LD(c[k, a, b]) * U ** a * V ** b
    return out


@pytest.mark.parametrize("p", ORDERS)
def test_polynomial_maps_are_reproduced(p):
    """One element over [0, 1]^2: source nodes at u = m/p, the elevated nodes must be the map at the target points."""
    for dist in ("gauss_lobatto", "prescribed"):
        t = elevation(p, dist).tables()[0]
        s = np.arange(p + 1, dtype=LD) / p
        exact_src = polynomial_map(s[:, None], s[None, :], p, seed=p)
        X = exact_src.astype(np.float64)
        Y, _, _ = host_block(X, p, dist)
        want = polynomial_map(t.astype(LD)[:, None], t.astype(LD)[None, :], p, seed=p)
        ref = hr.Reference(X, p, dist, hr.prescribed_nodes(p) if dist == "prescribed" else None)
        # the sources were rounded to fp64 before the library saw them: half an ulp each, carried through |T| |T|; and p t_a is rounded
        # in the tables' argument, which the (2p+6) bar already holds
        aT = np.abs(hr.tables(p, dist, hr.prescribed_nodes(p))[0])
        src_round = hr.U * np.einsum("am,mnc,bn->abc", aT, np.abs(exact_src), aT)
        bar = ref.bar_Y + src_round
        ratio = hr.worst_ratio(Y, want, bar)
        print(f"ho_parity: polynomial map p {p} {dist}: worst error / bar {ratio:.3f}")
        assert ratio <= 1.0


@pytest.mark.parametrize("p", ORDERS)
def test_affine_map_has_constant_jacobian(p):
    M = np.array([[0.75, -0.25], [0.5, 1.25]])                          # dyadic: the map is exact in fp64 on the dyadic lattice below
    det = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
    ni, nj = 2 * p + 1, 3 * p + 1
    I, J = np.meshgrid(np.arange(ni) / 8.0, np.arange(nj) / 16.0, indexing="ij")
    X = np.stack([M[0, 0] * I + M[0, 1] * J + 0.5, M[1, 0] * I + M[1, 1] * J - 0.25], axis=-1)
    for dist in DISTRIBUTIONS:
        _, q, sj = host_block(X, p, dist)
        ref = hr.Reference(X, p, dist, hr.prescribed_nodes(p) if dist == "prescribed" else None)
        want = det / 8.0 / 16.0                                          # d/du per index step
        d = float(ref.delta.max())
        assert q.invalid == 0 and q.orientation == 1
        assert abs(q.min_jacobian - want) <= d and abs(q.max_jacobian - want) <= d
        assert np.all(np.abs(sj - 1.0) <= 2 * d / want + 4 * np.finfo(float).eps)
    Xneg = X[::-1].copy()                                                # the other handedness
    _, q, sj = host_block(Xneg, p, "gauss_lobatto")
    assert q.orientation == -1 and q.invalid == 0 and q.min_jacobian > 0 and np.all(np.abs(sj - 1.0) <= 1e-9)


@pytest.mark.parametrize("p", [2, 3, 5, 8])
def test_corners_are_unchanged_and_edges_depend_on_their_grid_line_only(p):
    X = cfr.bent_clustered(2 * p + 1, 2 * p + 1)
    Y, _, _ = host_block(X, p, "gauss_lobatto")
    assert np.array_equal(Y[::p, ::p], X[::p, ::p])
    rng = np.random.default_rng(p)
    Z = X.copy()
    off = np.ones((2 * p + 1, 2 * p + 1), dtype=bool)
    off[::p, :] = False
    off[:, ::p] = False                                                  # nodes on no element edge
    Z[off] += rng.uniform(-0.01, 0.01, size=(int(off.sum()), 2))
    Yz, _, _ = host_block(Z, p, "gauss_lobatto")
    assert np.array_equal(Yz[::p, :], Y[::p, :]) and np.array_equal(Yz[:, ::p], Y[:, ::p])
    assert not np.array_equal(Yz, Y)


# ------------------------------------------------------------------ invalid elements
FOLDED = [(2, 7, 9), (3, 10, 7), (4, 9, 13), (8, 17, 17)]


@pytest.mark.parametrize("p,ni,nj", FOLDED)
def test_folded_elements_are_found(p, ni, nj):
    clean = cfr.bent_clustered(ni, nj)
    folded = hr.fold(clean, p)
    for dist in ("gauss_lobatto", "equidistant"):
        ref_c, ref_f = hr.Reference(clean, p, dist), hr.Reference(folded, p, dist)
        assert ref_c.invalid == 0 and ref_f.invalid >= 1 and ref_f.valid.sum() >= 1
        assert ref_f.decided().all() and ref_c.decided().all()
        _, qc, _ = host_block(clean, p, dist)
        _, qf, sj = host_block(folded, p, dist)
        assert qc.invalid == ref_c.invalid and qf.invalid == ref_f.invalid
        assert np.array_equal(np.isnan(sj), ~ref_f.valid) and np.isnan(sj[0, 0])
        assert sum(qf.hist) == qf.elements - qf.invalid


def test_non_finite_coordinates_make_invalid_elements_and_nothing_else():
    X = cfr.bent_clustered(9, 9)
    X[1, 1, 0] = np.nan
    _, q, sj = host_block(X, 4, "gauss_lobatto")
    assert q.invalid == 1 and np.isnan(sj[0, 0]) and np.isfinite(sj[1, 1]) and np.isfinite(q.min_scaled_jacobian)
    X[:] = np.nan
    _, q, sj = host_block(X, 4, "gauss_lobatto")
    assert q.invalid == q.elements == 4 and np.isnan(q.min_scaled_jacobian) and (q.worst_block, q.worst_e, q.worst_f) == (0, 0, 0)
    assert np.isnan(q.min_jacobian) and np.isnan(q.max_jacobian) and sum(q.hist) == 0 and np.isnan(sj).all()


def test_total_of_block_records():
    a = host_block(cfr.bent_clustered(9, 9), 4, "gauss_lobatto")[1]
    b = host_block(hr.fold(cfr.bent_clustered(9, 13, seed=2), 4), 4, "gauss_lobatto")[1]
    b.worst_block = 1
    t = quality.total_ho([a, b])
    assert t.elements == a.elements + b.elements and t.invalid == b.invalid == 1 and t.order == 4 and t.orientation == 1
    assert t.min_scaled_jacobian == min(a.min_scaled_jacobian, b.min_scaled_jacobian)
    assert t.worst_block == (0 if a.min_scaled_jacobian <= b.min_scaled_jacobian else 1)
    assert t.min_jacobian == min(a.min_jacobian, b.min_jacobian) and t.max_jacobian == max(a.max_jacobian, b.max_jacobian)
    assert t.hist == tuple(x + y for x, y in zip(a.hist, b.hist))
    empty = quality.total_ho([])
    assert empty.elements == 0 and np.isnan(empty.min_scaled_jacobian)


# ------------------------------------------------------------------ checks, arguments
def test_check_passes_where_the_order_divides():
    for p in (1, 2, 4):
        elevation(p, "gauss_lobatto").check(configs.strip(3, 4 * 2 + 1, 8 + 1, tfi=oracle_tfi))
        elevation(p, "gauss_lobatto").check(configs.two_by_two(9, 13, tfi=oracle_tfi))
    elevation(3, "equidistant").check(configs.strip(2, 7, 10, tfi=oracle_tfi))


def test_check_names_the_offender():
    m = configs.strip(3, 9, 13, tfi=oracle_tfi)
    with pytest.raises(_capi.TmError) as e:
        elevation(3, "gauss_lobatto").check(m)                           # 8 cells along i
    assert e.value.code == _capi.TM_E_SIZE and "block 0" in str(e.value) and "order 3" in str(e.value)
    m.blocks[1] = cfr.single_block_mesh(cfr.bent_clustered(9, 12)).blocks[0]
    with pytest.raises(_capi.TmError) as e:
        elevation(4, "gauss_lobatto").check(m)                           # block 1 has 11 cells along j
    assert e.value.code == _capi.TM_E_SIZE and "block 1" in str(e.value)
    m = configs.strip(3, 9, 13, tfi=oracle_tfi)
    m.connections[1].ranges[0].start = 2                                 # off the element grid of order 4
    with pytest.raises(_capi.TmError) as e:
        elevation(4, "gauss_lobatto").check(m)
    assert e.value.code == _capi.TM_E_SIZE and "connection 1" in str(e.value) and "block 1" in str(e.value)
    elevation(2, "gauss_lobatto").check(m)                               # 2 lies on the grid of order 2


def test_arguments_of_the_host_call():
    m = cfr.single_block_mesh(cfr.bent_clustered(9, 9))
    md = _capi.MeshDesc(m)
    L = _capi.lib()
    x, y = np.empty(81), np.empty(81)
    q = _capi.tm_ho_quality()
    opt = _capi.tm_ho_opt(4, _capi.TM_HO_GAUSS_LOBATTO, None)
    assert L.tm_ho_elevate_host(md.ref(), C.byref(opt), 0, None, None, C.byref(q), None) == _capi.TM_OK and q.elements == 4   # a report alone
    assert L.tm_ho_elevate_host(md.ref(), C.byref(opt), 0, _capi.f64ptr(x), _capi.f64ptr(y), None, None) == _capi.TM_OK
    assert L.tm_ho_elevate_host(md.ref(), C.byref(opt), 0, _capi.f64ptr(x), None, None, None) == _capi.TM_E_ARG
    assert L.tm_ho_elevate_host(md.ref(), C.byref(opt), 1, None, None, C.byref(q), None) == _capi.TM_E_ARG
    assert L.tm_ho_elevate_host(None, C.byref(opt), 0, None, None, C.byref(q), None) == _capi.TM_E_ARG
    opt3 = _capi.tm_ho_opt(3, _capi.TM_HO_GAUSS_LOBATTO, None)
    assert L.tm_ho_elevate_host(md.ref(), C.byref(opt3), 0, None, None, C.byref(q), None) == _capi.TM_E_SIZE
    assert C.sizeof(_capi.tm_ho_opt) == 16 and C.sizeof(_capi.tm_ho_quality) == 152


# ------------------------------------------------------------------ writer
def lagrange_order_stated_here(p):
    """VTK's PointIndexFromIJK for a quadrilateral of order p, restated: index -> (a, b)."""
    out = {}
    for a in range(p + 1):
        for b in range(p + 1):
            ibdy, jbdy = a in (0, p), b in (0, p)
            if ibdy and jbdy:                                            # corners: (0,0), (p,0), (p,p), (0,p)
                k = (3 if b else 0) if a == 0 else (2 if b else 1)
            elif jbdy:                                                   # edges along a: b = 0 first, then (after edge a = p) b = p
                k = 4 + (a - 1) + (0 if b == 0 else (p - 1) + (p - 1))
            elif ibdy:                                                   # edges along b: a = p second, a = 0 fourth
                k = 4 + (b - 1) + ((p - 1) if a == p else 3 * (p - 1))
            else:
                k = 4 + 4 * (p - 1) + (a - 1) + (p - 1) * (b - 1)
            out[k] = (a, b)
    return [out[k] for k in range((p + 1) ** 2)]


@pytest.mark.parametrize("p", [1, 2, 3])
def test_vtk_round_trip_and_connectivity(p, tmp_path):
    assert highorder.lagrange_quad_order(p) == lagrange_order_stated_here(p)
    A, B = cfr.bent_clustered(2 * p + 1, 3 * p + 1), cfr.bent_clustered(p + 1, 2 * p + 1, seed=3)
    A[0, 0, 1] = -0.0
    m = cfr.single_block_mesh(A)
    m.addBlock("block_1", configs.block_from_array(B.copy()))
    hom = elevation(p, "equidistant").mesh(m, host=True)
    f = str(tmp_path / "curved.vtk")
    hom.write(f)
    points, cells, types = output.read_vtk_lagrange(f)
    want = np.concatenate([np.stack([x.reshape(-1), y.reshape(-1), np.zeros(x.size)], axis=1) for x, y in hom.blocks])
    assert points.shape == want.shape and np.array_equal(points, want) and np.array_equal(np.signbit(points), np.signbit(want))
    assert np.all(types == 70) and cells.shape == (2 * 3 + 1 * 2, (p + 1) ** 2)
    k, offset = 0, 0
    for X in (A, B):
        ni, nj = X.shape[:2]
        for f_ in range((nj - 1) // p):
            for e in range((ni - 1) // p):                               # elements with e fastest, like the sj plane
                for n, (a, b) in enumerate(lagrange_order_stated_here(p)):
                    i, j = e * p + a, f_ * p + b
                    assert cells[k, n] == offset + j * ni + i
                    assert points[cells[k, n], 0] == X[i, j, 0] and points[cells[k, n], 1] == X[i, j, 1]
                k += 1
        offset += ni * nj
    with pytest.raises(ValueError):
        elevation(p, "gauss_lobatto").mesh(m, host=True).write(f)        # Lagrange cells assume equidistant nodes
    g = str(tmp_path / "curved.xyz")
    hom2 = elevation(p, "gauss_lobatto").mesh(m, host=True)
    hom2.write(g)
    back = output.read_plot3d(g)
    assert [(b[0], b[1]) for b in back] == hom2.sizes()
    assert all(np.array_equal(b[2].T, hom2.blocks[k][0]) and np.array_equal(b[3].T, hom2.blocks[k][1]) for k, b in enumerate(back))
    assert hom2.total.elements == 8 and hom2.elements() == [(2, 3), (1, 2)]


def test_python_layer_refuses_what_it_cannot_serve():
    with pytest.raises(ValueError):
        highorder.Elevation(2, "chebyshev")
    with pytest.raises(ValueError):
        highorder.Elevation(2, "prescribed")
    with pytest.raises(ValueError):
        highorder.Elevation(2, "gauss_lobatto", nodes=[0, 0.5, 1])
    with pytest.raises(ValueError):
        highorder.Elevation(3, "prescribed", nodes=[0, 0.5, 1])

    class FakeHandle:
        _h = 1
        _mesh = cfr.single_block_mesh(cfr.bent_clustered(5, 5))

    with pytest.raises(ValueError):
        highorder.Elevation(2).block(FakeHandle(), 0, host=True)
