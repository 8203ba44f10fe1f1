"""CPU: the high-order certificate (include/tm_hip.h, "high-order elements: certificate") -- tm_ho_certify_tables, tm_ho_jacobian_bezier_host,
tm_ho_certify_host and the Python layer against tests/ho_certify_reference.py: exact rational arithmetic on dyadic inputs (ground truth
that owes nothing to rounding) and numpy longdouble.  The only tolerance is the derived guard g = G(p) 2^-53 R.  No GPU: the device side
is tests/test_gpu_ho_certify.py."""
import ctypes as C
import functools
from fractions import Fraction as Fr

import numpy as np
import pytest

from tests import control_field_reference as cfr
from tests import ho_certify_reference as cr
from tests import ho_reference as hr
from turbomesh_amd import _capi, highorder, quality

LD = np.longdouble
U = Fr(1, 2 ** 53)
ORDERS = range(1, 9)
PROVEN, INVALID, UNDECIDED = _capi.TM_HO_PROVEN, _capi.TM_HO_INVALID, _capi.TM_HO_UNDECIDED

# the issue's p = 2 element: J >= 0.171875 at all nine nodes, J(0, 1.5) = -1.31640625
HIDDEN_2 = np.stack([np.array([[-0.625, 0.375, -0.625], [0.375, 1.0, 0.5], [2.375, 2.375, 1.375]]),
                     np.array([[-0.125, 1.625, 1.5], [-0.375, 0.5, 2.125], [-0.75, 1.25, 2.5]])], axis=-1)
# p = 3, found by the same seeded search: valid at its sixteen nodes, J(1.5, 0) = -0.0404... and J < 0 at three more points k*3/4
HIDDEN_3 = np.stack([np.array([[-0.625, 0.375, -0.125, 0.375], [0.875, 1.125, 0.75, 1.375], [0.875, 1.25, 1.5, 1.625], [2.75, 2.5, 1.875, 2.25]]),
                     np.array([[-0.625, 0.625, 1.875, 2.375], [-0.25, 1.0, 1.5, 2.125], [-0.5, 0.625, 1.375, 2.25], [0.0, 0.875, 1.625, 2.875]])], axis=-1)


def elevation(p):
    return highorder.Elevation(p, "equidistant")


def host(X, p, max_depth=3):
    """(HoCertificate, status (Ei, Ej), bounds (Ei, Ej, 2)) of tm_ho_certify_host on one block."""
    c, st, bd = elevation(p).certify(cfr.single_block_mesh(X), 0, host=True, max_depth=max_depth)
    return c, st.T, bd.transpose(1, 0, 2)


@functools.lru_cache(maxsize=None)
def exact_tables(p):
    return cr.Tables(p, Fr)


@functools.lru_cache(maxsize=None)
def samplers(p):
    """exact J on the 33 x 33 grid k p/32 (it holds every patch corner up to depth 5) and at the element's nodes"""
    return cr.Sampler(p, cr.dyadic_points(p, 32)), cr.Sampler(p, [Fr(m) for m in range(p + 1)])


def guard(p, R):
    """g = G(p) 2^-53 R (exact), R = S + the cross products"""
    return exact_tables(p).G * U * R


# ------------------------------------------------------------------ tables
@pytest.mark.parametrize("p", ORDERS)
def test_tables(p):
    M, wu, wv, G, norm = elevation(p).certify_tables()
    Mr = cr.lagrange_to_bernstein(p)
    for i in range(p + 1):
        for m in range(p + 1):
            assert abs(Fr(float(M[i, m])) - Mr[i, m]) <= U * abs(Mr[i, m]), (i, m)      # one rounding of the exact value
    unit = np.eye(p + 1)
    assert np.array_equal(M[0], unit[0]) and np.array_equal(M[p], unit[p])
    wur, wvr = cr.weights(p)
    assert np.array_equal(wu, np.array(wur, dtype=np.float64)) and np.array_equal(wv, np.array(wvr, dtype=np.float64))
    for k in range(2 * p):                                                              # weights of coefficient (k, l) sum to 1
        for l in range(2 * p):
            s = sum(Fr(float(wu[k, i])) * Fr(float(wv[l, j])) for i in range(p) for j in range(p + 1))
            assert abs(s - 1) <= 4 * U
            assert sum(wur[k]) == 1 and sum(wvr[l]) == 1
    assert abs(Fr(norm) - cr.norm_inf(p)) <= U * cr.norm_inf(p)
    assert abs(Fr(G) - cr.guard_factor(p)) <= 4 * U * cr.guard_factor(p)
    print(f"ho_certify: p {p}: max |M| {np.abs(M).max():.4g} ||M||_inf {norm:.4g} G {G:.6g}")
    assert np.abs(M).max() >= 1.0 and (p == 1 or np.abs(M).max() >= 2.0)


# ------------------------------------------------------------------ coefficients
@pytest.mark.parametrize("p", [1, 2, 3, 4, 5, 8])
def test_coefficients_against_the_exact_reference(p):
    X = cr.dyadic_block(2 * p + 1, 2 * p + 1, 0.15, seed=10 + p)
    mesh = cfr.single_block_mesh(X)
    ref = hr.Reference(X, p, "equidistant")
    T = exact_tables(p)
    worst = 0.0
    for e in range(2):
        for f in range(2):
            B = elevation(p).jacobian_bezier(mesh, 0, e, f)
            Br, S, R = cr.jacobian_bezier(cr.element(X, p, e, f), T)
            g = guard(p, S)                                                             # with S alone: stricter than the guard (S <= R)
            err = max(abs(Fr(float(B[k, l])) - Br[k, l]) for k in range(2 * p) for l in range(2 * p))
            worst = max(worst, float(err / g))
            assert err <= g                                                             # the derived guard itself, not a measured bar
            # the four corner coefficients are J at the element's corners (K13's own reference, within its bar)
            N = 2 * p
            for (k, l), (a, b) in zip(((0, 0), (0, N - 1), (N - 1, 0), (N - 1, N - 1)), ((0, 0), (0, p), (p, 0), (p, p))):
                assert abs(LD(B[k, l]) - ref.J[e, f, a, b]) <= ref.bar_J[e, f, a, b] + LD(float(g))
    print(f"ho_certify: p {p}: worst |B - B_exact| / g {worst:.3g}")
    with pytest.raises(_capi.TmError) as err:
        elevation(p).jacobian_bezier(mesh, 0, 2, 0)
    assert err.value.code == _capi.TM_E_ARG


@pytest.mark.parametrize("ratio", [2 ** 14, 2 ** 17, 2 ** 20], ids=["r1.6e4", "r1.3e5", "r1.0e6"])
@pytest.mark.parametrize("p", [2, 3, 4, 5])
def test_thin_skewed_elements_stay_within_the_guard(p, ratio):
    """Boundary-layer cells at an angle to the axes: the rounding of the conversion is relative to the element's extent in both
    directions, so it scales with the cross products, which S leaves out and R holds.  Coefficients within g = G u R of the exact
    ones, the element proven, and its bounds around the exact Jacobian at the corners and on a 9 x 9 sample."""
    X = cr.stretched_block(p, ratio, seed=7 * p + ratio % 1000)
    mesh = cfr.single_block_mesh(X)
    B = elevation(p).jacobian_bezier(mesh, 0, 0, 0)
    Br, S, R = cr.jacobian_bezier(X, exact_tables(p))
    g = guard(p, R)
    err = max(abs(Fr(float(B[k, l])) - Br[k, l]) for k in range(2 * p) for l in range(2 * p))
    print(f"ho_certify: p {p} aspect {ratio}: |B - B_exact| / g {float(err / g):.3g} (against G u S: {float(err / guard(p, S)):.3g}); R / S {float(R / S):.3g}")
    assert R > 1000 * S and err <= g
    c, st, bd = host(X, p)
    assert st[0, 0] == PROVEN and c.proven == 1 and c.decided_at[0] == 1
    J = cr.Sampler(p, cr.dyadic_points(p, 8))(X)
    lo, hi = Fr(float(bd[0, 0, 0])), Fr(float(bd[0, 0, 1]))
    assert 0 < lo <= min(J.reshape(-1)) and hi >= max(J.reshape(-1))
    N = 2 * p
    for (k, l), (a, b) in zip(((0, 0), (0, N - 1), (N - 1, 0), (N - 1, N - 1)), ((0, 0), (0, 8), (8, 0), (8, 8))):
        assert Br[k, l] == J[a, b] and lo <= J[a, b] <= hi                             # corner coefficients ARE the corner Jacobians
    sj = elevation(p).block(mesh, 0, host=True, planes=False)[3].T
    assert bd[0, 0, 0] / bd[0, 0, 1] <= sj[0, 0]


# ------------------------------------------------------------------ folds the nodes do not see
@pytest.mark.parametrize("p,X,point,level", [(2, HIDDEN_2, (Fr(0), Fr(3, 2)), 2), (3, HIDDEN_3, (Fr(3, 2), Fr(0)), 1)], ids=["p2", "p3"])
def test_hidden_fold(p, X, point, level):
    """level: the first subdivision level whose patch corners include a point with J <= 0 (k p/4 at level 2, k p/2 at level 1)"""
    mesh = cfr.single_block_mesh(X)
    q = elevation(p).block(mesh, 0, host=True, planes=False)[2]
    assert q.invalid == 0 and q.orientation == 1 and q.min_jacobian > 0                 # K13: valid
    if p == 2:
        assert q.min_jacobian == 0.171875
    at_point = cr.jacobian_at(X, p, *point)
    assert at_point < 0 and (p != 2 or at_point == Fr(-1.31640625))                    # folded at a point k p/4
    grid = cr.Sampler(p, cr.dyadic_points(p, 4))(X)
    assert min(grid.reshape(-1)) <= at_point
    B = cr.jacobian_bezier(X, exact_tables(p))[0]
    Bl, _, Rl = cr.jacobian_bezier(X, cr.Tables(p, LD))
    gl = cr.Tables(p, LD).G * LD(2.0) ** -53 * Rl
    for depth in range(5):
        c, st, bd = host(X, p, depth)
        want = UNDECIDED if depth < level else INVALID
        exact = cr.decide(B, 1, 0, depth)
        assert st[0, 0] == want == exact["status"] == cr.decide(Bl, 1, gl, depth)["status"], depth
        assert c.hidden_invalid == (1 if depth >= level else 0) and c.invalid == c.hidden_invalid and c.undecided == 1 - c.invalid
        assert c.proven == 0 and c.has_unproven and (c.first_unproven_e, c.first_unproven_f) == (0, 0) and np.isnan(c.min_scaled_bound)
        assert c.decided_at == (tuple(int(L == level) for L in range(5)) if depth >= level else (0,) * 5) and c.max_depth == depth and c.order == p
        assert Fr(float(bd[0, 0, 0])) <= exact["lo"] and Fr(float(bd[0, 0, 1])) >= exact["hi"]
        assert Fr(float(bd[0, 0, 0])) <= at_point


# ------------------------------------------------------------------ sound both ways
# orders 2 .. 5: the degree-8 interpolant of uncorrelated noise oscillates so much (derivative coefficients of 1e4 cells) that its guard
# exceeds the cell area and every coefficient lies within 2 g; order 8 is held to the exact coefficients above and to smooth blocks below
SOUND = [(p, amp) for p in (2, 3, 4, 5) for amp in (0.05, 0.15, 0.35)]


@functools.lru_cache(maxsize=None)
def sound_case(p, amp):
    """One seeded dyadic block with the fp64 verdicts and the exact ones: computed once, shared, never modified."""
    Ei, Ej = (4, 3) if p <= 4 else (2, 1)
    X = cr.dyadic_block(Ei * p + 1, Ej * p + 1, amp, seed=100 * p + int(100 * amp))
    c, st, bd = host(X, p)
    q, sj = elevation(p).block(cfr.single_block_mesh(X), 0, host=True, planes=False)[2:]
    grid, nodes = samplers(p)
    rows = []
    for e in range(Ei):
        for f in range(Ej):
            Xe = cr.element(X, p, e, f)
            B, _, R = cr.jacobian_bezier(Xe, exact_tables(p))
            Jg, Jn = grid(Xe), nodes(Xe)
            nodal_valid = min(Jn.reshape(-1)) > 0
            rows.append(dict(e=e, f=f, g=guard(p, R), exact=cr.decide(B, 1, 0, 3, nodal_valid), grid_min=min(Jg.reshape(-1)), grid_max=max(Jg.reshape(-1)),
                             node_min=min(Jn.reshape(-1))))
    return X, c, st, bd, q, sj.T, rows


@pytest.mark.parametrize("p,amp", SOUND)
def test_sound_both_ways(p, amp):
    X, c, st, bd, q, sj, rows = sound_case(p, amp)
    assert q.orientation == c.orientation == 1
    excluded = 0
    for r in rows:
        e, f = r["e"], r["f"]
        s = st[e, f]
        lo, hi = Fr(float(bd[e, f, 0])), Fr(float(bd[e, f, 1]))
        if s == PROVEN:                                                                 # no proven element has a non-positive exact J anywhere sampled
            assert r["grid_min"] > 0 and r["node_min"] > 0, (e, f)
            assert lo > 0 and bd[e, f, 0] / bd[e, f, 1] <= sj[e, f], (e, f)              # sb <= K13's sampled sj
        if s == INVALID:                                                                # no invalid element lacks a non-positive exact value
            assert min(r["grid_min"], r["node_min"]) <= 0, (e, f)
        assert lo <= r["grid_min"] and hi >= r["grid_max"], (e, f)                      # bounds hold on the exact sample
        if r["exact"]["min_abs"] > 2 * r["g"]:
            assert s == r["exact"]["status"], (e, f, s, r["exact"])
        else:
            excluded += 1
    assert excluded == 0                                                                # the seeds were chosen so that nothing needs excluding
    assert c.proven == (st == PROVEN).sum() and c.invalid == (st == INVALID).sum() and c.undecided == (st == UNDECIDED).sum()
    assert c.proven + c.invalid + c.undecided == c.elements == st.size and sum(c.decided_at) == c.proven + c.invalid
    assert c.hidden_invalid == sum(1 for r in rows if st[r["e"], r["f"]] == INVALID and not np.isnan(sj[r["e"], r["f"]]))
    unproven = [(r["e"], r["f"]) for r in rows if st[r["e"], r["f"]] != PROVEN]
    assert c.has_unproven == bool(unproven) and (not unproven or (c.first_unproven_e, c.first_unproven_f) == min(unproven))
    if c.proven:
        sb = np.where(st == PROVEN, bd[..., 0] / bd[..., 1], np.inf)
        assert c.min_scaled_bound == sb.min() and (c.worst_e, c.worst_f) == np.unravel_index(np.argmin(sb), sb.shape)
    else:
        assert np.isnan(c.min_scaled_bound)


def test_all_three_verdicts_occur():
    seen = set()
    for p, amp in SOUND:
        seen |= set(np.unique(sound_case(p, amp)[2]).tolist())
    assert seen == {PROVEN, INVALID, UNDECIDED}
    assert sum(sound_case(p, amp)[1].hidden_invalid for p, amp in SOUND) >= 1


# ------------------------------------------------------------------ geometry that is not folded
def unfolded_blocks(p):
    ni, nj = 3 * p + 1, 2 * p + 1
    i, j = np.meshgrid(np.arange(ni, dtype=np.float64), np.arange(nj, dtype=np.float64), indexing="ij")
    affine = np.stack([2.0 * i + 0.5 * j + 3.0, -0.25 * i + 1.5 * j - 7.0], axis=-1)
    a, b = i / (ni - 1), j / (nj - 1)
    bilinear = np.stack([a * (1 + 0.5 * b), b * (1 + 0.25 * a) + 0.1 * a], axis=-1)
    sinus = np.stack([a + 0.03 * np.sin(2.0 * b + 0.3), 0.7 * b + 0.02 * np.sin(3.0 * a)], axis=-1)
    return [("affine", affine), ("bilinear", bilinear), ("sinusoidal", sinus)]


@pytest.mark.parametrize("p", ORDERS)
def test_unfolded_geometry_is_proven_without_subdivision(p):
    for name, X in unfolded_blocks(p):
        c, st, bd = host(X, p, max_depth=0)
        assert c.proven == c.elements == 6 and not c.has_unproven and c.decided_at == (6, 0, 0, 0, 0), name
        assert np.all(st == PROVEN) and np.all(bd[..., 0] > 0) and np.all(bd[..., 1] >= bd[..., 0])
        sj = elevation(p).block(cfr.single_block_mesh(X), 0, host=True, planes=False)[3].T
        assert np.all(bd[..., 0] / bd[..., 1] <= sj) and c.min_scaled_bound == (bd[..., 0] / bd[..., 1]).min()
        # a mirrored block has orientation -1 and the same verdict
        cm = host(X[::-1].copy(), p, max_depth=0)[0]
        assert cm.orientation == -1 and cm.proven == 6
        # longdouble evaluation of the definition: proven at level 0 too, the bounds within the guard of each other
        T = cr.Tables(p, LD)
        B, _, R = cr.jacobian_bezier(cr.element(X, p, 1, 1), T)
        g = T.G * LD(2.0) ** -53 * R
        d = cr.decide(B, 1, g, 0)
        assert d["status"] == PROVEN and abs(d["lo"] - LD(bd[1, 1, 0])) <= 2 * g and abs(d["hi"] - LD(bd[1, 1, 1])) <= 2 * g


def test_the_distribution_is_validated_and_otherwise_ignored():
    X = cr.dyadic_block(9, 9, 0.35, seed=7)
    mesh = cfr.single_block_mesh(X)
    ref = elevation(4).certify(mesh, 0, host=True)
    for el in (highorder.Elevation(4, "gauss_lobatto"), highorder.Elevation(4, "prescribed", hr.prescribed_nodes(4))):
        got = el.certify(mesh, 0, host=True)
        assert bytes(got[0].to_struct()) == bytes(ref[0].to_struct()) and np.array_equal(got[1], ref[1]) and got[2].tobytes() == ref[2].tobytes()


@pytest.mark.parametrize("p,ni,nj", [(2, 7, 9), (3, 10, 7), (4, 9, 13), (8, 17, 17)])
def test_folded_elements(p, ni, nj):
    folded = hr.fold(cfr.bent_clustered(ni, nj), p)
    q = elevation(p).block(cfr.single_block_mesh(folded), 0, host=True, planes=False)[2]
    c, st, _ = host(folded, p)
    assert q.invalid >= 1 and c.invalid >= q.invalid and st[0, 0] == INVALID
    assert c.hidden_invalid == c.invalid - q.invalid                                   # every nodal-invalid element is invalid here
    assert host(cfr.bent_clustered(ni, nj), p)[0].invalid == 0


def test_non_finite_coordinates_are_invalid():
    X = cfr.bent_clustered(9, 9).copy()
    X[2, 2, 0] = np.nan
    c, st, bd = host(X, 4)
    assert st[0, 0] == INVALID and c.invalid >= 1 and c.hidden_invalid == 0


# ------------------------------------------------------------------ arguments, totals
def test_arguments_of_the_host_call():
    m = cfr.single_block_mesh(cfr.bent_clustered(9, 9))
    md = _capi.MeshDesc(m)
    L = _capi.lib()
    cert = _capi.tm_ho_certificate()
    status = np.empty(4, dtype=np.uint8)
    sp = status.ctypes.data_as(C.POINTER(C.c_uint8))
    bounds = np.empty(8)

    def rc(order=4, dist=_capi.TM_HO_GAUSS_LOBATTO, nodes=None, depth=3, block=0, mesh=md.ref()):
        n = None if nodes is None else np.asarray(nodes, dtype=np.float64)
        opt = _capi.tm_ho_opt(order, dist, _capi.f64ptr(n) if n is not None else None)
        return L.tm_ho_certify_host(mesh, C.byref(opt), depth, block, C.byref(cert), sp, _capi.f64ptr(bounds))

    assert rc() == _capi.TM_OK and cert.elements == 4 and cert.proven == 4
    opt = _capi.tm_ho_opt(4, 0, None)
    assert L.tm_ho_certify_host(md.ref(), C.byref(opt), 3, 0, None, None, None) == _capi.TM_OK                 # every output may be NULL
    for depth in (0, 4):
        assert rc(depth=depth) == _capi.TM_OK and cert.max_depth == depth
    assert rc(depth=-1) == _capi.TM_E_ARG and rc(depth=5) == _capi.TM_E_ARG
    assert rc(order=0) == _capi.TM_E_ARG and rc(order=9) == _capi.TM_E_ARG and rc(dist=7) == _capi.TM_E_ARG
    assert rc(dist=_capi.TM_HO_PRESCRIBED) == _capi.TM_E_ARG                                                   # no nodes
    assert rc(dist=_capi.TM_HO_PRESCRIBED, nodes=[0.0, 0.2, 0.5, 0.7, 1.0]) == _capi.TM_OK
    assert rc(dist=_capi.TM_HO_PRESCRIBED, nodes=[0.0, 0.5, 0.5, 0.7, 1.0]) == _capi.TM_E_ARG
    assert rc(block=1) == _capi.TM_E_ARG and rc(mesh=None) == _capi.TM_E_ARG
    assert L.tm_ho_certify_host(md.ref(), None, 3, 0, C.byref(cert), sp, _capi.f64ptr(bounds)) == _capi.TM_E_ARG
    assert rc(order=3) == _capi.TM_E_SIZE and b"block 0" in L.tm_last_error()
    nocoords = _capi.MeshDesc(m, with_coordinates=False)
    assert rc(mesh=nocoords.ref()) == _capi.TM_E_ARG
    assert L.tm_ho_certify_tables(None, None, None, None, None, None) == _capi.TM_E_ARG
    assert L.tm_ho_certify_tables(C.byref(opt), None, None, None, None, None) == _capi.TM_OK
    assert L.tm_ho_jacobian_bezier_host(md.ref(), C.byref(opt), 0, 0, 0, None) == _capi.TM_E_ARG
    assert C.sizeof(_capi.tm_ho_certificate) == 152
    with pytest.raises(_capi.TmError):
        elevation(4).certify(m, 0, host=True, max_depth=5)


def test_total_of_block_certificates():
    a = host(cfr.bent_clustered(9, 9), 4)[0]
    b = host(hr.fold(cfr.bent_clustered(9, 13, seed=2), 4), 4)[0]
    b.worst_block = b.first_unproven_block = 1
    t = quality.total_ho_certificate([a, b])
    assert t.elements == a.elements + b.elements and t.proven == a.proven + b.proven and t.invalid == b.invalid >= 1
    assert t.undecided == a.undecided + b.undecided and t.hidden_invalid == a.hidden_invalid + b.hidden_invalid
    assert t.decided_at == tuple(x + y for x, y in zip(a.decided_at, b.decided_at)) and t.order == 4 and t.orientation == 1 and t.max_depth == 3
    assert t.min_scaled_bound == min(a.min_scaled_bound, b.min_scaled_bound)
    assert t.worst_block == (0 if a.min_scaled_bound <= b.min_scaled_bound else 1)
    assert t.has_unproven and (t.first_unproven_block, t.first_unproven_e, t.first_unproven_f) == (1, b.first_unproven_e, b.first_unproven_f)
    c = host(cfr.bent_clustered(9, 9), 4, max_depth=1)[0]
    assert quality.total_ho_certificate([a, c]).max_depth == -1
    empty = quality.total_ho_certificate([])
    assert empty.elements == 0 and np.isnan(empty.min_scaled_bound) and not empty.has_unproven
    total, per_block, status, bounds = elevation(4).certify(cfr.single_block_mesh(cfr.bent_clustered(9, 9)), host=True)
    assert bytes(total.to_struct()) == bytes(a.to_struct()) and len(per_block) == len(status) == len(bounds) == 1


def test_log_lines(caplog):
    import logging

    a = host(HIDDEN_2, 2)[0]
    with caplog.at_level(logging.INFO, logger="quality"):
        quality.log_report_ho_certificate(logging.getLogger("quality"), ["block_0"], [a], quality.total_ho_certificate([a]))
    lines = [r.getMessage() for r in caplog.records]
    assert len(lines) == 2 and lines[0].startswith("certify block_0: order 2 depth 3 elements 1 proven 0 invalid 1 undecided 0 hidden invalid 1")
    assert "first unproven (block 0, e 0, f 0)" in lines[1] and lines[1].startswith("certify total:")


# ------------------------------------------------------------------ CLI: what the exit code says (the solve replaced by host records)
def test_cli_exit_codes(monkeypatch):
    from types import SimpleNamespace

    from turbomesh_amd import __main__ as cli

    def run_on(X, p):
        def _run(ap, args, config, keep=None, tag=""):
            mesh = cfr.single_block_mesh(X)
            el = elevation(p)
            stats = {"highorder": el.mesh(mesh, host=True)}
            if args.certify is not None:
                total, per_block, _, _ = el.certify(mesh, host=True, max_depth=args.certify)
                stats["certificate"] = {"per_block": per_block, "total": total}
            return SimpleNamespace(output=None), mesh, None, stats, None
        monkeypatch.setattr(cli, "_run", _run)

    def main(*flags):
        try:
            cli.main(["x.json", "--order", "2", *flags])
        except SystemExit as e:
            return e.code
        return 0

    run_on(HIDDEN_2, 2)
    assert main() == 0 and main("--fail-on-invalid-elements") == 0                      # the nodal record alone sees nothing
    assert main("--certify") == 0                                                       # reported, not failed
    msg = main("--certify", "--fail-on-invalid-elements")
    assert isinstance(msg, str) and "1 elements of order 2 are valid at their nodes and folded between them (1 invalid by the certificate)" in msg
    msg = main("--certify", "--fail-on-unproven-elements")
    assert isinstance(msg, str) and "1 of 1 elements of order 2 are not proven valid (1 invalid, 0 undecided at depth 3; first: block 0, e 0, f 0)" in msg
    assert main("--certify", "1", "--fail-on-invalid-elements") == 0                    # depth 1 leaves it undecided: not invalid ...
    msg = main("--certify", "1", "--fail-on-unproven-elements")
    assert isinstance(msg, str) and "(0 invalid, 1 undecided at depth 1; first: block 0, e 0, f 0)" in msg   # ... but not proven either
    big = cfr.bent_clustered(15, 11) * 40.0
    big[6:9, 4:7] = HIDDEN_2 + big[6, 4] - HIDDEN_2[0, 0]
    run_on(big, 2)
    t = host(big, 2)[0]                                                                 # the neighbours share the replaced edges: several fall
    msg = main("--certify", "--fail-on-unproven-elements")
    assert t.invalid >= 1 and (t.first_unproven_e, t.first_unproven_f) != (0, 0)
    assert isinstance(msg, str) and f"{t.invalid} of 35 elements" in msg and f"first: block 0, e {t.first_unproven_e}, f {t.first_unproven_f})" in msg
    run_on(hr.fold(cfr.bent_clustered(7, 9), 2), 2)                                     # folded at a node: the nodal message, as before
    msg = main("--certify", "--fail-on-invalid-elements")
    assert isinstance(msg, str) and "invalid elements of order 2 after smoothing" in msg
    run_on(cfr.bent_clustered(7, 9), 2)
    assert main("--certify", "--fail-on-invalid-elements", "--fail-on-unproven-elements") == 0
    assert main("--certify", "5") == 2 and main("--fail-on-unproven-elements") == 2
    monkeypatch.undo()
    try:
        cli.main(["x.json", "--certify"])
    except SystemExit as e:
        assert e.code == 2
