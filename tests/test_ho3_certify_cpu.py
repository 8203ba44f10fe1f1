"""CPU: the certificate of high-order hexahedra (include/tm_hip.h, "high-order hexahedra: certificate") -- tm_ho3_certify_tables,
tm_ho3_jacobian_bezier_host, tm_ho3_certify_planes_host, tm_stack_certify_host and the Python layer against tests/ho3_certify_reference.py:
exact rational arithmetic on dyadic inputs, by a route the library does not take (J sampled by Lagrange interpolation, converted to the
Bernstein basis).  The only tolerance is the derived guard g = G3(p) 2^-53 R3.  No GPU: the device side is tests/test_gpu_ho3_certify.py."""
import ctypes as C
import dataclasses
import functools
from fractions import Fraction as Fr

import numpy as np
import pytest

from tests import control_field_reference as cfr
from tests import ho3_certify_reference as r3
from tests import ho_certify_reference as cr
from tests import stack_reference as sr
from tests import stack_surface_reference as ssr
from tests.test_highorder3_cpu import bent_cuts, cut_meshes, stack_for
from turbomesh_amd import _capi, highorder, quality, stack

U = Fr(1, 2 ** 53)
ORDERS = (1, 2, 3, 4)
PROVEN, INVALID, UNDECIDED = _capi.TM_HO_PROVEN, _capi.TM_HO_INVALID, _capi.TM_HO_UNDECIDED

# the 2-D certificate's elements (tests/test_ho_certify_cpu.py, copied): valid at all their nodes and folded between them.
# p = 2: J >= 0.171875 at all nine nodes, J(0, 1.5) = -1.31640625, decided at level 2; p = 3: J(1.5, 0) = -0.0404..., decided at level 1
HIDDEN = {
    2: np.stack([np.array([[-0.625, 0.375, -0.625], [0.375, 1.0, 0.5], [2.375, 2.375, 1.375]]),
                 np.array([[-0.125, 1.625, 1.5], [-0.375, 0.5, 2.125], [-0.75, 1.25, 2.5]])], axis=-1),
    3: np.stack([np.array([[-0.625, 0.375, -0.125, 0.375], [0.875, 1.125, 0.75, 1.375], [0.875, 1.25, 1.5, 1.625], [2.75, 2.5, 1.875, 2.25]]),
                 np.array([[-0.625, 0.625, 1.875, 2.375], [-0.25, 1.0, 1.5, 2.125], [-0.5, 0.625, 1.375, 2.25], [0.0, 0.875, 1.625, 2.875]])], axis=-1),
}
HIDDEN_LEVEL = {2: 2, 3: 1}
# node noise in cells, per order, chosen on the CPU with the host definition.  ROUGH (with ROUGH_SEEDS draws): the rough inputs of
# tests/test_gpu_ho3_certify.py show every verdict and every deciding level 0 .. 3 (asserted there).  SOUND: the soundness blocks below
# hold at least one proven and one invalid element with at most half undecided at depth 3 (asserted below).
ROUGH = {1: (0.5, 0.5), 2: (0.5, 0.3), 3: (0.24, 0.16), 4: (0.14, 0.09)}   # draw `seed` takes entry seed % 2
ROUGH_SEEDS = {1: 2, 2: 4, 3: 16, 4: 16}
SOUND = {1: 0.5, 2: 0.3, 3: 0.16, 4: 0.1}


def elevation(p):
    return highorder.Elevation(p, "equidistant")


def same_certificate(a, b):
    """Every field equal bit for bit (NaN equals NaN)."""
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(dataclasses.astuple(a), dataclasses.astuple(b)))


def extruded(p):
    """HIDDEN[p] extruded to p+1 layers, z = the layer index: (nk, nj, ni) planes.  J3 = J2 exactly."""
    n = p + 1
    X = np.broadcast_to(HIDDEN[p][:, :, 0].T, (n, n, n)).copy()
    Y = np.broadcast_to(HIDDEN[p][:, :, 1].T, (n, n, n)).copy()
    Z = np.broadcast_to(np.arange(n, dtype=np.float64)[:, None, None], (n, n, n)).copy()
    return X, Y, Z


def smooth_cuts(ni, nj, K, p, seed=0):
    """The same bent, clustered cut, growing with the span."""
    return [cfr.bent_clustered(ni, nj) * (1.0 + 0.02 * c) for c in range(K)]


def rough_cuts(ni, nj, K, p, seed=0):
    """Cuts of 0.05-cells with uncorrelated node noise of ROUGH[p] cells, another draw per cut and seed."""
    i, j = np.meshgrid(np.arange(ni, dtype=np.float64), np.arange(nj, dtype=np.float64), indexing="ij")
    if p >= 2 and seed == ROUGH_SEEDS[p] - 1:
        # the last draw is no noise but a cut whose Jacobian grazes zero: x = i, y = j q(i), q = (i - 0.3)^2 + 0.001, so J = q > 0 with
        # its minimum off every dyadic point: the first element column is valid and stays undecided at depth 3
        return [0.05 * np.stack([i, j * ((i - 0.3) ** 2 + 0.001)], axis=-1)] * K
    out = []
    for c in range(K):
        rng = np.random.default_rng(7919 * seed + 101 * c + 13 * p + ni)
        amp = ROUGH[p][seed % len(ROUGH[p])]
        out.append(0.05 * (np.stack([i, j], axis=-1) + rng.uniform(-amp, amp, (ni, nj, 2))) + 0.002 * c)
    return out


def curved_cuts(ni, nj, K, p, seed=0):
    """An annulus sector, a quarter radian per element along i: strongly curved elements of negative orientation."""
    i, j = np.meshgrid(np.arange(ni, dtype=np.float64), np.arange(nj, dtype=np.float64), indexing="ij")
    out = []
    for c in range(K):
        th, r = (0.25 / p) * i + 0.02 * c, 1.0 + (0.1 / p) * j * (1.0 + 0.05 * c)
        out.append(np.stack([r * np.cos(th), r * np.sin(th)], axis=-1))
    return out


def worst_error(B, Br):
    return max(abs(Fr(float(a)) - b) for a, b in zip(B.reshape(-1), Br.reshape(-1)))


# ------------------------------------------------------------------ tables
@pytest.mark.parametrize("p", ORDERS)
def test_tables(p):
    M, wA, wB, G, norm = elevation(p).certify3d_tables()
    Mr = cr.lagrange_to_bernstein(p)
    for i in range(p + 1):
        for m in range(p + 1):
            assert abs(Fr(float(M[i, m])) - Mr[i, m]) <= U * abs(Mr[i, m]), (i, m)      # one rounding of the exact value
    unit = np.eye(p + 1)
    assert np.array_equal(M[0], unit[0]) and np.array_equal(M[p], unit[p])
    pa, pb = r3.weight_pairs(p)
    assert len(wA) == 3 and len(wB) == 2
    for w, (a, b) in list(zip(wA, pa)) + list(zip(wB, pb)):
        ref = r3.product_weights(a, b)
        assert w.shape == (a + b + 1, a + 1)
        assert np.array_equal(w, np.array([[float(v) for v in row] for row in ref]))       # float(Fraction) is the one correct rounding
        assert all(sum(row) == 1 for row in ref)                                           # each row sums to 1 exactly in the reference
    assert abs(Fr(norm) - cr.norm_inf(p)) <= U * cr.norm_inf(p)
    assert abs(Fr(G) - r3.guard_factor(p)) <= 4 * U * r3.guard_factor(p)
    print(f"ho3_certify: p {p}: ||M||_inf {norm:.4g} G3 {G:.6g}")


# ------------------------------------------------------------------ coefficients
@pytest.mark.parametrize("p", ORDERS)
def test_coefficients_against_the_exact_reference(p):
    X, Y, Z = r3.dyadic_block(2 * p + 1, 2 * p + 1, 2 * p + 1, 0.15, seed=10 + p)
    el = elevation(p)
    corner_sampler = r3.Sampler(p, [Fr(0), Fr(p)])
    worst = 0.0
    elements = [(e, f, g) for g in range(2) for f in range(2) for e in range(2)] if p < 4 else [(1, 0, 1)]   # p = 4: one element keeps the exact reference within seconds
    for e, f, g in elements:
        B = highorder.jacobian_bezier3d(X, Y, Z, el, e, f, g)
        Xe = r3.element(X, Y, Z, p, e, f, g)
        Br = r3.exact_bezier(Xe, p)
        gd, _, _ = r3.guard(Xe, p)
        err = worst_error(B, Br)
        worst = max(worst, float(err / gd))
        assert err <= gd                                                                # the derived guard itself, not a measured bar
        Jc = corner_sampler(Xe)                                                         # exact J at the eight corners
        N = 3 * p
        for a in (0, 1):
            for b in (0, 1):
                for c in (0, 1):
                    assert abs(Fr(float(B[a * (N - 1), b * (N - 1), c * (N - 1)])) - Jc[a, b, c]) <= gd
    print(f"ho3_certify: p {p}: worst |B - B_exact| / g {worst:.3g} over {len(elements)} elements")
    for bad in ((2, 0, 0), (0, 2, 0), (0, 0, 2)):
        with pytest.raises(_capi.TmError) as err:
            highorder.jacobian_bezier3d(X, Y, Z, el, *bad)
        assert err.value.code == _capi.TM_E_ARG


@pytest.mark.parametrize("p", [2, 3])
def test_extrusion_pins_the_3d_code_to_the_2d_certificate(p):
    X, Y, Z = extruded(p)
    el = elevation(p)
    B = highorder.jacobian_bezier3d(X, Y, Z, el, 0, 0, 0)
    B2, _, _ = cr.jacobian_bezier(HIDDEN[p], cr.Tables(p, Fr))                          # the exact 2-D coefficients
    Xe = r3.element(X, Y, Z, p, 0, 0, 0)
    gd, _, _ = r3.guard(Xe, p)
    err = worst_error(B, r3.elevate_degree(B2, p))                                      # J3 = J2: the exact degree elevation
    print(f"ho3_certify: extruded p {p}: |B - elevated B2| / g {float(err / gd):.3g}")
    assert err <= gd
    _, _, _, q, sj = highorder.planes3d(X, Y, Z, el, planes=False)
    assert q.invalid == 0 and np.isfinite(sj).all()                                     # valid at all its nodes
    c, status, _ = highorder.certify3d(X, Y, Z, el, 3)
    assert status[0, 0, 0] == INVALID and c.invalid == 1 and c.hidden_invalid == 1
    assert c.decided_at[HIDDEN_LEVEL[p]] == 1 and sum(c.decided_at) == 1                # the level the 2-D facts give
    for depth in range(HIDDEN_LEVEL[p]):
        assert highorder.certify3d(X, Y, Z, el, depth)[1][0, 0, 0] == UNDECIDED


def test_a_fold_only_the_3d_certificate_sees():
    """Two clean cuts: a square grid, and the same grid turned by half a turn and stretched 3 x in y.  Linear stacking gives the
    in-plane map (1-t) I + t A with determinant (1 - 2t)(1 - 4t): negative for 1/4 < t < 1/2, between the layers, positive at both."""
    n = 5
    i, j = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    cut0 = np.stack([i - 2.0, j - 2.0], axis=-1)
    cut1 = np.stack([-(i - 2.0), -3.0 * (j - 2.0)], axis=-1)
    for p, nk in ((1, 2), (2, 3)):
        el = elevation(p)
        for cut in (cut0, cut1):                                                        # the per-cut 2-D certificates are proven
            c2, _, _ = el.certify(cfr.single_block_mesh(cut), 0, host=True)
            assert c2.proven == c2.elements and c2.elements == ((n - 1) // p) ** 2
        st = stack.Stack([0.0, 1.0], np.linspace(0.0, 1.0, nk), "linear", "planar")
        c, status, bounds = st.certify(cut_meshes([cut0, cut1]), el, 0, host=True, max_depth=3)
        assert c.elements == ((n - 1) // p) ** 2 and c.invalid == c.elements and (status == INVALID).all()
        if p == 1:                                                                      # no node between the layers: only the certificate sees it
            assert c.hidden_invalid == c.elements and c.decided_at[0] == 0
        assert (bounds[..., 0] < 0).all()


def thin_block(p, ratio, seed, quantum=256):
    """One element of order p with aspect ratio `ratio` (a power of two): long side along (3, 1, 0), short sides along (-1, 3, 0) and z,
    nodes displaced by up to 0.05 of the short cell, every coordinate a multiple of 1/quantum."""
    rng = np.random.default_rng(seed)
    s = np.arange(p + 1, dtype=np.float64)
    l, n, m = np.meshgrid(s, s, s, indexing="ij")                                       # (nk, nj, ni)
    noise = lambda: rng.uniform(-0.05, 0.05, m.shape)   # noqa: E731
    X, Y, Z = 3.0 * ratio * m - n + noise(), 1.0 * ratio * m + 3.0 * n + noise(), l + noise()
    return tuple(np.round(A * quantum) / quantum for A in (X, Y, Z))


@pytest.mark.parametrize("ratio", [2 ** 10, 2 ** 14, 2 ** 17], ids=["r2^10", "r2^14", "r2^17"])
@pytest.mark.parametrize("p", [2, 3])
def test_thin_skewed_elements_stay_within_the_guard(p, ratio):
    X, Y, Z = thin_block(p, ratio, seed=7 * p + ratio % 1000)
    el = elevation(p)
    B = highorder.jacobian_bezier3d(X, Y, Z, el, 0, 0, 0)
    Xe = r3.element(X, Y, Z, p, 0, 0, 0)
    Br = r3.exact_bezier(Xe, p)
    gd, R3, m = r3.guard(Xe, p)
    six = sum(m[0][a] * m[1][b] * m[2][c] for a, b, c in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)))
    err = worst_error(B, Br)
    print(f"ho3_certify: thin p {p} aspect {ratio}: |B - B_exact| / g {float(err / gd):.3g} (against the six products alone: "
          f"{float(err / (r3.guard_factor(p) * U * six)):.3g}); R3 / six {float(R3 / six):.3g}")
    assert err <= gd
    c, status, bounds = highorder.certify3d(X, Y, Z, el, 3)
    J = r3.Sampler(p, r3_points(p, 4))(Xe)                                             # exact J on a 5^3 dyadic sample
    lo, hi = Fr(float(bounds[0, 0, 0, 0])), Fr(float(bounds[0, 0, 0, 1]))
    assert c.orientation == 1 and all(lo <= v <= hi for v in J.reshape(-1))
    if min(Br.reshape(-1)) > 2 * gd:                                                    # known without the code under test
        assert status[0, 0, 0] == PROVEN and c.decided_at[0] == 1
    else:
        print(f"ho3_certify: thin p {p} aspect {ratio}: min B_exact <= 2 g, no verdict asserted (status {status[0, 0, 0]})")


def r3_points(p, n):
    return [Fr(k * p, n) for k in range(n + 1)]


# ------------------------------------------------------------------ soundness, both ways
@functools.lru_cache(maxsize=None)
def soundness_block(p):
    X, Y, Z = r3.dyadic_block(2 * p + 1, 2 * p + 1, 2 * p + 1, SOUND[p], seed=40 + p)
    by_depth = [highorder.certify3d(X, Y, Z, elevation(p), d) for d in range(4)]
    return (X, Y, Z), by_depth


@pytest.mark.parametrize("p", ORDERS)
def test_soundness_both_ways(p):
    (X, Y, Z), by_depth = soundness_block(p)
    c, status, bounds = by_depth[3]
    assert c.elements == 8 and c.proven >= 1 and c.invalid >= 1 and c.undecided <= 4    # not vacuous: asserted, not assumed
    print(f"ho3_certify: soundness p {p}: proven {c.proven} invalid {c.invalid} undecided {c.undecided} decided at {c.decided_at}")
    _, _, _, q, sj = highorder.planes3d(X, Y, Z, elevation(p), planes=False)
    sampler = r3.Sampler(p, r3_points(p, 8))                                            # holds every patch corner up to depth 3
    o = c.orientation if c.orientation else 1
    for g in range(2):
        for f in range(2):
            for e in range(2):
                if status[g, f, e] == UNDECIDED:
                    continue
                Xe = r3.element(X, Y, Z, p, e, f, g)
                J = sampler(Xe) * o
                if status[g, f, e] == PROVEN:
                    assert all(v > 0 for v in J.reshape(-1)), (e, f, g)
                    lo = Fr(float(bounds[g, f, e, 0]))
                    assert all(v >= lo for v in J.reshape(-1))
                    continue
                if np.isnan(sj[g, f, e]):                                               # an invalid nodal record
                    continue
                level = next(d for d in range(4) if by_depth[d][1][g, f, e] == INVALID)  # breadth first: the first depth that refutes it
                gd, _, _ = r3.guard(Xe, p)
                step = 8 >> level
                corners = J[::step, ::step, ::step]
                assert min(corners.reshape(-1)) <= gd, (e, f, g, level)


# ------------------------------------------------------------------ consistency
def test_all_three_verdicts_occur():
    seen = set()
    for p in ORDERS:
        seen |= set(np.unique(soundness_block(p)[1][3][1]).tolist())
    assert seen == {PROVEN, INVALID, UNDECIDED}


@pytest.mark.parametrize("mapping", ["planar", "cylindrical", "revolution"])
def test_unperturbed_geometry_is_proven_at_depth_zero(mapping):
    for p in ORDERS:
        ni, nj, K, nk = 2 * p + 1, 3 * p + 1, 3, 2 * p + 1
        z = sr.spans(K, "uniform")
        u = np.linspace(-1.0, 3.0, 9)                                                    # cones that widen downstream, one per cut
        sf = stack.Surfaces([u] * K, [u] * K, [zc * (1.0 + 0.05 * u) for zc in z], z) if mapping == "revolution" else None
        st = stack.Stack(z, stack.layers_from(z, nk), "cubic", mapping, surfaces=sf)
        cuts = cut_meshes(smooth_cuts(ni, nj, K, p))
        c, status, bounds = st.certify(cuts, elevation(p), 0, host=True, max_depth=0)
        assert c.elements == 2 * 3 * 2 and c.proven == c.elements and c.decided_at[0] == c.elements and not c.has_unproven, (p, c)
        assert (status == PROVEN).all() and (bounds[..., 0] > 0).all()
        # for proven elements lo / hi is a lower bound of the scaled Jacobian the nodal record samples
        fine = st.block(cuts, 0, host=True)
        _, _, _, q, sj = highorder.planes3d(*fine[:3], elevation(p), planes=False)
        assert np.all(bounds[..., 0] / bounds[..., 1] <= sj)
        assert c.min_scaled_bound == (bounds[..., 0] / bounds[..., 1]).min() <= q.min_scaled_jacobian
        # and the call from the cuts is the call on the planes tm_stack_block[_surf]_host returns, bit for bit
        want = highorder.certify3d(*fine[:3], elevation(p), 0)
        assert same_certificate(c, want[0]) and status.tobytes() == want[1].tobytes() and bounds.tobytes() == want[2].tobytes()


def test_the_call_from_the_cuts_equals_the_call_on_the_planes_on_rough_cuts():
    for p, ni, nj, nk, K, mapping in ((1, 4, 3, 3, 2, "planar"), (2, 7, 5, 5, 3, "cylindrical"), (3, 7, 4, 4, 2, "revolution"), (4, 5, 5, 5, 3, "planar")):
        st = stack_for(K, nk, "cubic" if K == 3 else "linear", mapping, seed=ni)
        cuts = cut_meshes(rough_cuts(ni, nj, K, p))
        got = st.certify(cuts, elevation(p), 0, host=True, max_depth=3)
        want = highorder.certify3d(*st.block(cuts, 0, host=True)[:3], elevation(p), 3)
        assert same_certificate(got[0], want[0]) and got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()
        total, per_block, statuses, bnds = st.certify(cuts, elevation(p), host=True, max_depth=3)
        assert same_certificate(total, got[0]) and len(per_block) == 1 and statuses[0].tobytes() == got[1].tobytes()


# ------------------------------------------------------------------ interface
def test_non_finite_nodes_are_invalid():
    for bad in (np.nan, np.inf):
        X, Y, Z = r3.dyadic_block(5, 5, 5, 0.05, seed=3)
        Y[2, 1, 1] = bad                                                                # a node of element (0, 0, 0) ... and of its neighbours
        c, status, _ = highorder.certify3d(X, Y, Z, elevation(2), 2)
        assert status[0, 0, 0] == INVALID and c.invalid >= 1 and c.proven + c.invalid + c.undecided == 8
        assert c.decided_at[0] >= 1


def test_arguments():
    L = _capi.lib()
    X, Y, Z = r3.dyadic_block(5, 5, 5, 0.05, seed=1)
    ptr = [_capi.f64ptr(A) for A in (X, Y, Z)]
    cert = _capi.tm_ho3_certificate()
    status = np.empty(8, dtype=np.uint8)
    sp = status.ctypes.data_as(C.POINTER(C.c_uint8))
    bounds = np.empty(16)

    def rc(order=2, depth=2, ni=5, nj=5, nk=5, x=ptr[0]):
        opt = _capi.tm_ho_opt(order, _capi.TM_HO_GAUSS_LOBATTO, None)
        return L.tm_ho3_certify_planes_host(x, ptr[1], ptr[2], ni, nj, nk, C.byref(opt), depth, 0, C.byref(cert), sp, _capi.f64ptr(bounds))

    assert rc() == _capi.TM_OK and cert.elements == 8 and cert.proven == 8 and cert.max_depth == 2
    assert rc(order=1, ni=3, nj=3, nk=3) == _capi.TM_OK and rc(order=4) == _capi.TM_OK and cert.elements == 1
    for depth in (0, 3):
        assert rc(depth=depth) == _capi.TM_OK and cert.max_depth == depth
    assert rc(depth=4) == _capi.TM_E_ARG and rc(depth=-1) == _capi.TM_E_ARG
    assert rc(order=5) == _capi.TM_E_ARG and rc(order=0) == _capi.TM_E_ARG
    assert rc(order=3) == _capi.TM_E_SIZE and rc(nk=4) == _capi.TM_E_SIZE and rc(nk=1) == _capi.TM_E_SIZE   # the size rule
    assert rc(x=None) == _capi.TM_E_ARG
    opt = _capi.tm_ho_opt(2, 0, None)
    assert L.tm_ho3_certify_planes_host(*ptr, 5, 5, 5, C.byref(opt), 2, 0, None, None, None) == _capi.TM_OK   # every output may be NULL
    assert L.tm_ho3_certify_planes_host(*ptr, 5, 5, 5, None, 2, 0, C.byref(cert), sp, _capi.f64ptr(bounds)) == _capi.TM_E_ARG
    B = np.empty(216)
    assert L.tm_ho3_jacobian_bezier_host(*ptr, 5, 5, 5, C.byref(opt), 1, 1, 1, _capi.f64ptr(B)) == _capi.TM_OK
    assert L.tm_ho3_jacobian_bezier_host(*ptr, 5, 5, 5, C.byref(opt), 2, 0, 0, _capi.f64ptr(B)) == _capi.TM_E_ARG   # an element past the block
    assert L.tm_ho3_jacobian_bezier_host(*ptr, 5, 5, 5, C.byref(opt), 0, 0, 0, None) == _capi.TM_E_ARG
    assert L.tm_ho3_certify_tables(None, None, None, None, None, None) == _capi.TM_E_ARG
    assert L.tm_ho3_certify_tables(C.byref(opt), None, None, None, None, None) == _capi.TM_OK
    opt5 = _capi.tm_ho_opt(5, 0, None)
    assert L.tm_ho3_certify_tables(C.byref(opt5), None, None, None, None, None) == _capi.TM_E_ARG
    assert C.sizeof(_capi.tm_ho3_certificate) == 160
    # from the cuts: revolution without its tables, tables without revolution, depth
    cuts = cut_meshes(bent_cuts(5, 5, 2))
    z, s = np.array([1.0, 2.0]), np.array([1.0, 1.5, 2.0])
    descs = [_capi.MeshDesc(m) for m in cuts]
    arr = (C.POINTER(_capi.tm_mesh_desc) * 2)(*[C.pointer(d.desc) for d in descs])

    def rc_stack(mapping=0, depth=2, order=2, layers=s, surfaces=None):
        so = _capi.tm_stack_opt(2, _capi.f64ptr(z), layers.size, _capi.f64ptr(layers), 0, mapping)
        ho = _capi.tm_ho_opt(order, 0, None)
        return L.tm_stack_certify_host(arr, C.byref(so), surfaces, C.byref(ho), depth, 0, C.byref(cert), sp, _capi.f64ptr(bounds), None)

    assert rc_stack() == _capi.TM_OK and cert.elements == 4
    assert rc_stack(mapping=_capi.TM_STACK_CYLINDRICAL) == _capi.TM_OK
    assert rc_stack(mapping=_capi.TM_STACK_REVOLUTION) == _capi.TM_E_ARG              # the surfaces are missing
    u, x, r, rr = ssr.tables(2)
    sf = stack.Surfaces(u, x, r, rr)
    assert rc_stack(mapping=_capi.TM_STACK_REVOLUTION, surfaces=sf.ref()) == _capi.TM_OK
    assert rc_stack(surfaces=sf.ref()) == _capi.TM_E_ARG                               # tables without the mapping
    assert rc_stack(depth=4) == _capi.TM_E_ARG and rc_stack(depth=-1) == _capi.TM_E_ARG and rc_stack(order=5) == _capi.TM_E_ARG
    assert rc_stack(order=4) == _capi.TM_E_SIZE and rc_stack(layers=np.array([1.0, 2.0])) == _capi.TM_E_SIZE
    with pytest.raises(_capi.TmError):
        highorder.certify3d(X, Y, Z, elevation(2), 4)
    with pytest.raises(ValueError):
        highorder.certify3d(X, Y[:4], Z, elevation(2), 2)


def test_total_of_block_certificates():
    a = highorder.certify3d(*r3.dyadic_block(5, 5, 5, 0.05, seed=1), elevation(2), 2)[0]
    b = highorder.certify3d(*extruded(2), elevation(2), 2, block=1)[0]
    t = quality.total_ho3_certificate([a, b])
    assert t.elements == 9 and t.proven == 8 and t.invalid == 1 and t.hidden_invalid == 1 and t.undecided == 0
    assert t.decided_at == tuple(x + y for x, y in zip(a.decided_at, b.decided_at)) and t.order == 2 and t.orientation == 1 and t.max_depth == 2
    assert t.min_scaled_bound == a.min_scaled_bound and (t.worst_block, t.worst_e, t.worst_f, t.worst_g) == (0, a.worst_e, a.worst_f, a.worst_g)
    assert t.has_unproven and (t.first_unproven_block, t.first_unproven_e, t.first_unproven_f, t.first_unproven_g) == (1, 0, 0, 0)
    c = highorder.certify3d(*r3.dyadic_block(5, 5, 5, 0.05, seed=1), elevation(2), 1)[0]
    assert quality.total_ho3_certificate([a, c]).max_depth == -1
    empty = quality.total_ho3_certificate([])
    assert empty.elements == 0 and np.isnan(empty.min_scaled_bound) and not empty.has_unproven


def test_log_lines(caplog):
    import logging

    a = highorder.certify3d(*extruded(2), elevation(2), 3)[0]
    with caplog.at_level(logging.INFO, logger="quality"):
        quality.log_report_ho3_certificate(logging.getLogger("quality"), ["block_0"], [a], quality.total_ho3_certificate([a]))
    lines = [r.getMessage() for r in caplog.records]
    assert len(lines) == 2 and lines[0].startswith("certify3d block_0: order 2 depth 3 elements 1 proven 0 invalid 1 undecided 0 hidden invalid 1 decided at 0/0/1/0")
    assert "first unproven (block 0, e 0, f 0, g 0)" in lines[1] and lines[1].startswith("certify3d total:")


# ------------------------------------------------------------------ CLI: what the exit code says (the solve replaced by host cuts)
def test_cli_exit_codes(monkeypatch, tmp_path):
    from types import SimpleNamespace

    from turbomesh_amd import __main__ as cli

    def run_on(cut):
        def _run(ap, args, config, keep=None, tag="", stack=None):
            mesh = cfr.single_block_mesh(cut)
            return SimpleNamespace(output=None), mesh, mesh, {}, None
        monkeypatch.setattr(cli, "_run", _run)

    ho, cert = stack.Stack.mesh3d_ho, stack.Stack.certify
    monkeypatch.setattr(stack.Stack, "mesh3d_ho", lambda self, cuts, el: ho(self, cuts, el, host=True))
    monkeypatch.setattr(stack.Stack, "certify", lambda self, cuts, el, b=None, host=True, max_depth=2: cert(self, cuts, el, b, host=True, max_depth=max_depth))
    out = str(tmp_path / "o.xyz")

    def main(*flags, order="2"):
        try:
            cli.main(["a.json", "--stack", "b.json", "--span", "0,2", "--layers", "3", "--order", order, "--output", out, *flags])
        except SystemExit as e:
            return e.code
        return 0

    run_on(HIDDEN[2])                                                                    # extruded: valid at the nodes, folded between them
    assert main() == 0 and main("--fail-on-invalid-elements") == 0                      # the nodal record alone sees nothing
    assert main("--stack-certify") == 0                                                 # reported, not failed
    msg = main("--stack-certify", "--fail-on-invalid-elements")
    assert isinstance(msg, str) and "1 hexahedra of order 2 are valid at their nodes and folded between them (1 invalid by the certificate)" in msg
    msg = main("--stack-certify", "--fail-on-unproven-elements")
    assert isinstance(msg, str) and "1 of 1 hexahedra of order 2 are not proven valid (1 invalid, 0 undecided at depth 2; first: block 0, e 0, f 0, g 0)" in msg
    assert main("--stack-certify", "1", "--fail-on-invalid-elements") == 0              # depth 1 leaves it undecided: not invalid ...
    msg = main("--stack-certify", "1", "--fail-on-unproven-elements")
    assert isinstance(msg, str) and "(0 invalid, 1 undecided at depth 1; first: block 0, e 0, f 0, g 0)" in msg   # ... but not proven either
    run_on(cfr.bent_clustered(7, 9))
    assert main("--stack-certify", "--fail-on-invalid-elements", "--fail-on-unproven-elements") == 0
    assert main("--stack-certify", "4") == 2 and main("--fail-on-unproven-elements") == 2
    monkeypatch.undo()
    for argv in (["x.json", "--stack-certify"], ["x.json", "--order", "2", "--stack-certify"],
                 ["x.json", "--stack", "y.json", "--span", "0,1", "--layers", "3", "--output", out, "--stack-certify"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2
