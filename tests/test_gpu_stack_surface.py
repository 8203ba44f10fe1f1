"""GPU: the revolution mapping on the device (include/tm_hip.h, "cuts on stream surfaces of revolution"; the surface stage K15 inside
K11 and K12) against the longdouble reference of tests/stack_surface_reference.py and against the host definition, at the smallest shapes
that reach every edge of K11's 32 x 32 tiling and of K12's 15 x 15 cell tiles; the handle path, the CLI and the harness.

Device against host: X and R come from shared arithmetic (tm_stack_surface.hpp) and the same sums, so X is bit for bit, and so is Z where
v == 0 (sin 0 = 0, cos 0 = 1: Z is R itself); Y and Z otherwise differ by the two sine / cosine implementations, within twice the bar."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import control_field_reference as cfr
from tests import stack_reference as sr
from tests import stack_surface_reference as ssr
from tests.conftest import ROOT
from tests.test_o4h import GOLD
from tests.test_quality3d_cpu import same_bits
from tests.test_gpu_stack import T106_SIZES, _t106_cut_files
from tests.test_gpu_stack_quality import SEAM1, SEAM2, volume_bound
from turbomesh_amd import _capi, configs, output, stack
from turbomesh_amd.smoothing import smooth, solver

pytestmark = pytest.mark.gpu
LD = np.longdouble
EPS = sr.EPS
HARNESS = os.path.join(ROOT, "turbomesh_amd", "tm_harness")


def bent_cuts(ni, nj, K):
    return [cfr.bent_clustered(ni, nj, seed=c) + 0.01 * c for c in range(K)]


def cut_meshes(blocks):
    return [cfr.single_block_mesh(b) for b in blocks]


def rev_stack(z, s, u, x, r, rref=None, interpolation="cubic", curve="cubic"):
    return stack.Stack(z, s, interpolation, "revolution", surfaces=stack.Surfaces(u, x, r, rref, curve))


# (ni, nj, K, nk, span interpolation, curve interpolation, span kind): every value of every axis at least once, 16 cuts x 33 layers once; the
# tables of a call mix N from {2, 3, 65, 256} (K = 2 and 3 take the first ones of a rotation that starts at another N per case)
CASES = [
    (3, 3, 2, 1, "linear", "linear", "uniform"),
    (4, 5, 3, 2, "cubic", "cubic", "uniform"),
    (33, 31, 5, 7, "cubic", "linear", "nonuniform"),
    (33, 31, 3, 7, "linear", "cubic", "uniform"),
    (67, 130, 16, 33, "cubic", "cubic", "nonuniform"),
    (130, 67, 5, 7, "cubic", "cubic", "uniform"),
    (130, 67, 2, 33, "linear", "cubic", "nonuniform"),
    (67, 130, 16, 2, "linear", "linear", "uniform"),
]


@functools.lru_cache(maxsize=None)
def case_data(ni, nj, K, nk, interpolation, curve, kind):
    """Inputs, the library's weights and tables and the longdouble reference of a case: computed once, shared, never modified."""
    z = sr.spans(K, kind)
    s = sr.layers_with_cuts(z, nk, seed=ni + K)
    blocks = bent_cuts(ni, nj, K)
    u, x, r, rr = ssr.tables(K, seed=ni + nk)
    st = rev_stack(z, s, u, x, r, rr, interpolation, curve)
    ref, bar, _, _ = ssr.surf_ref(blocks, st.weights(), u, st.surface_tables(), rr)
    for a in (z, s, *blocks, *ref, *bar):
        a.setflags(write=False)
    return z, s, blocks, u, st, ref, bar


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_device_against_reference_and_host(case):
    ni, nj, K, nk, interpolation, curve, kind = case
    z, s, blocks, u, st, ref, bar = case_data(*case)
    cuts = cut_meshes(blocks)
    *dev, outside = st.block(cuts, 0, return_outside=True)
    assert all(d.shape == (nk, nj, ni) for d in dev)
    ratios = [sr.worst_ratio(d, q, b) for d, q, b in zip(dev, ref, bar)]
    print(f"stack_surface_parity: device {'-'.join(str(v) for v in case)}: worst ratio x {ratios[0]:.3f} y {ratios[1]:.3f} z {ratios[2]:.3f}")
    assert max(ratios) <= 1.0
    *host, outside_host = st.block(cuts, 0, host=True, return_outside=True)
    assert np.array_equal(dev[0], host[0])                                 # X bit for bit
    for d, h, b in zip(dev[1:], host[1:], bar[1:]):
        assert np.all(np.abs(d.astype(LD) - h.astype(LD)) <= 2 * b)
    assert np.array_equal(outside, outside_host) and np.array_equal(outside, ssr.outside_ref(blocks, u))
    if nk >= 2:   # windows concatenate to the full call bit for bit, and the count does not depend on the window
        cut = 3 if nk > 3 else 1
        a, b = st.block(cuts, 0, 0, cut, return_outside=True), st.block(cuts, 0, cut, return_outside=True)
        for f, p, q in zip(dev, a, b):
            assert np.array_equal(f, np.concatenate([p, q]))
        assert np.array_equal(a[3], outside) and np.array_equal(b[3], outside)


@pytest.mark.parametrize("ni,nj,K", [(33, 31, 5), (67, 40, 16)])
def test_radius_is_bit_for_bit_and_outside_counts(ni, nj, K):
    # v == 0: Y == 0 and Z is R itself, equal to the host's bit for bit.  Tables over the 5 % .. 95 % quantiles of the first coordinates,
    # half of their knots taken from the nodes: knot hits and extrapolated nodes at both ends
    z = sr.spans(K, "nonuniform")
    s = sr.layers_with_cuts(z, 2 * K - 1, seed=K)
    blocks = bent_cuts(ni, nj, K)
    for b in blocks:
        b[..., 1] = 0.0
    rr = ssr.rrefs(K)
    rng = np.random.default_rng(23)
    u = []
    for b in blocks:
        first = np.unique(b[..., 0])
        lo, hi = np.quantile(first, [0.05, 0.95])
        inside = first[(first > lo) & (first < hi)]
        u.append(np.unique(np.concatenate([[lo, hi], rng.choice(inside, 15, replace=False), rng.uniform(lo, hi, 15)])))
    xr = [ssr.curves(u[c], c, rr[c]) for c in range(K)]
    x, r = [a for a, _ in xr], [a for _, a in xr]
    st = rev_stack(z, s, u, x, r, rr)
    cuts = cut_meshes(blocks)
    X, Y, Z, outside = st.block(cuts, 0, return_outside=True)
    Xh, Yh, Zh, outside_host = st.block(cuts, 0, host=True, return_outside=True)
    assert np.array_equal(X, Xh) and np.array_equal(Z, Zh) and not Y.any() and not Yh.any()
    want = ssr.outside_ref(blocks, u)
    assert np.array_equal(outside, want) and np.array_equal(outside_host, want)
    for c, b in enumerate(blocks):
        un = b[..., 0].T
        assert np.count_nonzero(un < u[c][0]) > 0 and np.count_nonzero(un > u[c][-1]) > 0
        k = int(np.nonzero(s == z[c])[0][0])                               # a layer at the cut
        hit = np.isin(un, u[c][:-1])
        assert hit.any()
        n = ssr.locate(u[c], un[hit])
        assert np.array_equal(X[k][hit], x[c][n]) and np.array_equal(Z[k][hit], r[c][n])   # the knot values bit for bit


def test_cylinder_tables_reproduce_the_cylindrical_mapping():
    K, L = 3, 1.2
    radii = sr.spans(K, "uniform")
    s = sr.layers_with_cuts(radii, 7, seed=2)
    blocks = bent_cuts(33, 31, K)
    u = [np.array([0.0, L])] * K
    st = rev_stack(radii, s, u, u, [np.array([R, R]) for R in radii], None)
    cuts = cut_meshes(blocks)
    X, Y, Z = st.block(cuts, 0)
    Xc, Yc, Zc = stack.Stack(radii, s, "cubic", "cylindrical").block(cuts, 0)
    assert np.array_equal(X, Xc)
    for k, sk in enumerate(s):
        if np.any(radii == sk):
            assert np.array_equal(Y[k], Yc[k]) and np.array_equal(Z[k], Zc[k])


def _handles(ni=33, nj=31, K=3):
    meshes = [configs.single_block(ni, nj, amplitude=0.05 + 0.02 * c) for c in range(K)]
    return meshes, [smooth.Smoother(m, solver.Option.hip(inner=solver.Inner.relax)) for m in meshes]


def _unit_square_tables(K):
    """Tables for configs.single_block cuts (first coordinates within [0, 1] and a little beyond): a hub-to-shroud family of contoured walls."""
    rr = 0.5 + 0.25 * np.arange(K)
    u = [np.linspace(-0.05, 1.05, 9 + 8 * c) for c in range(K)]
    x = [a + 0.03 * (c + 1) * np.sin(3 * a) for c, a in enumerate(u)]
    r = [rr[c] * (1 + 0.2 * np.tanh(2 * (a - 0.5))) for c, a in enumerate(u)]
    return u, x, r, rr


def test_resident_handles_give_the_downloaded_bits_and_stay_untouched():
    z = [0.0, 0.4, 1.0]
    st = rev_stack(z, stack.layers_from(z, 7), *_unit_square_tables(3))
    plain_meshes, plain = _handles()
    watched_meshes, watched = _handles()
    try:
        for h in plain + watched:
            h.iterate(2)
        res = st.block(watched, 0, return_outside=True)       # ordered behind the sweeps, nothing downloaded
        q = st.quality(watched)
        field = st.quality_field(watched, 0)
        stats_plain = [h.iterate(2) for h in plain]
        stats_watched = [h.iterate(2) for h in watched]
        for h in plain + watched:
            h.download()
        for a, b, sa, sb in zip(plain_meshes, watched_meshes, stats_plain, stats_watched):
            assert a.blocks[0].points.data.tobytes() == b.blocks[0].points.data.tobytes()
            for k in sa:
                if k != "seconds":
                    assert np.asarray(sa[k]).tobytes() == np.asarray(sb[k]).tobytes(), k
    finally:
        for h in plain + watched:
            h.close()
    again_meshes, again = _handles()
    try:
        for h in again:
            h.iterate(2)
            h.download()
        up = st.block(again_meshes, 0, return_outside=True)
        assert all(np.array_equal(a, b) for a, b in zip(res, up))
        host = stack.quality_of_planes(*up[:3], field=True)
        assert same_bits(q[0][0], host[0], skip=("total_volume",)) and abs(q[0][0].total_volume - host[0].total_volume) <= volume_bound(*up[:3])
        assert field.tobytes() == host[1].tobytes()
        assert same_bits(st.quality(again_meshes)[0][0], q[0][0])
    finally:
        for h in again:
            h.close()


def _smoothers_rc(handles, z, s, tables, block=0, mapping=2, fn="tm_stack_smoothers_surf", k_count=None):
    z, s = np.asarray(z, dtype=np.float64), np.asarray(s, dtype=np.float64)
    opt = _capi.tm_stack_opt(z.size, _capi.f64ptr(z), s.size, _capi.f64ptr(s), 1, mapping)
    sf = stack.Surfaces(*tables)
    arr = (C.c_void_p * len(handles))(*handles)
    L = _capi.lib()
    if fn == "tm_stack_smoothers_quality_surf":
        return L.tm_stack_smoothers_quality_surf(arr, C.byref(opt), sf.ref(), block, C.byref(_capi.tm_quality3d()))
    if fn == "tm_stack_smoothers_quality_field_surf":
        return L.tm_stack_smoothers_quality_field_surf(arr, C.byref(opt), sf.ref(), block, 0, s.size - 1 if k_count is None else k_count, _capi.f64ptr(np.empty(s.size * 40 * 40)))
    out = [np.empty(s.size * 40 * 40) for _ in range(3)]
    return L.tm_stack_smoothers_surf(arr, C.byref(opt), sf.ref(), block, 0, s.size if k_count is None else k_count, *[_capi.f64ptr(o) for o in out], None)


def test_error_codes_of_the_handle_path():
    z, s = [1.0, 2.0], [1.0, 1.5]
    tables = _unit_square_tables(2)
    relax = solver.Option.hip(inner=solver.Inner.relax)
    a = smooth.Smoother(cfr.single_block_mesh(cfr.bent_clustered(9, 8)), relax)
    b = smooth.Smoother(cfr.single_block_mesh(cfr.bent_clustered(9, 8, seed=1)), relax)
    other = smooth.Smoother(cfr.single_block_mesh(cfr.bent_clustered(9, 7)), relax)
    strip = smooth.Smoother(configs.strip(2, 9, 8), relax)
    dead = smooth.Smoother(cfr.single_block_mesh(cfr.bent_clustered(9, 8)), relax)
    dead_handle = dead._h.value
    dead.close()
    try:
        for fn in ("tm_stack_smoothers_surf", "tm_stack_smoothers_quality_surf", "tm_stack_smoothers_quality_field_surf"):
            rc = functools.partial(_smoothers_rc, fn=fn)
            assert rc([a._h, b._h], z, s, tables) == _capi.TM_OK
            assert rc([a._h, other._h], z, s, tables) == _capi.TM_E_SIZE
            assert rc([a._h, strip._h], z, s, tables) == _capi.TM_E_SIZE
            assert rc([a._h, b._h], z, s, tables, block=1) == _capi.TM_E_ARG
            assert rc([a._h, None], z, s, tables) == _capi.TM_E_ARG
            assert rc([a._h, dead_handle], z, s, tables) == _capi.TM_E_ARG
            assert rc([a._h, b._h], z, [1.0, 2.5], tables) == _capi.TM_E_ARG
            assert rc([a._h, b._h], z, s, tables, mapping=1) == _capi.TM_E_ARG       # another mapping on the new entry points
            assert rc([a._h, b._h], z, s, tables, mapping=0) == _capi.TM_E_ARG
            assert rc([a._h, b._h], z, s, tables, k_count=0) in ((_capi.TM_E_ARG,) if fn != "tm_stack_smoothers_quality_surf" else (_capi.TM_OK,))
            bad = (tables[0], tables[1], [tables[2][0], -tables[2][1]], tables[3])
            assert rc([a._h, b._h], z, s, bad) == _capi.TM_E_ARG                     # r <= 0
        assert _smoothers_rc([a._h, b._h], z, [1.5], tables, fn="tm_stack_smoothers_quality_surf") == _capi.TM_E_SIZE   # one layer: no cells
        # mapping 2 on the entry points that have no tables
        zz, ss = np.array(z), np.array(s)
        opt = _capi.tm_stack_opt(2, _capi.f64ptr(zz), 2, _capi.f64ptr(ss), 1, 2)
        arr = (C.c_void_p * 2)(a._h, b._h)
        out = [np.empty(2 * 72) for _ in range(3)]
        assert _capi.lib().tm_stack_smoothers(arr, C.byref(opt), 0, 0, 2, *[_capi.f64ptr(o) for o in out]) == _capi.TM_E_ARG
        assert _capi.lib().tm_stack_smoothers_quality(arr, C.byref(opt), 0, C.byref(_capi.tm_quality3d())) == _capi.TM_E_ARG
        with pytest.raises(ValueError):
            stack.Stack(z, s, mapping="revolution", surfaces=stack.Surfaces(*tables)).block([a, b], 0, host=True)
    finally:
        for h in (a, b, other, strip):
            h.close()


# ------------------------------------------------------------------ the quality kernel
# (ni, nj, K, nk, span interpolation, curve): one cell; ni and nj one below, at and above both tile seams; K = 2, 3, 8, 16; nk = 2, 3, 9
QCASES = [
    (2, 2, 2, 2, "linear", "linear"),
    (SEAM1 - 1, SEAM1 + 1, 3, 3, "cubic", "cubic"),
    (SEAM1, SEAM1, 8, 2, "cubic", "cubic"),
    (SEAM1 + 1, SEAM1 - 1, 2, 9, "linear", "cubic"),
    (SEAM2 - 1, SEAM2 + 1, 16, 3, "cubic", "linear"),
    (SEAM2, SEAM2, 3, 9, "cubic", "cubic"),
    (SEAM2 + 1, SEAM2 - 1, 8, 3, "linear", "cubic"),
    (70, 35, 16, 9, "cubic", "cubic"),
]


def assert_quality_equals_host(st, blocks):
    cuts = cut_meshes(blocks)
    planes = st.block(cuts, 0)                                 # K11 + K15 on the device
    host, host_field = stack.quality_of_planes(*planes, field=True)
    dev = st.quality(cuts)[0][0]                               # K12 + K15 straight from the cuts
    assert same_bits(dev, host, skip=("total_volume",)), (dev, host)
    assert abs(dev.total_volume - host.total_volume) <= volume_bound(*planes)
    return dev, host_field


@pytest.mark.parametrize("case", QCASES, ids=lambda c: "-".join(str(v) for v in c))
def test_quality_device_equals_host_bit_for_bit(case):
    ni, nj, K, nk, interpolation, curve = case
    z = sr.spans(K, "uniform")
    s = np.sort(sr.layers_with_cuts(z, nk, seed=ni + K))
    u, x, r, rr = ssr.tables(K, seed=nj)
    st = rev_stack(z, s, u, x, r, rr, interpolation, curve)
    blocks = bent_cuts(ni, nj, K)
    dev, host_field = assert_quality_equals_host(st, blocks)
    assert dev.cells == (ni - 1) * (nj - 1) * (nk - 1) and sum(dev.hist) == dev.cells - dev.inverted - dev.degenerate
    if min(ni, nj) < 3:
        return                                                 # a handle takes blocks of 3 x 3 nodes and more
    handles = [smooth.Smoother(m, solver.Option.hip(inner=solver.Inner.relax)) for m in cut_meshes(blocks)]
    try:
        assert same_bits(st.quality(handles)[0][0], dev)
        assert st.quality_field(handles, 0).tobytes() == host_field.tobytes()      # create uploads the coordinates as they are
    finally:
        for h in handles:
            h.close()


def test_crossing_hub_and_shroud_give_inverted_cells():
    # r_1(u) < r_0(u) beyond u = 0.7: the shroud curve dips below the hub curve, the cells there are inside out
    ni, nj = 20, 18
    blocks = bent_cuts(ni, nj, 2)
    u = [np.linspace(-0.6, 2.0, 27)] * 2
    r = [np.full(27, 1.0), 1.3 - (3.0 / 7.0) * u[0]]
    assert r[1][0] > r[0][0] and r[1][-1] < r[0][-1]
    st = rev_stack([1.0, 2.0], np.linspace(1.0, 2.0, 4), u, [u[0], u[0]], r, [1.0, 1.0], curve="linear")
    dev, _ = assert_quality_equals_host(st, blocks)
    host = st.quality(cut_meshes(blocks), host=True)[0][0]
    assert dev.inverted > 0 and (dev.inverted, dev.degenerate, dev.cells, dev.orientation) == (host.inverted, host.degenerate, host.cells, host.orientation)


# ------------------------------------------------------------------ CLI, harness
def _write_table(path, u, x, r):
    with open(path, "w") as f:
        f.write("# u x r\n")
        for row in zip(u, x, r):
            f.write(" ".join(repr(float(v)) for v in row) + "\n")


def test_cli_places_three_t106_cuts_on_their_surfaces(tmp_path):
    files = _t106_cut_files(tmp_path)
    radii = [0.3, 0.35, 0.4]
    env = dict(os.environ, PYTHONPATH=ROOT)
    base = [sys.executable, "-m", "turbomesh_amd", files[0], "--hip", "--iterations", "1", "--stack", files[1], files[2], "--span", ",".join(map(str, radii)),
            "--layers", "5"]
    # cone to cylinder: the radius falls linearly up to u = ub (mid-chord; the mesh spans about [1.0, 1.15]) and stays; x = u
    ub = 1.09
    u = np.concatenate([np.linspace(0.95, ub, 6), np.linspace(1.12, 1.2, 4)])
    tabs, cyl = [], []
    for c, R in enumerate(radii):
        r = np.where(u < ub, R + 0.4 * (c + 1) * (ub - u), R)
        tabs.append(str(tmp_path / f"m{c}.txt"))
        _write_table(tabs[-1], u, u, r)
        cyl.append(str(tmp_path / f"c{c}.txt"))
        _write_table(cyl[-1], [0.0, 10.0], [0.0, 10.0], [R, R])     # x = 0 + t (1 + ...), t = u - 0: u itself, also where it is continued below 0
    out = str(tmp_path / "rev.xyz")
    run = subprocess.run(base + ["--output", out, "--stack-mapping", "revolution", "--meridional", *tabs, "--meridional-interpolation", "linear", "--stack-quality"],
                         capture_output=True, text=True, timeout=600, cwd=GOLD, env=env)
    assert run.returncode == 0, run.stderr[-3000:]
    assert "3 cuts, 5 layers" in run.stderr
    back = output.read_plot3d_3d(out)
    assert [(b[0], b[1], b[2]) for b in back] == [(ni, nj, 5) for ni, nj in T106_SIZES]
    assert all(np.isfinite(b[k]).all() for b in back for k in (3, 4, 5))
    warned = [line for line in run.stderr.splitlines() if "WARNING(stack)" in line]
    # layer 0 is cut 0 on its surface: hypot(Y, Z) is r_0(X) (x = u on this table), within bar_R + |r'| bar_X + 2 eps |R|, r' = -0.4;
    # with one cut in the sum (the unit row) bar_X = eps (K+1 + 8) |x| and bar_R likewise; P_c <= |a| + |t| |b| <= 2 |r|
    inside = 0
    for ni, nj, nk, X, Y, Z in back:
        x0 = X[0].astype(LD)
        R0 = np.where(x0 < ub, radii[0] + 0.4 * (ub - x0), radii[0])
        ok = (x0 >= u[0]) & (x0 <= u[-1])
        inside += int(np.count_nonzero(ok))
        bar = EPS * (4 + 16) * np.abs(R0) + 0.4 * EPS * (4 + 16) * np.abs(x0) + 2 * EPS * np.abs(R0)
        assert np.all(np.abs(np.hypot(Y[0].astype(LD), Z[0].astype(LD)) - R0)[ok] <= bar[ok])
    assert inside > 0
    if any(np.any((b[3][0] < u[0] - 1e-9) | (b[3][0] > u[-1] + 1e-9)) for b in back):
        assert warned                                                     # one warning per cut and block with extrapolated nodes
    # cylinder tables reproduce the cylindrical run's X planes
    out_c, out_r = str(tmp_path / "cyl.xyz"), str(tmp_path / "revcyl.xyz")
    a = subprocess.run(base + ["--output", out_c, "--stack-mapping", "cylindrical"], capture_output=True, text=True, timeout=600, cwd=GOLD, env=env)
    b = subprocess.run(base + ["--output", out_r, "--stack-mapping", "revolution", "--meridional", *cyl], capture_output=True, text=True, timeout=600, cwd=GOLD, env=env)
    assert a.returncode == 0 and b.returncode == 0, a.stderr[-2000:] + b.stderr[-2000:]
    for p, q in zip(output.read_plot3d_3d(out_c), output.read_plot3d_3d(out_r)):
        assert np.array_equal(p[3], q[3])
        for k in (0, 4):   # layers at cuts: all three coordinates
            assert np.array_equal(p[4][k], q[4][k]) and np.array_equal(p[5][k], q[5][k])


def test_harness_places_layers_on_their_surfaces():
    r = subprocess.run([HARNESS, "stack-revolution", "33", "25", "3", "7"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "stack-revolution: layers at cuts lie on their surfaces: yes" in r.stdout
    assert len([l for l in r.stdout.splitlines() if l.startswith("stack-revolution: layer ")]) == 7
