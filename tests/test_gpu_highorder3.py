"""GPU: high-order hexahedra of stacked blocks on the device (include/tm_hip.h, "high-order hexahedra of stacked blocks"; kernel K16)
against the host definition, at the smallest shapes that reach every edge of K16's tiling; the handle path, the CLI and the harness.

The statement needs no tolerance: K16's planes, sj and every field of the record equal tm_ho3_planes_host applied to the planes
tm_stack_block[_surf] (K11) returned for the same inputs, bit for bit -- the fine nodes are K11's expression, every line of the three
contraction stages is the function the host loops over (tm_highorder3.hpp)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import control_field_reference as cfr
from tests import stack_reference as sr
from tests import stack_surface_reference as ssr
from tests.conftest import ROOT
from tests.test_gpu_stack import T106_SIZES
from tests.test_o4h import GOLD
from tests.test_gpu_stack_quality import _t106_cuts
from tests.test_highorder3_cpu import bent_cuts, cut_meshes, elevation, folded_stack, same_record
from turbomesh_amd import _capi, configs, highorder, output, stack
from turbomesh_amd.smoothing import smooth, solver

pytestmark = pytest.mark.gpu
HARNESS = os.path.join(ROOT, "turbomesh_amd", "tm_harness")

# tm_highorder3_dev.hpp: a workgroup owns ho3_tile_ei(p) x ho3_tile_ej(p) whole elements in-plane, i.e. TILE_I[p] x TILE_J[p] cells, one
# thread per node of the tile ((cells + 1)^2 <= HO3_THREADS = 256); tiles step by those cells, so a seam lies at n = m * cells + 1 nodes.
# There is no blocking in span: a workgroup marches over all span elements.
TILE_EI = {1: 16, 2: 8, 3: 5, 4: 4}
TILE_EJ = {1: 14, 2: 7, 3: 5, 4: 3}
TILE_I = {p: TILE_EI[p] * p for p in TILE_EI}
TILE_J = {p: TILE_EJ[p] * p for p in TILE_EJ}


def shapes(p):
    """(ni, nj, K, Eg, interpolation, mapping, distribution): a single element; ni and nj one element below, at and one above the first
    and the second tile seam; Eg = 1, 2, 3; K = 2, 3, 8, 16; both interpolations, the three mappings and the three distributions."""
    ci, cj = TILE_I[p], TILE_J[p]
    return [
        (p + 1, p + 1, 2, 1, "linear", "planar", "equidistant"),
        (ci - p + 1, cj + p + 1, 3, 2, "cubic", "cylindrical", "gauss_lobatto"),
        (ci + 1, cj + 1, 8, 3, "cubic", "planar", "prescribed"),
        (ci + p + 1, cj - p + 1, 16, 1, "linear", "revolution", "gauss_lobatto"),
        (2 * ci - p + 1, 2 * cj + 1, 3, 2, "cubic", "revolution", "equidistant"),
        (2 * ci + 1, 2 * cj + p + 1, 2, 2, "linear", "cylindrical", "prescribed"),
        (2 * ci + p + 1, 2 * cj - p + 1, 8, 3, "cubic", "planar", "gauss_lobatto"),
    ]


CASES = [(p,) + s for p in (1, 2, 3, 4) for s in shapes(p)]
# The records of more than 256 workgroups meet in two stages (records_first_stage, tm_records.hpp).  At p = 4 a workgroup owns 4 x 3
# elements: 245 x 193 nodes are 61 x 48 elements = 16 x 16 = 256 workgroups, the last block with one stage; 245 x 197 nodes are 61 x 49
# elements = 16 x 17 = 272 workgroups, the smallest block above it.  One span element, two cuts: the host takes 0.1 s.
CASES += [(4, 245, 193, 2, 1, "linear", "planar", "gauss_lobatto"), (4, 245, 197, 2, 1, "linear", "planar", "gauss_lobatto")]


def stack_for(K, nk, interpolation, mapping, seed):
    z = sr.spans(K, "uniform" if mapping != "planar" else "nonuniform")
    s = np.sort(sr.layers_with_cuts(z, nk, seed=seed))
    if mapping == "revolution":
        u, x, r, rr = ssr.tables(K, seed=seed)
        return stack.Stack(z, s, interpolation, mapping, surfaces=stack.Surfaces(u, x, r, rr))
    return stack.Stack(z, s, interpolation, mapping)


def assert_equal(got, want):
    assert all(a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(got[:3], want[:3]))
    assert same_record(got[3], want[3]), (got[3], want[3])
    assert got[4].shape == want[4].shape and got[4].tobytes() == want[4].tobytes()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_device_equals_host_on_what_k11_writes(case):
    p, ni, nj, K, Eg, interpolation, mapping, dist = case
    st = stack_for(K, Eg * p + 1, interpolation, mapping, seed=ni + K)
    cuts = cut_meshes(bent_cuts(ni, nj, K))
    el = elevation(p, dist)
    rev = mapping == "revolution"
    fine = st.block(cuts, 0, return_outside=rev)                             # K11 on the device
    want = highorder.planes3d(*fine[:3], el)                                 # the CPU on what K11 wrote
    got = st.elevate(cuts, el, 0, return_outside=rev)                        # K16 straight from the cuts
    assert_equal(got, want)
    q = got[3]
    assert q.elements == ((ni - 1) // p) * ((nj - 1) // p) * Eg and q.order == p and sum(q.hist) == q.elements - q.invalid
    if dist == "equidistant" or p == 1:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], fine[:3]))   # copied: K11's planes themselves
    if rev:
        assert np.array_equal(got[5], fine[3])
    if Eg >= 2:   # windows with g_begin > 0 tile the block; the record and sj cover the block whatever the window
        for g in range(Eg):
            part = st.elevate(cuts, el, 0, g, 1)
            assert all(part[k].tobytes() == want[k][g * p:(g + 1) * p + 1].tobytes() for k in range(3))
            assert same_record(part[3], want[3]) and part[4].tobytes() == want[4].tobytes()


def test_a_report_alone_equals_the_record_of_the_full_call():
    p, ni, nj, K = 3, TILE_I[3] + 4, TILE_J[3] + 7, 3
    st = stack_for(K, 2 * p + 1, "cubic", "cylindrical", seed=5)
    cuts = cut_meshes(bent_cuts(ni, nj, K))
    el = elevation(p, "gauss_lobatto")
    full = st.elevate(cuts, el, 0)
    rep = st.elevate(cuts, el, 0, planes=False)
    assert rep[0] is None and rep[1] is None and rep[2] is None
    assert same_record(rep[3], full[3]) and rep[4].tobytes() == full[4].tobytes()
    # and with neither record nor sj only the window is evaluated: the planes are the same
    L = _capi.lib()
    descs = [_capi.MeshDesc(m) for m in cuts]
    arr = (C.POINTER(_capi.tm_mesh_desc) * K)(*[C.pointer(d.desc) for d in descs])
    out = [np.empty((p + 1, nj, ni)) for _ in range(3)]
    rc = L.tm_stack_elevate(arr, C.byref(st._opt), None, C.byref(el._opt), 0, 1, 1, *[_capi.f64ptr(o) for o in out], None, None, None)
    assert rc == _capi.TM_OK and all(o.tobytes() == f[p:].tobytes() for o, f in zip(out, full[:3]))


def _handles(ni=33, nj=31, K=3):
    meshes = [configs.single_block(ni, nj, amplitude=0.05 + 0.02 * c) for c in range(K)]
    return meshes, [smooth.Smoother(m, solver.Option.hip(inner=solver.Inner.relax)) for m in meshes]


def test_resident_handles_are_elevated_and_stay_untouched():
    z = [0.0, 0.4, 1.0]
    st = stack.Stack(z, stack.layers_from(z, 7))
    el = elevation(2, "gauss_lobatto")
    plain_meshes, plain = _handles()
    watched_meshes, watched = _handles()
    try:
        for h in plain + watched:
            h.iterate(2)
        res = st.elevate(watched, el, 0)              # ordered behind the sweeps, nothing downloaded
        stats_plain = [h.iterate(2) for h in plain]
        stats_watched = [h.iterate(2) for h in watched]
        for h in plain + watched:
            h.download()
        for a, b, sa, sb in zip(plain_meshes, watched_meshes, stats_plain, stats_watched):
            assert a.blocks[0].points.data.tobytes() == b.blocks[0].points.data.tobytes()
            for k in sa:
                if k != "seconds":   # wall time of the call
                    assert np.asarray(sa[k]).tobytes() == np.asarray(sb[k]).tobytes(), k
    finally:
        for h in plain + watched:
            h.close()
    # the same elements from the coordinates the handles held at the time of the call
    again_meshes, again = _handles()
    try:
        for h in again:
            h.iterate(2)
            h.download()
        assert_equal(res, st.elevate(again_meshes, el, 0))
        assert_equal(st.elevate(again, el, 0), res)
        assert_equal(res, highorder.planes3d(*st.block(again, 0), el))
    finally:
        for h in again:
            h.close()


def _elevate_rc(handles, z, s, order=2, block=0, g_begin=0, g_count=1, mapping=0, shape=(9, 8)):
    z, s = np.asarray(z, dtype=np.float64), np.asarray(s, dtype=np.float64)
    opt = _capi.tm_stack_opt(z.size, _capi.f64ptr(z), s.size, _capi.f64ptr(s), 1, mapping)
    ho = _capi.tm_ho_opt(order, _capi.TM_HO_GAUSS_LOBATTO, None)
    out = [np.empty((g_count * max(order, 1) + 1) * shape[0] * shape[1]) for _ in range(3)]
    q = _capi.tm_ho3_quality()
    return _capi.lib().tm_stack_smoothers_elevate((C.c_void_p * len(handles))(*handles), C.byref(opt), None, C.byref(ho), block, g_begin, g_count,
                                                  *[_capi.f64ptr(o) for o in out], C.byref(q), None, None)


def test_error_codes_of_the_handle_path():
    from turbomesh_amd.distributed import HooksBase

    class NullHooks(HooksBase):   # a transport that moves nothing: the handle is only created and read, never iterated
        def exchange(self, send, recv):
            pass

        def exchange_wait(self):
            pass

        def allreduce(self, t):
            pass

    relax = lambda: solver.Option.hip(inner=solver.Inner.relax)   # noqa: E731
    z, s = [1.0, 2.0], [1.0, 1.25, 1.5, 1.75, 2.0]
    a = smooth.Smoother(cfr.single_block_mesh(cfr.bent_clustered(9, 7)), relax())
    b = smooth.Smoother(cfr.single_block_mesh(cfr.bent_clustered(9, 7, seed=1)), relax())
    odd = [smooth.Smoother(cfr.single_block_mesh(cfr.bent_clustered(9, 8, seed=c)), relax()) for c in range(2)]
    whole = smooth.Smoother(configs.strip(2, 9, 7), relax())
    part = NullHooks(configs.strip(2, 9, 7), [0, 1], 0, 2, option=relax())
    dead = smooth.Smoother(cfr.single_block_mesh(cfr.bent_clustered(9, 7)), relax())
    dead_handle = dead._h.value
    dead.close()
    try:
        ok = [a._h, b._h]
        assert _elevate_rc(ok, z, s) == _capi.TM_OK and _elevate_rc(ok, z, s, g_begin=1) == _capi.TM_OK and _elevate_rc(ok, z, s, g_count=2) == _capi.TM_OK
        assert _elevate_rc(ok, z, s, order=1, g_count=4) == _capi.TM_OK
        assert _elevate_rc([a._h, dead_handle], z, s) == _capi.TM_E_ARG           # a dead handle
        assert _elevate_rc([a._h, None], z, s) == _capi.TM_E_ARG
        assert _elevate_rc([whole._h, part.smoother._h], z, s, block=0) == _capi.TM_OK
        assert _elevate_rc([whole._h, part.smoother._h], z, s, block=1) == _capi.TM_E_ARG   # a handle that does not own the block
        assert _elevate_rc([h._h for h in odd], z, s) == _capi.TM_E_SIZE         # 7 cells along j at order 2
        assert _elevate_rc(ok, z, s[:4]) == _capi.TM_E_SIZE                      # 3 layer cells at order 2
        assert _elevate_rc(ok, z, s, order=4) == _capi.TM_E_SIZE                 # 6 cells along j at order 4
        assert _elevate_rc(ok, z, s, order=5) == _capi.TM_E_ARG                  # an order hexahedra do not take
        assert _elevate_rc(ok, z, s, g_begin=1, g_count=2) == _capi.TM_E_ARG     # a window past Eg
        assert _elevate_rc(ok, z, s, g_begin=3, g_count=1) == _capi.TM_E_ARG
        assert _elevate_rc(ok, z, s, g_count=0) == _capi.TM_E_ARG                # planes with an empty window
        assert _elevate_rc(ok, z, s, mapping=_capi.TM_STACK_REVOLUTION) == _capi.TM_E_ARG   # revolution without surfaces
        with pytest.raises(ValueError):
            stack.Stack(z, s).elevate([a, b], elevation(2, "gauss_lobatto"), 0, host=True)
    finally:
        for h in (a, b, *odd, whole, part.smoother):
            h.close()


def test_a_fold_in_span_on_the_device():
    ni, nj = 2 * TILE_I[2] + 1, TILE_J[2] + 3
    cuts = cut_meshes(bent_cuts(ni, nj, 2))
    st = folded_stack()
    for dist in ("equidistant", "gauss_lobatto"):
        got = st.elevate(cuts, elevation(2, dist), 0)
        assert_equal(got, highorder.planes3d(*st.block(cuts, 0), elevation(2, dist)))
        q, sj = got[3], got[4]
        Ei, Ej = (ni - 1) // 2, (nj - 1) // 2
        assert q.elements == 2 * Ei * Ej and q.invalid == Ei * Ej and q.orientation == 1 and q.worst_g == 1
        assert np.isnan(sj[0]).all() and np.isfinite(sj[1]).all()


def test_cli_elevates_three_stacked_t106_cuts(tmp_path):
    files = _t106_cuts(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT)
    base = [sys.executable, "-m", "turbomesh_amd", files[0], "--hip", "--iterations", "1", "--stack", files[1], files[2], "--span", "0,0.05,0.1", "--layers", "5", "--order", "2"]
    vtk, xyz = str(tmp_path / "blade.vtk"), str(tmp_path / "blade.xyz")
    elements = sum((ni - 1) * (nj - 1) for ni, nj in T106_SIZES) // 4 * 2
    r = subprocess.run(base + ["--output", vtk], capture_output=True, text=True, timeout=600, cwd=GOLD, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stderr.splitlines() if l.startswith("INFO(quality): elevate3d ")]
    assert len(lines) == 9 and lines[-1].startswith(f"INFO(quality): elevate3d total: order 2 elements {elements} invalid "), r.stderr[-3000:]
    points, cells, types = output.read_vtk_lagrange(vtk)
    assert cells.shape == (elements, 27) and np.all(types == 72) and points.shape == (sum(ni * nj for ni, nj in T106_SIZES) * 5, 3)
    assert np.array_equal(np.unique(points[:, 2]), stack.layers_from([0.0, 0.05, 0.1], 5))
    r = subprocess.run(base + ["--output", xyz, "--nodes", "gauss-lobatto", "--fail-on-invalid-elements"], capture_output=True, text=True, timeout=600,
                       cwd=GOLD, env=env)
    total = [l for l in r.stderr.splitlines() if l.startswith("INFO(quality): elevate3d total: ")][0].split()
    invalid = int(total[total.index("invalid") + 1])
    assert (r.returncode != 0) == (invalid > 0), r.stderr[-3000:]                # the exit status follows the record
    back = output.read_plot3d_3d(xyz)
    assert [b[:3] for b in back] == [(ni, nj, 5) for ni, nj in T106_SIZES]
    first = points[:T106_SIZES[0][0] * T106_SIZES[0][1] * 5]
    assert np.array_equal(back[0][3].reshape(-1), first[:, 0]) and np.array_equal(back[0][5].reshape(-1), first[:, 2])   # order 2: Gauss-Lobatto is equidistant
    # refused before anything is smoothed: layers off the element grid, a certificate, an order hexahedra do not take
    bad = subprocess.run(base[:-4] + ["--layers", "4", "--order", "2", "--output", xyz], capture_output=True, text=True, timeout=600, cwd=GOLD, env=env)
    assert bad.returncode != 0 and "4 layers" in bad.stderr and "iteration:" not in bad.stderr
    bad = subprocess.run(base + ["--output", xyz, "--certify"], capture_output=True, text=True, timeout=600, cwd=GOLD, env=env)
    assert bad.returncode == 2 and "3-D certificate is not built" in bad.stderr
    bad = subprocess.run(base[:-1] + ["5", "--output", xyz], capture_output=True, text=True, timeout=600, cwd=GOLD, env=env)
    assert bad.returncode == 2 and "1 .. 4" in bad.stderr


def test_harness_elevates_stacked_cuts():
    r = subprocess.run([HARNESS, "stack-elevate", "33", "25", "3", "7", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"^stack-elevate: hexahedra 576 invalid 0 min sj ", r.stdout, flags=re.M), r.stdout
    assert "stack-elevate: corners unchanged: yes" in r.stdout and "stack-elevate: device equals host: yes" in r.stdout
