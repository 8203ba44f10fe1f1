"""GPU: spanwise stacking on the device (kernel K11: tm_stack_block, tm_stack_smoothers) against the longdouble reference of
tests/stack_reference.py, at the smallest shapes that reach every edge of the 32 x 32 tiling; the Python layer, the CLI and the harness.

Measured on the MI355X (profiles/stack_parity.txt): worst |device - reference| / bar over all cases 0.32 (planar and x), 0.11
(cylindrical y, z); sin / cos alone 0.75 ulp of the result, where the bar allows 4."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import control_field_reference as cfr
from tests import stack_reference as sr
from tests.conftest import ROOT
from tests.test_o4h import GOLD
from turbomesh_amd import _capi, configs, output, stack
from turbomesh_amd.smoothing import smooth, solver

pytestmark = pytest.mark.gpu
LD = np.longdouble
HARNESS = os.path.join(ROOT, "turbomesh_amd", "tm_harness")


def bent_cuts(ni, nj, K):
    return [cfr.bent_clustered(ni, nj, seed=c) + 0.01 * c for c in range(K)]


def cut_meshes(blocks):
    return [cfr.single_block_mesh(b) for b in blocks]


# (ni, nj, K, nk, interpolation, mapping, span kind): every value of every axis at least once; 16 cuts x 33 layers once, on 67 x 130.
# Cylindrical cases take the radii 1 + 0.25 c (the uniform span).
CASES = [
    (3, 3, 2, 1, "linear", "planar", "uniform"),
    (4, 5, 3, 2, "cubic", "cylindrical", "uniform"),
    (33, 31, 5, 7, "cubic", "planar", "nonuniform"),          # one full tile plus a ragged one
    (33, 31, 3, 7, "linear", "cylindrical", "uniform"),
    (67, 130, 16, 33, "cubic", "planar", "nonuniform"),       # tile and wave straddles in both directions
    (130, 67, 5, 7, "cubic", "cylindrical", "uniform"),
    (130, 67, 2, 33, "linear", "planar", "nonuniform"),
    (67, 130, 16, 2, "linear", "cylindrical", "uniform"),
]


@functools.lru_cache(maxsize=None)
def case_data(ni, nj, K, nk, interpolation, mapping, kind):
    """Inputs, the library's weights and the longdouble reference of a case: computed once, shared, never modified."""
    z = sr.spans(K, kind)
    s = sr.layers_with_cuts(z, nk, seed=ni + K)
    blocks = bent_cuts(ni, nj, K)
    st = stack.Stack(z, s, interpolation, mapping)
    A = st.weights()
    ref = sr.stack_ref(blocks, A, mapping, z, s)
    bar = sr.stack_bar(blocks, A, mapping, z, s)
    for a in (z, s, A, *blocks, *ref, *bar):
        a.setflags(write=False)
    return z, s, blocks, st, ref, bar


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_device_against_reference(case):
    ni, nj, K, nk, interpolation, mapping, kind = case
    z, s, blocks, st, ref, bar = case_data(*case)
    cuts = cut_meshes(blocks)
    dev = st.block(cuts, 0)
    assert all(d.shape == (nk, nj, ni) for d in dev)
    ratios = [sr.worst_ratio(d, r, b) if np.any(b > 0) else float(np.max(np.abs(d.astype(LD) - r))) for d, r, b in zip(dev, ref, bar)]
    print(f"stack_parity: device {'-'.join(str(v) for v in case)}: worst ratio x {ratios[0]:.3f} y {ratios[1]:.3f} z {ratios[2]:.3f}")
    assert max(ratios) <= 1.0
    if mapping == "planar":
        assert np.array_equal(dev[2], np.broadcast_to(s[:, None, None], dev[2].shape))   # Z is s_k itself
    at_cuts = 0
    for k, sk in enumerate(s):   # layers at cuts equal the cut
        hit = np.nonzero(z == sk)[0]
        if hit.size:
            at_cuts += 1
            assert np.array_equal(dev[0][k], blocks[hit[0]][..., 0].T)
            if mapping == "planar":
                assert np.array_equal(dev[1][k], blocks[hit[0]][..., 1].T)
    assert at_cuts >= (2 if nk >= 3 else nk - 1)   # tests/stack_reference.py layers_with_cuts: one layer is no cut, two are the first cut and a position between
    # windows concatenate to the full call bit for bit
    if nk >= 2:
        cut = 3 if nk > 3 else 1
        a, b = st.block(cuts, 0, 0, cut), st.block(cuts, 0, cut)
        for f, p, q in zip(dev, a, b):
            assert np.array_equal(f, np.concatenate([p, q]))
    # the host evaluation: within twice the bar of the device (planar: the same sums in the same order)
    host = st.block(cuts, 0, host=True)
    for d, h, b in zip(dev, host, bar):
        assert np.all(np.abs(d.astype(LD) - h.astype(LD)) <= 2 * b)
    if mapping == "planar":
        assert all(np.array_equal(d, h) for d, h in zip(dev, host))
    # one kernel for both device paths: the resident coordinates of K handles give the same bits
    handles = [smooth.Smoother(m, solver.Option.hip(inner=solver.Inner.relax)) for m in cut_meshes(blocks)]
    try:
        res = st.block(handles, 0)
        for h in handles:
            h.download()
        up = st.block([h._mesh for h in handles], 0)
        assert all(np.array_equal(a, b) for a, b in zip(res, up))
        assert all(np.array_equal(a, b) for a, b in zip(res, dev))   # create uploads the coordinates as they are
    finally:
        for h in handles:
            h.close()


def test_sin_cos_of_the_device_alone():
    # the mapping's sin / cos in isolation: two equal cuts at radius 1, one layer at radius 1 -> theta = y, output (x, sin y, cos y)
    y = np.linspace(-6.5, 6.5, 33 * 31).reshape(33, 31)
    r = np.stack([np.zeros_like(y), y], axis=-1)
    st = stack.Stack([1.0, 2.0], [1.0], "linear", "cylindrical")
    X, Y, Z = st.block(cut_meshes([r, 2.0 * r]), 0)
    t = y.T.astype(LD)
    ulp_s = np.abs(Y[0].astype(LD) - np.sin(t)) / np.spacing(np.abs(np.sin(t)).astype(np.float64))
    ulp_c = np.abs(Z[0].astype(LD) - np.cos(t)) / np.spacing(np.abs(np.cos(t)).astype(np.float64))
    print(f"stack_parity: device sin / cos alone on [-6.5, 6.5]: worst error sin {float(ulp_s.max()):.3f} ulp cos {float(ulp_c.max()):.3f} ulp (bar 4)")
    assert float(ulp_s.max()) <= 4.0 and float(ulp_c.max()) <= 4.0


def test_resident_coordinates_are_what_is_stacked():
    meshes = [configs.single_block(33, 31, amplitude=0.05 + 0.02 * c) for c in range(3)]
    seeds = [m.blocks[0].points.data.copy() for m in meshes]
    z = [0.0, 0.4, 1.0]
    st = stack.Stack(z, stack.layers_from(z, 7))
    handles = [smooth.Smoother(m, solver.Option.hip(inner=solver.Inner.relax)) for m in meshes]
    try:
        for h in handles:
            h.iterate(2)
        res = st.block(handles, 0)            # ordered behind the sweeps, nothing downloaded
        for h in handles:
            h.download()
        down = st.block(meshes, 0)
        assert all(np.array_equal(a, b) for a, b in zip(res, down))
        from_seeds = st.block(cut_meshes(seeds), 0)
        assert not np.array_equal(res[0], from_seeds[0]) or not np.array_equal(res[1], from_seeds[1])
        assert np.array_equal(res[0][0], meshes[0].blocks[0].points.data[..., 0].T) and np.array_equal(res[1][-1], meshes[2].blocks[0].points.data[..., 1].T)
    finally:
        for h in handles:
            h.close()


def _smoothers_rc(handles, z, s, block=0):
    z, s = np.asarray(z, dtype=np.float64), np.asarray(s, dtype=np.float64)
    opt = _capi.tm_stack_opt(z.size, _capi.f64ptr(z), s.size, _capi.f64ptr(s), 1, 0)
    out = [np.empty(s.size * 40 * 40) for _ in range(3)]
    arr = (C.c_void_p * len(handles))(*handles)
    return _capi.lib().tm_stack_smoothers(arr, C.byref(opt), block, 0, s.size, *[_capi.f64ptr(o) for o in out])


def test_error_codes_of_the_handle_path():
    z, s = [1.0, 2.0], [1.5]
    a = smooth.Smoother(cfr.single_block_mesh(cfr.bent_clustered(9, 8)), solver.Option.hip(inner=solver.Inner.relax))
    b = smooth.Smoother(cfr.single_block_mesh(cfr.bent_clustered(9, 8, seed=1)), solver.Option.hip(inner=solver.Inner.relax))
    other = smooth.Smoother(cfr.single_block_mesh(cfr.bent_clustered(9, 7)), solver.Option.hip(inner=solver.Inner.relax))
    strip = smooth.Smoother(configs.strip(2, 9, 8), solver.Option.hip(inner=solver.Inner.relax))
    dead = smooth.Smoother(cfr.single_block_mesh(cfr.bent_clustered(9, 8)), solver.Option.hip(inner=solver.Inner.relax))
    dead_handle = dead._h.value
    dead.close()
    try:
        assert _smoothers_rc([a._h, b._h], z, s) == _capi.TM_OK
        assert _smoothers_rc([a._h, other._h], z, s) == _capi.TM_E_SIZE          # unequal sizes between handles
        assert _smoothers_rc([a._h, strip._h], z, s) == _capi.TM_E_SIZE          # unequal block counts
        assert _smoothers_rc([a._h, b._h], z, s, block=1) == _capi.TM_E_ARG      # no such block
        assert _smoothers_rc([a._h, None], z, s) == _capi.TM_E_ARG               # NULL handle in the list
        assert _smoothers_rc([a._h, dead_handle], z, s) == _capi.TM_E_ARG        # destroyed handle in the list
        assert _smoothers_rc([a._h, b._h], z, [2.5]) == _capi.TM_E_ARG
        with pytest.raises(ValueError):
            stack.Stack(z, s).block([a, b], 0, host=True)
    finally:
        for h in (a, b, other, strip):
            h.close()


def test_handle_that_does_not_own_the_block():
    # a rank of a two-rank partition owns block 0 only: stacking block 1 from it is refused (cuts spread over ranks are not served)
    from turbomesh_amd.distributed import HooksBase

    class NullHooks(HooksBase):   # a transport that moves nothing: the handle is only created and read, never iterated
        def exchange(self, send, recv):
            pass

        def exchange_wait(self):
            pass

        def allreduce(self, t):
            pass

    part = NullHooks(configs.strip(2, 9, 8), [0, 1], 0, 2, option=solver.Option.hip(inner=solver.Inner.relax))
    whole = smooth.Smoother(configs.strip(2, 9, 8), solver.Option.hip(inner=solver.Inner.relax))
    try:
        assert _smoothers_rc([whole._h, part.smoother._h], [1.0, 2.0], [1.5], block=0) == _capi.TM_OK
        assert _smoothers_rc([whole._h, part.smoother._h], [1.0, 2.0], [1.5], block=1) == _capi.TM_E_ARG
        assert _smoothers_rc([part.smoother._h, whole._h], [1.0, 2.0], [1.5], block=1) == _capi.TM_E_ARG
        assert _smoothers_rc([whole._h, whole._h], [1.0, 2.0], [1.5], block=1) == _capi.TM_OK
    finally:
        whole.close()
        part.smoother.close()


# ------------------------------------------------------------------ Python layer, CLI, harness
def _t106_cut_files(tmp_path):
    base = json.load(open(os.path.join(GOLD, "examples", "T106", "T106.json")))
    files = [os.path.join(GOLD, "examples", "T106", "T106.json")]
    for c, f in ((1, 1.03), (2, 1.06)):
        d = json.loads(json.dumps(base))
        d["geometry"]["pitch"] = base["geometry"]["pitch"] * f
        for k in ("down_csv_path", "up_csv_path"):
            d["geometry"]["profile"]["csv"][k] = os.path.join(GOLD, base["geometry"]["profile"]["csv"][k])
        p = str(tmp_path / f"T106_cut{c}.json")
        json.dump(d, open(p, "w"))
        files.append(p)
    return files


T106_SIZES = [(221, 41), (121, 41), (11, 41), (11, 51), (121, 41), (161, 11), (21, 91), (11, 131)]


def test_t106_three_cuts_through_mesh3d(tmp_path):
    from turbomesh_amd.input import Input

    meshes = []
    for f in _t106_cut_files(tmp_path):
        inp = Input.parse(open(f).read())
        meshes.append(inp.template.run(inp.geometry(GOLD)))
    z = [0.0, 0.05, 0.1]
    st = stack.Stack(z, stack.layers_from(z, 5))
    handles = [smooth.Smoother(m, solver.Option.hip()) for m in meshes]
    try:
        for h in handles:
            h.iterate(1)
        m3 = st.mesh3d(handles)
        for h in handles:
            h.download()
    finally:
        for h in handles:
            h.close()
    assert len(m3.blocks) == 8 and m3.names == meshes[0].names
    assert m3.sizes() == [(ni, nj, 5) for ni, nj in T106_SIZES]
    f = str(tmp_path / "t106_3d.xyz")
    m3.write(f)
    back = output.read_plot3d_3d(f)
    assert [(b[0], b[1], b[2]) for b in back] == m3.sizes()
    for b, (ni, nj, nk, X, Y, Z) in enumerate(back):
        assert np.array_equal(X, m3.blocks[b][0]) and np.array_equal(Y, m3.blocks[b][1]) and np.array_equal(Z, m3.blocks[b][2])
        for layer, cut in ((0, 0), (4, 2)):   # the first and the last layer are cuts 0 and 2
            xy = meshes[cut].blocks[b].points.data
            assert np.array_equal(X[layer], xy[..., 0].T) and np.array_equal(Y[layer], xy[..., 1].T)
            assert np.all(Z[layer] == z[cut])
        assert np.isfinite(X).all() and np.isfinite(Y).all()


def test_cli_stacks_three_t106_cuts(tmp_path):
    files = _t106_cut_files(tmp_path)
    out = str(tmp_path / "blade.xyz")
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "turbomesh_amd", files[0], "--hip", "--iterations", "1", "--stack", files[1], files[2], "--span", "0,0.05,0.1",
                        "--layers", "5", "--output", out], capture_output=True, text=True, timeout=600, cwd=GOLD, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "3 cuts, 5 layers" in r.stderr
    back = output.read_plot3d_3d(out)
    assert [(b[0], b[1], b[2]) for b in back] == [(ni, nj, 5) for ni, nj in T106_SIZES]
    assert all(np.isfinite(b[3]).all() and np.isfinite(b[4]).all() for b in back)
    assert all(np.array_equal(b[5][k], np.full_like(b[5][k], s)) for b in back for k, s in ((0, 0.0), (4, 0.1)))


def test_harness_stacks_config5_cuts():
    r = subprocess.run([HARNESS, "stack", "33", "25", "3", "7"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "stack: layers at cuts equal the cuts: yes" in r.stdout
    assert len([l for l in r.stdout.splitlines() if l.startswith("stack: layer ")]) == 7
