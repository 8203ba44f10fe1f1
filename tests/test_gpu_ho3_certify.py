"""GPU: the certificate of high-order hexahedra on the device (include/tm_hip.h, "high-order hexahedra: certificate"; kernel K17) against
the host definition, the handle path, the CLI and the harness.

The statement needs no tolerance: record, status and bounds of tm_stack_certify equal tm_ho3_certify_planes_host applied to the planes
tm_stack_block[_surf] (K11) returned for the same inputs, bit for bit -- the fine nodes are K11's own launch, every rounded expression is
the function the host loops over (tm_highorder3_cert.hpp), and only minima, maxima and counts are combined across lanes."""
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
from tests.test_highorder3_cpu import cut_meshes, elevation, stack_for
from tests.test_ho3_certify_cpu import HIDDEN, HIDDEN_LEVEL, ROUGH_SEEDS, curved_cuts, rough_cuts, same_certificate, smooth_cuts
from turbomesh_amd import _capi, configs, highorder, stack
from turbomesh_amd.smoothing import smooth, solver

pytestmark = pytest.mark.gpu
HARNESS = os.path.join(ROOT, "turbomesh_amd", "tm_harness")
PROVEN, INVALID, UNDECIDED = _capi.TM_HO_PROVEN, _capi.TM_HO_INVALID, _capi.TM_HO_UNDECIDED

# (p, ni, nj, nk): fewer elements than a workgroup has rounds; odd element counts; one element; 8192 elements -- 2048 records, past the
# reduce threshold of 256, and with the plane budget forced small a window boundary; element counts that are no multiple of the
# elements per workgroup (4 rounds)
SHAPES = [(1, 4, 3, 2), (2, 7, 5, 5), (2, 5, 9, 3), (3, 7, 10, 4), (4, 9, 5, 9), (4, 5, 5, 5), (1, 33, 33, 9), (2, 9, 7, 7)]
GEOMETRIES = {"smooth": smooth_cuts, "rough": rough_cuts, "curved": curved_cuts}
MAPPINGS = ("planar", "cylindrical", "revolution")


def certify_both(st, cuts, el, depth):
    """(device, host on what K11 wrote)"""
    rev = st.surfaces is not None
    fine = st.block(cuts, 0, return_outside=rev)
    want = highorder.certify3d(*fine[:3], el, depth)
    got = st.certify(cuts, el, 0, max_depth=depth)
    return got, want


def assert_equal(got, want):
    assert same_certificate(got[0], want[0]), (got[0], want[0])
    assert got[1].shape == want[1].shape and got[1].tobytes() == want[1].tobytes()
    assert got[2].shape == want[2].shape and got[2].tobytes() == want[2].tobytes()


def runs(shape):
    """(name, mapping, stack, cuts, depth) of every run on a shape: the three geometries times the three mappings, K = 2 and 3
    alternating; the rough geometry at depth 3 with ROUGH_SEEDS[p] draws, the others at the depths 0 .. 3 in turn."""
    p, ni, nj, nk = shape
    for gi, (name, make) in enumerate(GEOMETRIES.items()):
        for mi, mapping in enumerate(MAPPINGS):
            K = 2 + (gi + mi) % 2
            interpolation = "cubic" if K == 3 else "linear"
            # cuts unevenly spaced 1 : 100 with layers at random positions (splines that overshoot, elements stretched in span), and cuts
            # and layers evenly spaced
            uneven = stack_for(K, nk, interpolation, mapping, seed=ni + K)
            z = sr.spans(K, "uniform")
            sf = stack.Surfaces(*ssr.tables(K, seed=ni + K)) if mapping == "revolution" else None
            even = stack.Stack(z, stack.layers_from(z, nk), interpolation, mapping, surfaces=sf)
            if name != "rough":
                yield name, mapping, even, cut_meshes(make(ni, nj, K, p)), (gi + mi) % 4
                continue
            for seed in range(ROUGH_SEEDS[p]):   # even draws on the uneven stack, odd draws (with the smaller noise) on the even one
                yield name, mapping, even if seed % 2 else uneven, cut_meshes(make(ni, nj, K, p, seed)), 3


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(str(v) for v in s))
def test_device_equals_host_on_what_k11_writes(shape, monkeypatch):
    p, ni, nj, nk = shape
    el = elevation(p, "gauss_lobatto")
    elements = ((ni - 1) // p) * ((nj - 1) // p) * ((nk - 1) // p)
    seen = set()
    for name, mapping, st, cuts, depth in runs(shape):
        got, want = certify_both(st, cuts, el, depth)
        assert_equal(got, want)
        c = got[0]
        assert c.elements == elements == c.proven + c.invalid + c.undecided and c.order == p and c.max_depth == depth
        assert sum(c.decided_at) == c.proven + c.invalid and got[1].shape == ((nk - 1) // p, (nj - 1) // p, (ni - 1) // p)
        seen |= set(np.unique(got[1]).tolist())
        if ni == 33 and name == "rough" and mapping == "planar":   # three span elements per window: three windows, the last one short
            monkeypatch.setenv("TM_HO3_CERT_WINDOW_BYTES", str(24 * ni * nj * 4))
            assert_equal(st.certify(cuts, el, 0, max_depth=depth), want)
            monkeypatch.delenv("TM_HO3_CERT_WINDOW_BYTES")
    assert PROVEN in seen


@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_what_the_rough_blocks_exercise(p):
    """From the host results alone: the rough inputs of the test above show every verdict and every deciding level at each order."""
    el = elevation(p, "gauss_lobatto")
    counts, levels = np.zeros(3, dtype=np.int64), np.zeros(4, dtype=np.int64)
    for shape in SHAPES:
        if shape[0] != p:
            continue
        for name, mapping, st, cuts, depth in runs(shape):
            if name == "rough":
                c = st.certify(cuts, el, 0, host=True, max_depth=depth)[0]
                counts += (c.proven, c.invalid, c.undecided)
                levels += c.decided_at
    print(f"ho3_certify: rough p {p}: proven / invalid / undecided {counts.tolist()} of {counts.sum()}, decided at {levels.tolist()}")
    assert (counts > 0).all() and (levels > 0).all()


def test_the_extruded_hidden_folds_on_the_device():
    for p in (2, 3):
        cut = cfr.single_block_mesh(HIDDEN[p])
        st = stack.Stack([0.0, float(p)], np.arange(p + 1, dtype=np.float64), "linear", "planar")
        el = elevation(p, "equidistant")
        c, status, bounds = st.certify([cut, cut], el, 0, max_depth=3)
        assert_equal((c, status, bounds), highorder.certify3d(*st.block([cut, cut], 0), el, 3))
        assert status[0, 0, 0] == INVALID and c.hidden_invalid == 1 and c.decided_at[HIDDEN_LEVEL[p]] == 1


def _handles(ni=17, nj=13, K=3):
    meshes = [configs.single_block(ni, nj, amplitude=0.05 + 0.02 * c) for c in range(K)]
    return meshes, [smooth.Smoother(m, solver.Option.hip(inner=solver.Inner.relax)) for m in meshes]


def test_resident_coordinates_are_what_is_certified():
    z = [0.0, 0.4, 1.0]
    st = stack.Stack(z, stack.layers_from(z, 5))
    el = elevation(2, "gauss_lobatto")
    plain_meshes, plain = _handles()
    watched_meshes, watched = _handles()
    try:
        for h in plain + watched:
            h.iterate(2)
        res = st.certify(watched, el, 0, max_depth=2)      # ordered behind the sweeps, nothing downloaded
        for h in plain + watched:
            h.iterate(2)
            h.download()
        for a, b in zip(plain_meshes, watched_meshes):     # the handles are unchanged by the call
            assert a.blocks[0].points.data.tobytes() == b.blocks[0].points.data.tobytes()
    finally:
        for h in plain + watched:
            h.close()
    again_meshes, again = _handles()
    try:
        for h in again:
            h.iterate(2)
            h.download()
        assert_equal(res, st.certify(again_meshes, el, 0, max_depth=2))
        assert_equal(st.certify(again, el, 0, max_depth=2), res)
        assert_equal(res, highorder.certify3d(*st.block(again, 0), el, 2))
        assert res[0].elements == 8 * 6 * 2
    finally:
        for h in again:
            h.close()


def _certify_rc(handles, z, s, order=2, block=0, depth=2, mapping=0):
    z, s = np.asarray(z, dtype=np.float64), np.asarray(s, dtype=np.float64)
    opt = _capi.tm_stack_opt(z.size, _capi.f64ptr(z), s.size, _capi.f64ptr(s), 1, mapping)
    ho = _capi.tm_ho_opt(order, _capi.TM_HO_GAUSS_LOBATTO, None)
    c = _capi.tm_ho3_certificate()
    return _capi.lib().tm_stack_smoothers_certify((C.c_void_p * len(handles))(*handles), C.byref(opt), None, C.byref(ho), depth, block, C.byref(c), None, None, None)


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
        assert _certify_rc(ok, z, s) == _capi.TM_OK and _certify_rc(ok, z, s, depth=0) == _capi.TM_OK and _certify_rc(ok, z, s, order=1, depth=3) == _capi.TM_OK
        assert _certify_rc([a._h, dead_handle], z, s) == _capi.TM_E_ARG           # a dead handle
        assert _certify_rc([a._h, None], z, s) == _capi.TM_E_ARG
        assert _certify_rc([whole._h, part.smoother._h], z, s, block=0) == _capi.TM_OK
        assert _certify_rc([whole._h, part.smoother._h], z, s, block=1) == _capi.TM_E_ARG   # a handle that does not own the block
        assert _certify_rc([h._h for h in odd], z, s) == _capi.TM_E_SIZE         # 7 cells along j at order 2
        assert _certify_rc(ok, z, s[:4]) == _capi.TM_E_SIZE                      # 3 layer cells at order 2
        assert _certify_rc(ok, z, s, order=5) == _capi.TM_E_ARG                  # an order hexahedra do not take
        assert _certify_rc(ok, z, s, depth=4) == _capi.TM_E_ARG and _certify_rc(ok, z, s, depth=-1) == _capi.TM_E_ARG
        assert _certify_rc(ok, z, s, mapping=_capi.TM_STACK_REVOLUTION) == _capi.TM_E_ARG   # revolution without surfaces
        with pytest.raises(ValueError):
            stack.Stack(z, s).certify([a, b], elevation(2, "gauss_lobatto"), 0, host=True)
    finally:
        for h in (a, b, *odd, whole, part.smoother):
            h.close()


def test_cli_certifies_three_stacked_t106_cuts(tmp_path):
    files = _t106_cuts(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT)
    base = [sys.executable, "-m", "turbomesh_amd", files[0], "--hip", "--iterations", "1", "--stack", files[1], files[2], "--span", "0,0.05,0.1", "--layers", "5", "--order", "2"]
    plain, flagged = str(tmp_path / "plain.xyz"), str(tmp_path / "flagged.xyz")
    elements = sum((ni - 1) * (nj - 1) for ni, nj in T106_SIZES) // 4 * 2
    r0 = subprocess.run(base + ["--output", plain], capture_output=True, text=True, timeout=600, cwd=GOLD, env=env)
    r = subprocess.run(base + ["--output", flagged, "--stack-certify"], capture_output=True, text=True, timeout=600, cwd=GOLD, env=env)
    assert r0.returncode == 0 and r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stderr.splitlines() if l.startswith("INFO(quality): certify3d ")]
    assert len(lines) == 9 and lines[-1].startswith(f"INFO(quality): certify3d total: order 2 depth 2 elements {elements} proven "), r.stderr[-3000:]
    assert not [l for l in r0.stderr.splitlines() if "certify3d" in l]
    counts = {k: int(lines[-1].split()[lines[-1].split().index(k) + 1]) for k in ("elements", "proven", "invalid", "undecided")}
    assert counts["proven"] + counts["invalid"] + counts["undecided"] == counts["elements"]
    per_block = [int(l.split()[l.split().index("elements") + 1]) for l in lines[:-1]]
    assert sum(per_block) == elements
    with open(plain, "rb") as fa, open(flagged, "rb") as fb:
        assert fa.read() == fb.read()                                            # the certificate changes nothing that is written
    r = subprocess.run(base + ["--output", flagged, "--stack-certify", "1", "--fail-on-unproven-elements"], capture_output=True, text=True, timeout=600,
                       cwd=GOLD, env=env)
    total = [l for l in r.stderr.splitlines() if l.startswith("INFO(quality): certify3d total: ")][0].split()
    assert total[total.index("depth") + 1] == "1"
    assert (r.returncode != 0) == (int(total[total.index("proven") + 1]) != elements), r.stderr[-3000:]


def test_harness_certifies_stacked_cuts():
    r = subprocess.run([HARNESS, "stack-certify", "17", "13", "3", "5", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"^stack-certify: hexahedra 96 proven \d+ invalid \d+ undecided \d+", r.stdout, flags=re.M), r.stdout
    assert "stack-certify: device equals host: yes" in r.stdout
