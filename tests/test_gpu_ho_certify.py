"""GPU: the high-order certificate (include/tm_hip.h, "high-order elements: certificate"; kernel K14) against the host evaluation of the
same definition -- record, status and bounds bit for bit -- on smooth blocks and on rough ones where the subdivision reaches every
depth; the folds the nodes do not see, the resident path and its error codes, the CLI and the C++ harness.  The definition itself is
held to exact arithmetic in tests/test_ho_certify_cpu.py."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import control_field_reference as cfr
from tests import ho_certify_reference as cr
from tests.conftest import ROOT
from tests.test_ho_certify_cpu import HIDDEN_2, HIDDEN_3
from tests.test_o4h import GOLD
from turbomesh_amd import _capi, configs, highorder, output, quality
from turbomesh_amd.smoothing import smooth, solver

pytestmark = pytest.mark.gpu

HARNESS = os.path.join(ROOT, "turbomesh_amd", "tm_harness")
PROVEN, INVALID, UNDECIDED = _capi.TM_HO_PROVEN, _capi.TM_HO_INVALID, _capi.TM_HO_UNDECIDED
# K14 packs 16 / 4 / 1 elements into a wave (p = 1 / 2 / 3..8) and gives a workgroup 8 rounds: 128 / 32 / 8 elements.  One element per
# order; the small shapes of the issue; per order a block whose element counts are multiples of neither in either direction (p = 5:
# 13 x 26, p = 8: 9 x 17, p = 1: 66 x 129, ...); the last: 519 workgroups, past the 256 records the finalize combines in one stage
SHAPES = ([(p, p + 1, p + 1) for p in range(1, 9)] + [(2, 7, 9), (3, 10, 7), (4, 9, 13), (8, 17, 17)] +
          [(1, 67, 130), (2, 67, 131), (3, 67, 130), (4, 69, 133), (5, 66, 131), (6, 67, 133), (7, 71, 134), (8, 73, 137)] + [(1, 258, 259)])


def elevation(p):
    return highorder.Elevation(p, "equidistant")


def curved_block(p, ni, nj, seed):
    """Elements of order p that are biquadratic maps: the amplitude-0.35 block on the grid of half elements, interpolated to the
    (p+1)^2 nodes of every element.  Node noise at order 5 and above only makes elements that are folded at their nodes (the
    interpolant oscillates); these are as close to folding as the order-2 ones, so their subdivision reaches every depth too."""
    Ei, Ej = (ni - 1) // p, (nj - 1) // p
    coarse = cr.dyadic_block(2 * Ei + 1, 2 * Ej + 1, 0.35, seed) * (p / 2.0)
    t = 2.0 * np.arange(p + 1) / p
    L = np.stack([(t - 1) * (t - 2) / 2, t * (2 - t), t * (t - 1) / 2], axis=1)              # (p+1, 3): quadratic Lagrange on 0, 1, 2
    X = np.empty((ni, nj, 2))
    for e in range(Ei):
        for f in range(Ej):
            X[e * p:e * p + p + 1, f * p:f * p + p + 1] = np.einsum("am,mnc,bn->abc", L, coarse[2 * e:2 * e + 3, 2 * f:2 * f + 3], L)
    return X


@functools.lru_cache(maxsize=None)
def case_data(p, ni, nj, kind):
    """Input and host evaluation of a case: computed once, shared, never modified."""
    X = {"smooth": lambda: cfr.bent_clustered(ni, nj), "rough": lambda: cr.dyadic_block(ni, nj, 0.35, seed=1000 * p + ni),
         "curved": lambda: curved_block(p, ni, nj, seed=2000 * p + ni)}[kind]()
    depth = 3 if kind == "smooth" else 4
    host = elevation(p).certify(cfr.single_block_mesh(X), 0, host=True, max_depth=depth)
    for a in (X, host[1], host[2]):
        a.setflags(write=False)
    return X, depth, host


def same_record(a, b):
    return bytes(a.to_struct()) == bytes(b.to_struct())


@pytest.mark.parametrize("kind", ["smooth", "rough", "curved"])
@pytest.mark.parametrize("p,ni,nj", SHAPES, ids=lambda v: str(v))
def test_device_equals_host(p, ni, nj, kind):
    X, depth, (hc, hst, hbd) = case_data(p, ni, nj, kind)
    dc, dst, dbd = elevation(p).certify(cfr.single_block_mesh(X), 0, max_depth=depth)
    print(f"ho_certify: device p {p} {ni} x {nj} {kind}: {dc.line('block')}")
    assert same_record(dc, hc), (dc, hc)
    assert np.array_equal(dst, hst) and dbd.tobytes() == hbd.tobytes()
    assert dc.proven + dc.invalid + dc.undecided == dc.elements == ((ni - 1) // p) * ((nj - 1) // p)
    if kind == "smooth" and ni > 4 * p:                                  # (a lone element of a clustered 2 x 2-cell block is folded at its nodes)
        assert dc.proven == dc.elements


def _seen(kind, order):
    decided, seen, hidden = np.zeros(5, dtype=np.int64), set(), 0
    for p, ni, nj in SHAPES:
        if p == order:
            hc, hst, _ = case_data(p, ni, nj, kind)[2]
            decided += hc.decided_at
            seen |= set(np.unique(hst).tolist())
            hidden += hc.hidden_invalid
    return decided, seen, hidden


def test_what_the_rough_blocks_exercise():
    """The amplitude-0.35 blocks at orders 2 and 3: elements decided at each level 0 .. 4, all three verdicts, folds the nodes do not
    see.  The biquadratic blocks at every order from 2: subdivision happens (their degree-elevated hulls are tighter the higher the order,
    so the deepest levels are reached at the low orders only), with proven and invalid elements."""
    for order in (2, 3):
        decided, seen, hidden = _seen("rough", order)
        assert np.all(decided > 0) and seen == {PROVEN, INVALID, UNDECIDED} and hidden > 0, (order, decided, seen, hidden)
    for order in range(2, 9):
        decided, seen, hidden = _seen("curved", order)
        assert decided[0] > 0 and decided[1:].sum() > 0 and {PROVEN, INVALID} <= seen, (order, decided, seen)


@pytest.mark.parametrize("p,X,level", [(2, HIDDEN_2, 2), (3, HIDDEN_3, 1)], ids=["p2", "p3"])
def test_hidden_folds_on_the_device(p, X, level):
    mesh = cfr.single_block_mesh(X)
    q = elevation(p).block(mesh, 0, planes=False)[2]
    assert q.invalid == 0                                                # K13 on the device: valid at every node
    for depth in range(5):
        dc, dst, dbd = elevation(p).certify(mesh, 0, max_depth=depth)
        hc, hst, hbd = elevation(p).certify(mesh, 0, host=True, max_depth=depth)
        assert same_record(dc, hc) and np.array_equal(dst, hst) and dbd.tobytes() == hbd.tobytes()
        assert dst[0, 0] == (UNDECIDED if depth < level else INVALID) and dc.hidden_invalid == int(depth >= level)
    # inside a block of valid elements, at an odd position
    big = cfr.bent_clustered(7 * p + 1, 5 * p + 1) * 40.0
    big[3 * p:4 * p + 1, 2 * p:3 * p + 1] = X + big[3 * p, 2 * p] - X[0, 0]
    dc, dst, dbd = elevation(p).certify(cfr.single_block_mesh(big), 0)
    hc, hst, hbd = elevation(p).certify(cfr.single_block_mesh(big), 0, host=True)
    assert same_record(dc, hc) and np.array_equal(dst, hst) and dbd.tobytes() == hbd.tobytes()
    assert dst[2, 3] == INVALID and dc.hidden_invalid >= 1 and (dc.first_unproven_e, dc.first_unproven_f) <= (3, 2)


def test_resident_coordinates_are_what_is_certified():
    el = elevation(2)
    mesh = configs.single_block(33, 31, amplitude=0.07)
    twin = configs.single_block(33, 31, amplitude=0.07)
    opt = solver.Option.hip(inner=solver.Inner.relax)
    with smooth.Smoother(mesh, opt) as sm, smooth.Smoother(twin, opt) as ref:
        sm.iterate(2)
        ref.iterate(2)
        rc, rst, rbd = sm.certify(el, 0)                                 # ordered behind the sweeps, nothing downloaded
        sm.download()
        again = sm.certify(el, 0)
        total = sm.certify(el)
        now = mesh.blocks[0].points.data.copy()
        sm.iterate(1)
        ref.iterate(1)
        sm.download()
        ref.download()
    dc, dst, dbd = el.certify(cfr.single_block_mesh(now), 0)
    assert same_record(rc, dc) and np.array_equal(rst, dst) and rbd.tobytes() == dbd.tobytes()
    assert same_record(again[0], rc) and again[2].tobytes() == rbd.tobytes() and same_record(total[0], rc)
    # neither the coordinates nor the next iterate were touched
    assert mesh.blocks[0].points.data.tobytes() == twin.blocks[0].points.data.tobytes()

    strip = configs.strip(2, 9, 13)
    el4 = elevation(4)
    with smooth.Smoother(strip, opt) as sm:
        sm.iterate(2)
        res = [sm.certify(el4, b) for b in (0, 1)]
        sm.download()
    for b in (0, 1):
        dc, dst, dbd = el4.certify(strip, b)
        assert same_record(res[b][0], dc) and np.array_equal(res[b][1], dst) and res[b][2].tobytes() == dbd.tobytes()
        assert dc.elements == 2 * 3 and (dc.proven == 0 or dc.worst_block == b)


def _certify_rc(handle, order, block, distribution=_capi.TM_HO_GAUSS_LOBATTO, depth=3):
    opt = _capi.tm_ho_opt(order, distribution, None)
    status, bounds = np.empty(64 * 64, dtype=np.uint8), np.empty(2 * 64 * 64)
    c = _capi.tm_ho_certificate()
    return _capi.lib().tm_smoother_certify(handle, C.byref(opt), depth, block, C.byref(c), status.ctypes.data_as(C.POINTER(C.c_uint8)), _capi.f64ptr(bounds))


def test_error_codes_of_the_handle_path():
    a = smooth.Smoother(cfr.single_block_mesh(cfr.bent_clustered(9, 13)), solver.Option.hip(inner=solver.Inner.relax))
    dead = smooth.Smoother(cfr.single_block_mesh(cfr.bent_clustered(9, 13)), solver.Option.hip(inner=solver.Inner.relax))
    dead_handle = dead._h.value
    dead.close()
    try:
        assert _certify_rc(a._h, 4, 0) == _capi.TM_OK
        assert _certify_rc(a._h, 2, 0, depth=0) == _capi.TM_OK and _certify_rc(a._h, 2, 0, depth=4) == _capi.TM_OK
        assert _certify_rc(a._h, 2, 0, depth=-1) == _capi.TM_E_ARG and _certify_rc(a._h, 2, 0, depth=5) == _capi.TM_E_ARG
        assert _certify_rc(a._h, 3, 0) == _capi.TM_E_SIZE                # 8 x 12 cells
        assert b"block 0" in _capi.lib().tm_last_error()
        assert _certify_rc(a._h, 8, 0) == _capi.TM_E_SIZE
        assert _certify_rc(a._h, 4, 1) == _capi.TM_E_ARG                 # no such block
        assert _certify_rc(a._h, 0, 0) == _capi.TM_E_ARG and _certify_rc(a._h, 9, 0) == _capi.TM_E_ARG
        assert _certify_rc(a._h, 4, 0, distribution=5) == _capi.TM_E_ARG
        assert _certify_rc(a._h, 4, 0, distribution=_capi.TM_HO_PRESCRIBED) == _capi.TM_E_ARG   # no nodes
        assert _certify_rc(None, 4, 0) == _capi.TM_E_ARG                 # NULL handle
        assert _certify_rc(dead_handle, 4, 0) == _capi.TM_E_ARG          # destroyed handle
        with pytest.raises(ValueError):
            elevation(4).certify(a, 0, host=True)
    finally:
        a.close()


def test_handle_that_does_not_own_the_block():
    from turbomesh_amd.distributed import HooksBase

    class NullHooks(HooksBase):   # a transport that moves nothing: the handle is only created and read, never iterated
        def exchange(self, send, recv):
            pass

        def exchange_wait(self):
            pass

        def allreduce(self, t):
            pass

    part = NullHooks(configs.strip(2, 9, 13), [0, 1], 0, 2, option=solver.Option.hip(inner=solver.Inner.relax))
    try:
        assert _certify_rc(part.smoother._h, 4, 0) == _capi.TM_OK
        assert _certify_rc(part.smoother._h, 4, 1) == _capi.TM_E_ARG
    finally:
        part.smoother.close()


# ------------------------------------------------------------------ CLI, harness
T106_SIZES = [(221, 41), (121, 41), (11, 41), (11, 51), (121, 41), (161, 11), (21, 91), (11, 131)]


def _cli(tmp_path, *flags):
    out = str(tmp_path / "t106.xyz")
    env = dict(os.environ, PYTHONPATH=ROOT)
    cfg = os.path.join(GOLD, "examples", "T106", "T106.json")
    r = subprocess.run([sys.executable, "-m", "turbomesh_amd", cfg, "--hip", "--iterations", "1", "--order", "2", "--nodes", "equidistant", "--output", out, *flags],
                       capture_output=True, text=True, timeout=600, cwd=GOLD, env=env)
    return r, out


def test_cli_certifies_t106(tmp_path):
    r, out = _cli(tmp_path, "--certify", "--fail-on-unproven-elements")
    total = sum((ni - 1) * (nj - 1) for ni, nj in T106_SIZES) // 4
    lines = [l.split(": ", 1)[1] for l in r.stderr.splitlines() if "certify " in l and "(quality)" in l]
    assert len(lines) == 9 and lines[-1].startswith(f"certify total: order 2 depth 3 elements {total} proven "), r.stderr[-3000:]
    assert sum("elevate " in l for l in r.stderr.splitlines()) == 9                            # next to the nodal report
    m = re.search(r"proven (\d+) invalid (\d+) undecided (\d+) hidden invalid (\d+)", lines[-1])
    proven, invalid, undecided, hidden = (int(v) for v in m.groups())
    assert proven + invalid + undecided == total
    assert (r.returncode == 0) == (proven == total), r.stderr[-3000:]                          # non-zero exactly when the record says so
    # the equidistant elevated nodes are the smoothed nodes: the host's certificate of what was written is what was logged
    blocks = output.read_plot3d(out)
    assert [(ni, nj) for ni, nj, _, _ in blocks] == T106_SIZES
    per_block = []
    for b, (ni, nj, x, y) in enumerate(blocks):
        X = np.stack([x, y], axis=-1)
        c = elevation(2).certify(cfr.single_block_mesh(X), 0, host=True)[0]
        c.worst_block = b if c.proven else 0
        c.first_unproven_block = b if c.has_unproven else 0
        per_block.append(c)
    names = [l.split(":")[0] for l in lines[:-1]]
    want = [c.line(n) for n, c in zip(names, per_block)] + [quality.total_ho_certificate(per_block).line("certify total")]
    assert lines == want


def test_cli_without_certify_is_unchanged(tmp_path):
    r, _ = _cli(tmp_path)
    assert r.returncode == 0 and "(quality): certify " not in r.stderr and sum("elevate " in l for l in r.stderr.splitlines()) == 9
    r = subprocess.run([sys.executable, "-m", "turbomesh_amd", "x.json", "--fail-on-unproven-elements"], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 2 and "--certify" in r.stderr


def test_harness_certifies():
    r = subprocess.run([HARNESS, "certify", "33", "25", "4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"^certify: elements 48 proven \d+ invalid \d+ undecided \d+ hidden invalid \d+ min scaled bound ", r.stdout, flags=re.M), r.stdout
    assert "certify: counts add up: yes" in r.stdout and "certify: device equals host: yes" in r.stdout
