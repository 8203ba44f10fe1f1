"""GPU: high-order elevation (include/tm_hip.h, "high-order elements"; kernel K13) against the host evaluation of the same definition
(bit for bit: planes, scaled Jacobians, every field of the record) and against tests/ho_reference.py (numpy longdouble) within its bar;
the resident path, its error codes, folded elements, the Python layer, the CLI and the C++ harness.  No timing and no measured
threshold is asserted; the printed `ho_parity:` lines are kept in profiles/ho_parity.txt."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import control_field_reference as cfr
from tests import ho_reference as hr
from tests.conftest import ROOT
from tests.test_o4h import GOLD
from turbomesh_amd import _capi, configs, highorder, output
from turbomesh_amd.smoothing import smooth, solver

pytestmark = pytest.mark.gpu

HARNESS = os.path.join(ROOT, "turbomesh_amd", "tm_harness")
DISTRIBUTIONS = ("equidistant", "gauss_lobatto", "prescribed")
# a single element per order, and per order a block with at least two full tiles and a ragged one in both directions for any tile of up
# to 40 nodes; the last two: 256 and 272 workgroups, either side of the size from which the records are combined in two stages
SHAPES = ([(p, p + 1, p + 1) for p in range(1, 9)] + [(2, 67, 131), (3, 67, 130), (4, 69, 133), (5, 66, 131), (6, 67, 133), (7, 71, 134), (8, 73, 137)] +
          [(1, 257, 257), (1, 273, 257)])


def elevation(p, dist):
    return highorder.Elevation(p, dist, hr.prescribed_nodes(p) if dist == "prescribed" else None)


@functools.lru_cache(maxsize=None)
def case_data(p, ni, nj, dist):
    """Input, host evaluation and longdouble reference of a case: computed once, shared, never modified."""
    X = cfr.bent_clustered(ni, nj)
    host = elevation(p, dist).block(cfr.single_block_mesh(X), 0, host=True)
    ref = hr.Reference(X, p, dist, hr.prescribed_nodes(p) if dist == "prescribed" else None)
    for a in (X, host[0], host[1], host[3], ref.Y, ref.bar_Y):
        a.setflags(write=False)
    return X, host, ref


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def same_record(a, b):
    """Every field bit for bit (a NaN equals a NaN)."""
    return bytes(a.to_struct()) == bytes(b.to_struct())


@pytest.mark.parametrize("p,ni,nj", SHAPES, ids=lambda v: str(v))
def test_device_equals_host_and_stays_within_the_reference_bar(p, ni, nj):
    for dist in DISTRIBUTIONS:
        X, (hx, hy, hq, hsj), ref = case_data(p, ni, nj, dist)
        dx, dy, dq, dsj = elevation(p, dist).block(cfr.single_block_mesh(X), 0)
        assert same_bits(dx, hx) and same_bits(dy, hy), dist
        assert same_bits(dsj, hsj), dist
        assert same_record(dq, hq), (dist, dq, hq)                       # no summed field: every field bit for bit
        ratio = hr.worst_ratio(np.stack([dx.T, dy.T], axis=-1), ref.Y, ref.bar_Y)
        print(f"ho_parity: device p {p} {ni} x {nj} {dist}: worst |Y - Y_ref| / bar {ratio:.3f}; elements {dq.elements} invalid {dq.invalid} "
              f"(reference {ref.invalid})")
        assert ratio <= 1.0
        assert dq.elements == ref.Ei * ref.Ej and dq.order == p
        # a report alone gives the same record
        _, _, q_alone, sj_alone = elevation(p, dist).block(cfr.single_block_mesh(X), 0, planes=False)
        assert same_record(q_alone, dq) and same_bits(sj_alone, dsj)


@pytest.mark.parametrize("p,ni,nj", [(1, 67, 130), (2, 67, 131), (5, 66, 131), (8, 73, 137)])
def test_copied_planes_equal_the_export_planes(p, ni, nj):
    X = cfr.bent_clustered(ni, nj).copy()
    X[0, 0, 1] = -0.0
    ex, ey = output.block_planes(X)
    for dist in DISTRIBUTIONS if p == 1 else ("equidistant",):
        dx, dy, _, _ = elevation(p, dist).block(cfr.single_block_mesh(X), 0)
        assert dx.reshape(-1).tobytes() == ex.tobytes() and dy.reshape(-1).tobytes() == ey.tobytes()


def test_resident_coordinates_are_what_is_elevated():
    el = elevation(2, "gauss_lobatto")
    mesh = configs.single_block(33, 31, amplitude=0.07)
    seed = mesh.blocks[0].points.data.copy()
    with smooth.Smoother(mesh, solver.Option.hip(inner=solver.Inner.relax)) as sm:
        sm.iterate(2)
        rx, ry, rq, rsj = sm.elevate(el, 0)                             # ordered behind the sweeps, nothing downloaded
        before = mesh.blocks[0].points.data.copy()
        sm.download()
        again = sm.elevate(el, 0)
    assert np.array_equal(before, seed) and not np.array_equal(mesh.blocks[0].points.data, seed)
    dx, dy, dq, dsj = el.block(mesh, 0)
    assert same_bits(rx, dx) and same_bits(ry, dy) and same_bits(rsj, dsj) and same_record(rq, dq)
    assert same_bits(again[0], rx) and same_record(again[2], rq)                   # the call modified nothing
    sx, sy, _, _ = el.block(cfr.single_block_mesh(seed), 0)
    assert not (np.array_equal(sx, rx) and np.array_equal(sy, ry))

    strip = configs.strip(2, 9, 13)
    el4 = elevation(4, "gauss_lobatto")
    with smooth.Smoother(strip, solver.Option.hip(inner=solver.Inner.relax)) as sm:
        sm.iterate(2)
        res = [sm.elevate(el4, b) for b in (0, 1)]
        sm.download()
    for b in (0, 1):
        dx, dy, dq, dsj = el4.block(strip, b)
        assert same_bits(res[b][0], dx) and same_bits(res[b][1], dy) and same_bits(res[b][3], dsj) and same_record(res[b][2], dq)
        assert dq.worst_block == b and dq.elements == 2 * 3


def _elevate_rc(handle, order, block, distribution=_capi.TM_HO_GAUSS_LOBATTO):
    opt = _capi.tm_ho_opt(order, distribution, None)
    x, y, sj = np.empty(64 * 64), np.empty(64 * 64), np.empty(64 * 64)
    q = _capi.tm_ho_quality()
    return _capi.lib().tm_smoother_elevate(handle, C.byref(opt), block, _capi.f64ptr(x), _capi.f64ptr(y), C.byref(q), _capi.f64ptr(sj))


def test_error_codes_of_the_handle_path():
    a = smooth.Smoother(cfr.single_block_mesh(cfr.bent_clustered(9, 13)), solver.Option.hip(inner=solver.Inner.relax))
    dead = smooth.Smoother(cfr.single_block_mesh(cfr.bent_clustered(9, 13)), solver.Option.hip(inner=solver.Inner.relax))
    dead_handle = dead._h.value
    dead.close()
    try:
        assert _elevate_rc(a._h, 4, 0) == _capi.TM_OK
        assert _elevate_rc(a._h, 2, 0) == _capi.TM_OK
        assert _elevate_rc(a._h, 3, 0) == _capi.TM_E_SIZE                # 8 x 12 cells
        assert b"block 0" in _capi.lib().tm_last_error()
        assert _elevate_rc(a._h, 8, 0) == _capi.TM_E_SIZE
        assert _elevate_rc(a._h, 4, 1) == _capi.TM_E_ARG                 # no such block
        assert _elevate_rc(a._h, 0, 0) == _capi.TM_E_ARG and _elevate_rc(a._h, 9, 0) == _capi.TM_E_ARG
        assert _elevate_rc(a._h, 4, 0, distribution=5) == _capi.TM_E_ARG
        assert _elevate_rc(a._h, 4, 0, distribution=_capi.TM_HO_PRESCRIBED) == _capi.TM_E_ARG   # no nodes
        assert _elevate_rc(None, 4, 0) == _capi.TM_E_ARG                 # NULL handle
        assert _elevate_rc(dead_handle, 4, 0) == _capi.TM_E_ARG          # destroyed handle
        with pytest.raises(ValueError):
            elevation(4, "gauss_lobatto").block(a, 0, host=True)
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
        assert _elevate_rc(part.smoother._h, 4, 0) == _capi.TM_OK
        assert _elevate_rc(part.smoother._h, 4, 1) == _capi.TM_E_ARG
    finally:
        part.smoother.close()


@pytest.mark.parametrize("p,ni,nj", [(2, 7, 9), (3, 10, 7), (4, 9, 13), (8, 17, 17)])
def test_folded_elements_on_the_device(p, ni, nj):
    clean = cfr.bent_clustered(ni, nj)
    folded = hr.fold(clean, p)
    for dist in ("gauss_lobatto", "equidistant"):
        ref_c, ref_f = hr.Reference(clean, p, dist), hr.Reference(folded, p, dist)
        assert ref_c.invalid == 0 and ref_f.invalid >= 1 and ref_f.valid.sum() >= 1
        qc = elevation(p, dist).block(cfr.single_block_mesh(clean), 0)[2]
        _, _, qf, sj = elevation(p, dist).block(cfr.single_block_mesh(folded), 0)
        assert qc.invalid == ref_c.invalid and qf.invalid == ref_f.invalid
        assert np.array_equal(np.isnan(sj.T), ~ref_f.valid)
        hq, hsj = elevation(p, dist).block(cfr.single_block_mesh(folded), 0, host=True)[2:]
        assert same_record(qf, hq) and same_bits(sj, hsj)


# ------------------------------------------------------------------ Python layer, CLI, harness
T106_SIZES = [(221, 41), (121, 41), (11, 41), (11, 51), (121, 41), (161, 11), (21, 91), (11, 131)]


def test_t106_at_order_two_through_the_python_layer(tmp_path, caplog):
    import logging

    from turbomesh_amd import quality
    from turbomesh_amd.input import Input

    inp = Input.parse(open(os.path.join(GOLD, "examples", "T106", "T106.json")).read())
    mesh = inp.template.run(inp.geometry(GOLD))
    el = elevation(2, "equidistant")
    el.check(mesh)
    elevation(5, "gauss_lobatto").check(mesh)
    with smooth.Smoother(mesh, solver.Option.hip()) as sm:
        sm.iterate(1)
        hom = el.mesh(sm)
        sm.download()
    assert len(hom.blocks) == 8 and hom.names == mesh.names and hom.sizes() == T106_SIZES
    assert hom.elements() == [((ni - 1) // 2, (nj - 1) // 2) for ni, nj in T106_SIZES]
    assert [q.elements for q in hom.per_block] == [(ni - 1) * (nj - 1) // 4 for ni, nj in T106_SIZES]     # a quarter of the cells
    assert hom.total.elements == sum((ni - 1) * (nj - 1) for ni, nj in T106_SIZES) // 4 and hom.total.order == 2
    for b, (X, Y) in enumerate(hom.blocks):                              # equidistant: the smoothed nodes themselves
        xy = mesh.blocks[b].points.data
        assert np.array_equal(X, xy[..., 0].T) and np.array_equal(Y, xy[..., 1].T)
    f = str(tmp_path / "t106.vtk")
    hom.write(f)
    points, cells, types = output.read_vtk_lagrange(f)
    assert len(points) == sum(ni * nj for ni, nj in T106_SIZES) and cells.shape == (hom.total.elements, 9) and np.all(types == 70)
    assert np.array_equal(points[:221 * 41, 0], hom.blocks[0][0].reshape(-1))
    with caplog.at_level(logging.INFO, logger="quality"):
        quality.log_report_ho(logging.getLogger("quality"), hom.names, hom.per_block, hom.total)
    assert sum("elevate" in r.getMessage() and "order 2 elements" in r.getMessage() for r in caplog.records) == 9


def test_cli_elevates_t106(tmp_path):
    out = str(tmp_path / "t106.vtk")
    env = dict(os.environ, PYTHONPATH=ROOT)
    cfg = os.path.join(GOLD, "examples", "T106", "T106.json")
    r = subprocess.run([sys.executable, "-m", "turbomesh_amd", cfg, "--hip", "--iterations", "1", "--order", "2", "--fail-on-invalid-elements", "--output", out],
                       capture_output=True, text=True, timeout=600, cwd=GOLD, env=env)
    total = sum((ni - 1) * (nj - 1) for ni, nj in T106_SIZES) // 4
    lines = [l for l in r.stderr.splitlines() if "elevate " in l]
    assert len(lines) == 9 and f"elevate total: order 2 elements {total} invalid" in lines[-1], r.stderr[-3000:]
    invalid = int(lines[-1].split(" invalid ")[1].split()[0])
    assert (r.returncode == 0) == (invalid == 0), r.stderr[-3000:]       # non-zero under the flag exactly when invalid elements remain
    points, cells, types = output.read_vtk_lagrange(out)                 # the file is written either way
    assert cells.shape == (total, 9) and np.all(types == 70) and np.isfinite(points).all()
    assert len(points) == sum(ni * nj for ni, nj in T106_SIZES)


def test_cli_names_the_block_the_order_does_not_divide(tmp_path):
    out = str(tmp_path / "t106.xyz")
    env = dict(os.environ, PYTHONPATH=ROOT)
    cfg = os.path.join(GOLD, "examples", "T106", "T106.json")
    r = subprocess.run([sys.executable, "-m", "turbomesh_amd", cfg, "--hip", "--iterations", "1", "--order", "3", "--output", out],
                       capture_output=True, text=True, timeout=600, cwd=GOLD, env=env)
    assert r.returncode != 0 and "block 0" in r.stderr and "order 3" in r.stderr, r.stderr[-3000:]
    assert "iteration:" not in r.stderr and not os.path.exists(out)      # refused before anything is smoothed


def test_harness_elevates():
    r = subprocess.run([HARNESS, "elevate", "33", "25", "4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"^elevate: elements 48 invalid \d+ min sj ", r.stdout, flags=re.M), r.stdout
    assert "elevate: corners unchanged: yes" in r.stdout and "elevate: device equals host: yes" in r.stdout
