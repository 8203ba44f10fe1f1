"""GPU: the 3-D elliptic smoothing on the device (kernels K22: k_s3_control_faces, k_s3_control_blend, k_s3_sweep) against its host twin,
bit for bit in the planes, in the control field and in every record field but the two sums, which agree within 2 (n-1) 2^-53 sum and
are the same from run to run; the stack entry point on resident handles; weld and command line behind the smoothing.

The kernel's constants (csrc/tm_smooth3d.hip): a workgroup owns S3_TI x S3_TJ nodes of an i-j plane and marches S3_KCHUNK node layers."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import control_field_reference as cfr
from tests import smooth3d_reference as R
from tests.conftest import ROOT
from tests.test_gpu_stack import T106_SIZES, _t106_cut_files, bent_cuts, cut_meshes
from tests.test_o4h import GOLD
from tests.test_quality3d_cpu import mirrored_cuts
from tests.test_smooth3d_cpu import faces_equal, prescribed_field
from turbomesh_amd import _capi, configs, output, stack, weld
from turbomesh_amd.smoothing import smooth, solver

pytestmark = pytest.mark.gpu

S3_TI, S3_TJ, S3_KCHUNK = 32, 8, 16
ALGORITHMS = ["laplace", "thomas-middlecoff", "prescribed"]

# (ni, nj, nk): ni and nj one below, at and one above the first and the second tile seam; nk = 3 and 4 and around a chunk seam
SHAPES = sorted({(ni, 5, 4) for t in (1, 2) for ni in (t * S3_TI - 1, t * S3_TI, t * S3_TI + 1)}
                | {(6, nj, 3) for t in (1, 2) for nj in (t * S3_TJ - 1, t * S3_TJ, t * S3_TJ + 1)}
                | {(5, 4, nk) for nk in (3, 4, S3_KCHUNK - 1, S3_KCHUNK, S3_KCHUNK + 1, 2 * S3_KCHUNK + 1)}
                | {(S3_TI + 1, S3_TJ + 1, S3_KCHUNK + 1), (3, 67, 3), (70, 35, 9)})


def test_constants_are_the_kernels():
    assert (_capi.S3_TI, _capi.S3_TJ, _capi.S3_KCHUNK) == (S3_TI, S3_TJ, S3_KCHUNK)
    src = open(os.path.join(ROOT, "turbomesh_amd", "csrc", "tm_smooth3d.hip")).read()
    assert f"S3_TI = {S3_TI}, S3_TJ = {S3_TJ}" in src and f"S3_KCHUNK = {S3_KCHUNK}" in src


@functools.lru_cache(maxsize=None)
def block_of(shape):
    """a block with something to smooth: the bent clustered block plus a smooth interior perturbation; shared, never modified"""
    planes = [a.copy() for a in R.bent_clustered3(*shape)]
    nk, nj, ni = planes[0].shape
    k, j, i = np.meshgrid(np.arange(nk), np.arange(nj), np.arange(ni), indexing="ij")
    for c, a in enumerate(planes):
        a[1:-1, 1:-1, 1:-1] += 0.004 * np.sin(1.7 * i + 0.9 * j + 1.3 * k + c)[1:-1, 1:-1, 1:-1]
    field = prescribed_field(planes)
    for a in (*planes, *field):
        a.setflags(write=False)
    return tuple(planes), tuple(field)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_record(d, h):
    n = h.interior
    for k in ("nodes", "interior", "sweeps_done", "frozen", "first_neg", "first_pos", "first_zero_or_nan", "last_neg", "last_pos", "last_zero_or_nan",
              "last_max_node"):
        assert getattr(d, k) == getattr(h, k), (k, d, h)
    assert np.array_equal(bits(np.array([d.last_max_update, *d.control_max])), bits(np.array([h.last_max_update, *h.control_max]))), (d, h)
    for k in ("first_sum_sq", "last_sum_sq"):
        assert abs(getattr(d, k) - getattr(h, k)) <= 2 * max(0, n - 1) * 2.0 ** -53 * getattr(h, k), (k, d, h)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_device_equals_host_twin(shape):
    planes, field = block_of(shape)
    fd, fh = stack.control_of_planes(*planes), stack.control_of_planes(*planes, host=True)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(fd, fh))
    for algorithm in ALGORITHMS:
        control = field if algorithm == "prescribed" else None
        for sweeps in (1, 2, 5):   # both parities of the ping-pong
            d = stack.smooth_planes(*planes, sweeps, algorithm, control=control)
            h = stack.smooth_planes(*planes, sweeps, algorithm, control=control, host=True)
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(d[:3], h[:3])), (algorithm, sweeps)
            same_record(d[3], h[3])
            assert faces_equal(d[:3], planes)
    w = stack.smooth_planes(*planes, 2, "thomas-middlecoff", omega=0.625)
    wh = stack.smooth_planes(*planes, 2, "thomas-middlecoff", omega=0.625, host=True)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(w[:3], wh[:3]))


def test_second_call_gives_the_same_bits():
    planes, _ = block_of((70, 35, 9))
    a = stack.smooth_planes(*planes, 5, "thomas-middlecoff")
    b = stack.smooth_planes(*planes, 5, "thomas-middlecoff")
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a[:3], b[:3]))
    assert a[3] == b[3] and bits(np.array([a[3].first_sum_sq, a[3].last_sum_sq])).tolist() == bits(np.array([b[3].first_sum_sq, b[3].last_sum_sq])).tolist()


def test_edges_on_the_device():
    planes, _ = block_of((5, 4, 3))
    for shape in ((2, 5, 4), (5, 4, 2)):   # no interior node
        p = R.bent_clustered3(*shape)
        d = stack.smooth_planes(*p, 3, "thomas-middlecoff")
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(d[:3], p)) and d[3] == stack.smooth_planes(*p, 3, "thomas-middlecoff", host=True)[3]
    d, h = stack.smooth_planes(*planes, 0, "thomas-middlecoff"), stack.smooth_planes(*planes, 0, "thomas-middlecoff", host=True)
    assert d[3] == h[3] and all(np.array_equal(bits(a), bits(b)) for a, b in zip(d[:3], planes))
    # a NaN node, a block collapsed onto a line, the early stop: the record is the host's
    nan = [a.copy() for a in R.affine_lattice(7, 7, 7)]
    nan[1][3, 3, 3] = np.nan
    k, j, i = np.meshgrid(np.arange(5.0), np.arange(6.0), np.arange(7.0), indexing="ij")
    line = (np.ascontiguousarray(i + j + k), np.zeros(i.shape), np.zeros(i.shape))
    for p, sweeps, tol in ((nan, 1, 0.0), (line, 2, 0.0), (R.noisy_lattice(), 400, 1e-6)):
        d, h = stack.smooth_planes(*p, sweeps, "laplace", tol=tol), stack.smooth_planes(*p, sweeps, "laplace", tol=tol, host=True)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(d[:3], h[:3]))
        assert d[3].sweeps_done == h[3].sweeps_done and d[3].frozen == h[3].frozen and d[3].last_max_node == h[3].last_max_node
        assert bits(np.array([d[3].last_max_update])) == bits(np.array([h[3].last_max_update]))
    with pytest.raises(_capi.TmError) as e:
        stack.smooth_planes(*planes, 1, "laplace", omega=0.0)
    assert e.value.code == _capi.TM_E_ARG
    with pytest.raises(_capi.TmError) as e:
        stack.smooth_planes(*planes, 1, "prescribed")
    assert e.value.code == _capi.TM_E_ARG


@pytest.mark.parametrize("mapping", ["planar", "cylindrical"])
def test_stack_smooth_on_resident_handles(mapping):
    blocks = bent_cuts(33, 31, 3)
    z = [1.0, 1.25, 1.5]
    st = stack.Stack(z, stack.layers_from(z, 7), "cubic", mapping)
    handles = [smooth.Smoother(m, solver.Option.hip(inner=solver.Inner.relax)) for m in cut_meshes(blocks)]

    def exported(h):
        x, y = np.empty(33 * 31), np.empty(33 * 31)
        _capi.check(_capi.lib().tm_smoother_export_soa(h._h, 0, _capi.f64ptr(x), _capi.f64ptr(y), None, None))
        return x, y

    try:
        before = [exported(h) for h in handles]
        stacked = st.block(handles, 0)
        for algorithm, sweeps in (("thomas-middlecoff", 3), ("laplace", 2)):
            got = st.smooth(handles, 0, sweeps, algorithm)
            ref = stack.smooth_planes(*stacked, sweeps, algorithm)
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got[:3], ref[:3]))
            assert got[3] == ref[3] and got[3].sweeps_done == sweeps and faces_equal(got[:3], stacked)
            assert not np.array_equal(got[0], stacked[0])
        after = [exported(h) for h in handles]
        assert all(np.array_equal(bits(a), bits(b)) for p, q in zip(before, after) for a, b in zip(p, q))   # no handle is modified
        # host cuts take the same route in two steps
        meshes = [h._mesh for h in handles]
        two = st.smooth(meshes, 0, 3, "thomas-middlecoff")
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(two[:3], st.smooth(handles, 0, 3, "thomas-middlecoff")[:3]))
        bad = _capi.tm_smooth3d_opt(_capi.TM_S3_LAPLACE, 0, 1, 2.0, 0.0, None, None, None)
        out = [np.empty(stacked[0].shape) for _ in range(3)]
        info = _capi.tm_smooth3d_info()
        arr = (C.c_void_p * 3)(*[h._h for h in handles])
        assert _capi.lib().tm_stack_smoothers_smooth(arr, C.byref(st._opt), 0, C.byref(bad), *[_capi.f64ptr(o) for o in out], C.byref(info)) == _capi.TM_E_ARG
        assert _capi.lib().tm_stack_smoothers_smooth(arr, C.byref(st._opt), 1, C.byref(bad), *[_capi.f64ptr(o) for o in out], C.byref(info)) == _capi.TM_E_ARG
    finally:
        for h in handles:
            h.close()


def test_mirrored_cuts_after_twenty_laplace_sweeps():
    """Clean cuts with inverted hexahedra between them (test_quality3d_cpu.mirrored_cuts on 5 layers).  Whether held faces allow a valid mesh
    there is not known in advance: only the faces and `inverted` not growing are asserted; the report is printed (profiles/smooth3d_parity.txt)."""
    cuts = [cfr.single_block_mesh(b) for b in mirrored_cuts()]
    st = stack.Stack([0.0, 1.0], np.linspace(0.0, 1.0, 5), "linear", "planar")
    before = st.quality(cuts)[0][0]
    assert before.inverted > 0
    planes = st.block(cuts, 0)
    got = st.smooth(cuts, 0, 20, "laplace")
    after = stack.quality_of_planes(*got[:3])
    print(f"smooth3d_parity: mirrored cuts, 5 layers: inverted {before.inverted} -> {after.inverted} after 20 Laplace sweeps, "
          f"min scaled jacobian {before.min_scaled_jacobian:.4f} -> {after.min_scaled_jacobian:.4f}; {got[3].line('record')}")
    assert faces_equal(got[:3], planes) and after.inverted <= before.inverted


def test_weld_after_smoothing():
    cuts = [configs.strip(2, 17, 13), configs.strip(2, 17, 13)]
    for c, m in enumerate(cuts):
        for b in m.blocks:
            d = b.points.data
            d[1:-1, 1:-1] += 0.004 * (1 + c) * np.sin(31.0 * np.arange(d[1:-1, 1:-1].size)).reshape(d[1:-1, 1:-1].shape)
    st = stack.Stack([0.0, 1.0], stack.layers_from([0.0, 1.0], 4), "linear", "planar")
    m3 = st.mesh3d(cuts)
    plain = weld.Weld(cuts[0]).mesh(m3)
    nodes_out, max_gap = plain.info.nodes_out, plain.info.max_gap
    unsmoothed = [tuple(a.copy() for a in blk) for blk in m3.blocks]
    records = m3.smooth(3, "thomas-middlecoff")
    assert all(r.sweeps_done == 3 and r.last_max_update > 0 for r in records)
    assert all(faces_equal(a, b) for a, b in zip(m3.blocks, unsmoothed))
    smoothed = weld.Weld(cuts[0]).mesh(m3)
    assert smoothed.info.nodes_out == nodes_out and bits(np.array([smoothed.info.max_gap])) == bits(np.array([max_gap]))
    assert not np.array_equal(smoothed.points, plain.points)


def test_cli_smooths_three_t106_cuts(tmp_path):
    files = _t106_cut_files(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT)
    base = [sys.executable, "-m", "turbomesh_amd", files[0], "--hip", "--iterations", "1", "--stack", files[1], files[2], "--span", "0,0.05,0.1", "--layers", "5"]
    plain, out = str(tmp_path / "plain.xyz"), str(tmp_path / "smooth.xyz")
    r0 = subprocess.run(base + ["--output", plain], capture_output=True, text=True, timeout=600, cwd=GOLD, env=env)
    assert r0.returncode == 0, r0.stderr[-3000:]
    r = subprocess.run(base + ["--output", out, "--stack-smooth", "3", "--stack-quality"], capture_output=True, text=True, timeout=600, cwd=GOLD, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "stack total: hexahedra" in r.stderr and "stack-smooth total: hexahedra" in r.stderr   # the report before and after
    assert r.stderr.count("stack-smooth ") >= 2 * len(T106_SIZES) and ": sweeps 3 interior " in r.stderr
    a, b = output.read_plot3d_3d(plain), output.read_plot3d_3d(out)
    assert [(x[0], x[1], x[2]) for x in b] == [(ni, nj, 5) for ni, nj in T106_SIZES]
    for p, q in zip(a, b):
        assert faces_equal(q[3:], p[3:])
    assert any(not np.array_equal(p[3], q[3]) for p, q in zip(a, b))


def test_cpp_mirror_smooths_a_stack():
    exe = os.path.join(ROOT, "turbomesh_amd", "tm_harness")
    r = subprocess.run([exe, "stack-smooth", "33", "25", "17", "3"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "stack-smooth: device equals host: yes" in r.stdout and "stack-smooth: faces held: yes" in r.stdout
    assert "interior 10695 sweeps 3" in r.stdout
