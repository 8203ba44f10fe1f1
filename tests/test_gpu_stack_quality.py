"""GPU: the 3-D quality report evaluated on the device straight from the cuts (kernel K12, turbomesh_amd/csrc/tm_stack_quality.hip).

The statement under test needs no tolerance: every field of tm_stack_quality equals tm_quality3d_planes_host applied to the planes
tm_stack_block (K11) returned for the same inputs -- the fused kernel sees exactly the block K11 writes.  total_volume alone, a sum that
the device adds in another order, is held within cells * 2^-53 * sum |V|."""
import ctypes as C
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
from tests.test_quality3d_cpu import mirrored_cuts, same_bits
from turbomesh_amd import _capi, configs, stack
from turbomesh_amd.smoothing import smooth, solver

pytestmark = pytest.mark.gpu
HARNESS = os.path.join(ROOT, "turbomesh_amd", "tm_harness")

# tm_stack_quality.hip: a workgroup holds SQ_TILE x SQ_TILE nodes and owns SQ_OWN x SQ_OWN cells; tiles step by SQ_OWN.  A seam lies
# where the cell count of a direction reaches a multiple of SQ_OWN, i.e. at n = m * SQ_OWN + 1 nodes.  There is no blocking of the layers.
SQ_TILE, SQ_OWN = 16, 15
SEAM1, SEAM2 = SQ_OWN + 1, 2 * SQ_OWN + 1


def bent_cuts(ni, nj, K):
    return [cfr.bent_clustered(ni, nj, seed=c) + 0.01 * c for c in range(K)]


def cut_meshes(blocks):
    return [cfr.single_block_mesh(b) for b in blocks]


def volume_bound(X, Y, Z):
    """cells * 2^-53 * sum |V|: the record does not carry sum |V|, so it is taken from the longdouble reference of the same planes."""
    from tests import quality3d_reference as q3r

    r = q3r.report(X, Y, Z)
    return float(r["cells"] * 2.0 ** -53 * r["sum_abs_volume"])


def assert_device_equals_host(st, blocks):
    cuts = cut_meshes(blocks)
    planes = st.block(cuts, 0)                       # K11 on the device
    host = stack.quality_of_planes(*planes)          # the CPU on what K11 wrote
    dev = st.quality(cuts)[0][0]                     # K12 straight from the cuts
    assert same_bits(dev, host, skip=("total_volume",)), (dev, host)
    assert abs(dev.total_volume - host.total_volume) <= volume_bound(*planes)
    return dev, planes


# (ni, nj, K, nk, interpolation, mapping): one cell; ni and nj one below, at and one above the first and the second tile seam; nk = 2, 3 and
# more; K = 2, 3, 8, 16; both interpolations and mappings
CASES = [
    (2, 2, 2, 2, "linear", "planar"),
    (2, 2, 3, 2, "cubic", "cylindrical"),
    (SEAM1 - 1, SEAM1 + 1, 2, 2, "linear", "planar"),
    (SEAM1, SEAM1, 3, 3, "cubic", "cylindrical"),
    (SEAM1 + 1, SEAM1 - 1, 8, 2, "cubic", "planar"),
    (SEAM1, SEAM2 - 1, 16, 3, "cubic", "planar"),
    (SEAM2 + 1, SEAM2, 8, 3, "linear", "cylindrical"),
    (SEAM2 - 1, SEAM2 + 1, 3, 5, "cubic", "planar"),
    (3, 67, 3, 2, "linear", "cylindrical"),
    (70, 35, 16, 9, "cubic", "cylindrical"),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_device_equals_host_bit_for_bit(case):
    ni, nj, K, nk, interpolation, mapping = case
    z = sr.spans(K, "uniform" if mapping == "cylindrical" else "nonuniform")
    s = sr.layers_with_cuts(z, nk, seed=ni + K)
    dev, _ = assert_device_equals_host(stack.Stack(z, s, interpolation, mapping), bent_cuts(ni, nj, K))
    assert dev.cells == (ni - 1) * (nj - 1) * (nk - 1) and sum(dev.hist) == dev.cells - dev.inverted - dev.degenerate


def test_mirrored_cuts_and_repeated_layer():
    blocks = mirrored_cuts()
    ni, nj = blocks[0].shape[:2]
    dev, _ = assert_device_equals_host(stack.Stack([0.0, 1.0], np.linspace(0.0, 1.0, 5), "linear", "planar"), blocks)
    assert dev.orientation == 1 and dev.degenerate == 0 and dev.inverted == 2 * (ni - 1) * (nj - 1)
    blocks = bent_cuts(18, 17, 2)
    dev, _ = assert_device_equals_host(stack.Stack([0.0, 1.0], [0.0, 0.3, 0.3, 0.7, 1.0], "linear"), blocks)
    assert dev.degenerate == 17 * 16 and dev.inverted == 0


def _handles(ni=33, nj=31, K=3):
    meshes = [configs.single_block(ni, nj, amplitude=0.05 + 0.02 * c) for c in range(K)]
    return meshes, [smooth.Smoother(m, solver.Option.hip(inner=solver.Inner.relax)) for m in meshes]


def test_resident_handles_report_and_stay_untouched():
    z = [0.0, 0.4, 1.0]
    st = stack.Stack(z, stack.layers_from(z, 7))
    plain_meshes, plain = _handles()
    watched_meshes, watched = _handles()
    try:
        for h in plain + watched:
            h.iterate(2)
        res = st.quality(watched)                     # ordered behind the sweeps, nothing downloaded
        field = st.quality_field(watched, 0)
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
    # the same report from the coordinates the handles held at the time of the call
    again_meshes, again = _handles()
    try:
        for h in again:
            h.iterate(2)
            h.download()
        up = st.quality(again_meshes)
        assert same_bits(res[0][0], up[0][0]) and same_bits(res[1], up[1])
        assert same_bits(st.quality(again)[0][0], up[0][0])
        planes = st.block(again, 0)
        _, host_field = stack.quality_of_planes(*planes, field=True)
        assert field.tobytes() == host_field.tobytes()
    finally:
        for h in again:
            h.close()


def test_field_of_a_stack_with_inverted_and_degenerate_cells():
    blocks = mirrored_cuts()
    s = [0.0, 0.25, 0.5, 0.5, 0.75, 1.0]              # one repeated layer: a layer of degenerate cells
    st = stack.Stack([0.0, 1.0], s, "linear")
    handles = [smooth.Smoother(m, solver.Option.hip(inner=solver.Inner.relax)) for m in cut_meshes(blocks)]
    try:
        q = st.quality(handles)[0][0]
        f = st.quality_field(handles, 0)
        assert f.shape == (5, blocks[0].shape[1] - 1, blocks[0].shape[0] - 1)
        assert q.degenerate == 12 and q.inverted > 0
        assert int((f <= 0).sum()) == q.inverted and int(np.isnan(f).sum()) == q.degenerate and np.nanmin(f) == q.min_scaled_jacobian
        mid = st.quality_field(handles, 0, 1, 3)      # a window in the middle equals the slice of the whole
        assert mid.tobytes() == f[1:4].tobytes()
        assert st.quality_field(handles, 0, 4).tobytes() == f[4:].tobytes()
    finally:
        for h in handles:
            h.close()


def _quality_rc(handles, z, s, block=0):
    z, s = np.asarray(z, dtype=np.float64), np.asarray(s, dtype=np.float64)
    opt = _capi.tm_stack_opt(z.size, _capi.f64ptr(z), s.size, _capi.f64ptr(s), 1, 0)
    q = _capi.tm_quality3d()
    return _capi.lib().tm_stack_smoothers_quality((C.c_void_p * len(handles))(*handles), C.byref(opt), block, C.byref(q))


def _field_rc(handles, z, s, k_begin, k_count, block=0):
    z, s = np.asarray(z, dtype=np.float64), np.asarray(s, dtype=np.float64)
    opt = _capi.tm_stack_opt(z.size, _capi.f64ptr(z), s.size, _capi.f64ptr(s), 1, 0)
    out = np.empty(s.size * 40 * 40)
    return _capi.lib().tm_stack_smoothers_quality_field((C.c_void_p * len(handles))(*handles), C.byref(opt), block, k_begin, k_count, _capi.f64ptr(out))


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
    z, s = [1.0, 2.0], [1.0, 1.5, 2.0]
    a = smooth.Smoother(cfr.single_block_mesh(cfr.bent_clustered(9, 8)), relax())
    b = smooth.Smoother(cfr.single_block_mesh(cfr.bent_clustered(9, 8, seed=1)), relax())
    other = smooth.Smoother(cfr.single_block_mesh(cfr.bent_clustered(9, 7)), relax())
    whole = smooth.Smoother(configs.strip(2, 9, 8), relax())
    part = NullHooks(configs.strip(2, 9, 8), [0, 1], 0, 2, option=relax())
    dead = smooth.Smoother(cfr.single_block_mesh(cfr.bent_clustered(9, 8)), relax())
    dead_handle = dead._h.value
    dead.close()
    try:
        assert _quality_rc([a._h, b._h], z, s) == _capi.TM_OK
        assert _quality_rc([a._h, other._h], z, s) == _capi.TM_E_SIZE           # unequal sizes between handles
        assert _quality_rc([a._h, whole._h], z, s) == _capi.TM_E_SIZE           # unequal block counts
        assert _quality_rc([a._h, b._h], z, [1.5]) == _capi.TM_E_SIZE           # one layer: no cells
        assert _quality_rc([a._h, b._h], z, s, block=1) == _capi.TM_E_ARG
        assert _quality_rc([a._h, None], z, s) == _capi.TM_E_ARG
        assert _quality_rc([a._h, dead_handle], z, s) == _capi.TM_E_ARG
        assert _quality_rc([whole._h, part.smoother._h], z, s, block=0) == _capi.TM_OK
        assert _quality_rc([whole._h, part.smoother._h], z, s, block=1) == _capi.TM_E_ARG   # a handle that does not own the block
        assert _field_rc([a._h, b._h], z, s, 0, 2) == _capi.TM_OK
        assert _field_rc([a._h, b._h], z, s, 1, 1) == _capi.TM_OK
        assert _field_rc([a._h, b._h], z, s, 1, 2) == _capi.TM_E_ARG            # a window past nlayers - 1
        assert _field_rc([a._h, b._h], z, s, 2, 1) == _capi.TM_E_ARG
        assert _field_rc([a._h, b._h], z, s, 0, 0) == _capi.TM_E_ARG
        assert _field_rc([a._h, other._h], z, s, 0, 1) == _capi.TM_E_SIZE
        with pytest.raises(ValueError):
            stack.Stack(z, s).quality([a, b], host=True)
    finally:
        for h in (a, b, other, whole, part.smoother):
            h.close()


def _t106_cuts(tmp_path):
    """T106 and two copies with the pitch scaled by 1.03 and 1.06: three spanwise cuts of one blade (the construction of the stacking's CLI test)."""
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


def test_cli_reports_on_three_t106_cuts(tmp_path):
    files = _t106_cuts(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT)
    base = [sys.executable, "-m", "turbomesh_amd", files[0], "--hip", "--iterations", "1", "--stack", files[1], files[2], "--span", "0,0.05,0.1", "--layers", "5"]
    plain_out, out = str(tmp_path / "plain.xyz"), str(tmp_path / "blade.xyz")
    plain = subprocess.run(base + ["--output", plain_out], capture_output=True, text=True, timeout=600, cwd=GOLD, env=env)
    assert plain.returncode == 0, plain.stderr[-3000:]
    assert "hexahedra" not in plain.stderr
    r = subprocess.run(base + ["--output", out, "--stack-quality", "--fail-on-inverted-3d"], capture_output=True, text=True, timeout=600, cwd=GOLD, env=env)
    lines = [l for l in r.stderr.splitlines() if l.startswith("INFO(quality): stack ")]
    assert len(lines) == 9 and lines[-1].startswith("INFO(quality): stack total: hexahedra "), r.stderr[-3000:]
    assert open(out, "rb").read() == open(plain_out, "rb").read()      # the file is written either way, and is the same file
    total = lines[-1].split()
    inverted, degenerate = int(total[total.index("inverted") + 1]), int(total[total.index("degenerate") + 1])
    assert int(total[total.index("hexahedra") + 1]) == sum((ni - 1) * (nj - 1) * 4 for ni, nj in
                                                           [(221, 41), (121, 41), (11, 41), (11, 51), (121, 41), (161, 11), (21, 91), (11, 131)])
    if inverted or degenerate:                                         # the exit status follows the record
        assert r.returncode != 0 and "the stacked mesh has" in r.stderr and " k " in r.stderr.splitlines()[-1]
    else:
        assert r.returncode == 0, r.stderr[-3000:]
    # the same cuts wrapped on cylinders of radius 0.01 .. 0.03: theta = y / r turns by radians between neighbouring layers
    twisted = subprocess.run(base[:-4] + ["--span", "0.01,0.02,0.03", "--layers", "5", "--stack-mapping", "cylindrical", "--output", str(tmp_path / "twisted.xyz"),
                                          "--fail-on-inverted-3d"], capture_output=True, text=True, timeout=600, cwd=GOLD, env=env)
    print(f"twisted stack: exit status {twisted.returncode}: {twisted.stderr.splitlines()[-1][:200]}")
    assert os.path.exists(str(tmp_path / "twisted.xyz")) and "INFO(quality): stack " not in twisted.stderr   # written either way; no report asked for
    assert (twisted.returncode != 0) == ("the stacked mesh has" in twisted.stderr)
    # both flags are refused without --stack
    bad = subprocess.run([sys.executable, "-m", "turbomesh_amd", files[0], "--hip", "--stack-quality"], capture_output=True, text=True, timeout=600, cwd=GOLD, env=env)
    assert bad.returncode == 2 and "--stack" in bad.stderr


def test_harness_reports_on_config5_cuts():
    r = subprocess.run([HARNESS, "stack-quality", "33", "25", "3", "7"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "stack-quality: device equals host: yes" in r.stdout
    assert "stack-quality: hexahedra 4608 " in r.stdout


def test_a_users_size_against_the_host():
    # 8 cuts of 1025 x 1025, 9 layers: 8.4 million hexahedra, cell indices beyond 2^23 and byte offsets beyond 2^27
    ni = nj = 1025
    K, nk = 8, 9
    base = cfr.bent_clustered(ni, nj, seed=0)
    rng = np.random.default_rng(7)
    blocks = [base + 0.01 * c + 1e-5 * rng.standard_normal(base.shape) for c in range(K)]
    z = sr.spans(K, "uniform")
    st = stack.Stack(z, stack.layers_from(z, nk), "cubic", "planar")
    cuts = cut_meshes(blocks)
    dev = st.quality(cuts)[0][0]
    host = st.quality(cuts, host=True)[0][0]          # planar: tm_stack_block_host equals the device's planes bit for bit
    assert same_bits(dev, host, skip=("total_volume",)), (dev, host)
    assert dev.cells == 1024 * 1024 * 8
    assert abs(dev.total_volume - host.total_volume) <= dev.cells * 2.0 ** -53 * abs(host.total_volume)   # |sum V| <= sum |V|: no wider than the bar
