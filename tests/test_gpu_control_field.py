"""GPU: the Thomas-Middlecoff and the prescribed control field through the C ABI.

1. the field itself against the longdouble reference (tests/control_field_reference.py), node by node, within
   16 eps x (the term-wise absolute variant) + eps |reference|;
2. the separable clustered rectangle is a fixed point under the field in every inner mode (and not under Laplace);
3. every Picard iterate within the project's flat 1e-10 RMS of oracle.picard_exact holding the same field;
4. the assembled system with a prescribed field bit-identical to the oracle's;
5. the entry points: set / get, update, upload, the error codes, the command line;
6. ranks: the reversed 3-strip over three virtual ranks, bit-identical to one handle.

Measured figures (MI355X) are in profiles/control_field_parity.txt."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle
from tests import control_field_reference as cfr
from tests.conftest import OracleMesh, mesh_flat
from turbomesh_amd import _capi, configs
from turbomesh_amd.smoothing import smooth, solver, wall_control_function as wcf

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TM = wcf.Algorithm.thomas_middlecoff
INNER = {"bicgstab": solver.Inner.bicgstab, "mg_bicgstab": solver.Inner.mg_bicgstab, "gmres": solver.Inner.gmres, "relax": solver.Inner.relax}


def _blocks(mesh):
    return [b.points.data for b in mesh.blocks]


def _rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a) - np.asarray(b)) ** 2)))


def _t106():
    from turbomesh_amd.input import Input

    inp = Input.parse(open(os.path.join(GOLD, "examples", "T106", "T106.json")).read())
    return inp.template.run(inp.geometry(GOLD))


def _smooth_random_field(mesh, seed):
    """Per block a few low Fourier modes with random coefficients, scaled to max |P|, |Q| = 0.5 (1 +- P/2 stay positive): smooth, and
    nothing the Thomas-Middlecoff evaluation would produce (it differs on the two sides of every interface)."""
    rng = np.random.default_rng(seed)
    fields = []
    for b in mesh.blocks:
        ni, nj = b.points.size
        u, v = np.linspace(0.0, 1.0, ni)[:, None], np.linspace(0.0, 1.0, nj)[None, :]
        f = np.zeros((ni, nj, 2))
        for c in range(2):
            for k in range(3):
                for l in range(3):
                    a, p, q = rng.standard_normal(), rng.uniform(0, 2 * np.pi), rng.uniform(0, 2 * np.pi)
                    f[..., c] += a * np.cos(np.pi * k * u + p) * np.cos(np.pi * l * v + q)
            f[..., c] *= 0.5 / np.abs(f[..., c]).max()
        fields.append(f)
    return fields


# ------------------------------------------------------------------ 1. the field
FIELD_MESHES = {
    "3x3": lambda: cfr.single_block_mesh(cfr.bent_clustered(3, 3)),        # one interior node: both ends copy the single interior edge point
    "3x9": lambda: cfr.single_block_mesh(cfr.bent_clustered(3, 9)),
    "9x3": lambda: cfr.single_block_mesh(cfr.bent_clustered(9, 3)),
    "4x5": lambda: cfr.single_block_mesh(cfr.bent_clustered(4, 5)),
    "33x25": lambda: cfr.single_block_mesh(cfr.rectangle(33, 25, bend=cfr.BEND)),
    "67x130": lambda: cfr.single_block_mesh(cfr.bent_clustered(67, 130)),   # rows that straddle a 64-lane wave and a workgroup of the blend
    "130x67": lambda: cfr.single_block_mesh(cfr.bent_clustered(130, 67, seed=1)),
    "two_by_two_9": lambda: configs.two_by_two(9),                           # the block table: four blocks, three blocks of two shapes
    "strip3_reversed": lambda: configs.strip(3, 17, 13, reverse_odd=True),
}


@pytest.mark.parametrize("name", list(FIELD_MESHES))
def test_field_equals_the_longdouble_reference(name):
    mesh = FIELD_MESHES[name]()
    with smooth.Smoother(mesh, solver.Option.hip(), TM()) as sm:
        dev = sm.control_function()
    worst = cfr.check_against_reference(dev, _blocks(mesh))
    ref = cfr.mesh_field(_blocks(mesh))
    print(f"{name}: max |P| {float(np.abs(ref[:, 0]).max()):.3f} max |Q| {float(np.abs(ref[:, 1]).max()):.3f}, worst |dev - ref| / bar {worst:.3f}")
    assert np.isfinite(dev).all()
    assert worst <= 1.0, (name, worst)
    assert np.abs(dev).max() > 0


def test_field_is_finite_and_zero_at_coincident_edge_points():
    r = cfr.bent_clustered(9, 7)
    r[0, 4] = r[0, 2]          # the neighbours of edge point k = 3 of the i = 0 edge coincide: d1 = 0 there
    r[5, 0] = r[3, 0]          # ... and those of k = 4 of the j = 0 edge
    mesh = cfr.single_block_mesh(r)
    with smooth.Smoother(mesh, solver.Option.hip(), TM()) as sm:
        dev = sm.control_function().reshape(9, 7, 2)
    assert np.isfinite(dev).all()
    assert dev[0, 3, 1] == 0.0 and dev[4, 0, 0] == 0.0     # psi_lo[3] at s = 0, phi_lo[4] at t = 0
    assert cfr.check_against_reference(dev.reshape(-1, 2), [r]) <= 1.0


# ------------------------------------------------------------------ 2. analytic pin
@pytest.mark.parametrize("inner", ["bicgstab", "mg_bicgstab", "gmres", "relax"])
def test_separable_rectangle_is_a_fixed_point_under_the_field(inner):
    seed = cfr.rectangle(33, 25, bend=0.0)
    mesh = cfr.single_block_mesh(seed)
    with smooth.Smoother(mesh, solver.Option.hip(inner=INNER[inner]), TM()) as sm:
        st = sm.iterate(200 if inner == "relax" else 5)
        sm.download()
    moved = _rms(mesh.blocks[0].points.data, seed)
    print(f"separable 33 x 25 rectangle under the field, {inner}, {st['outer_iterations']} outer iterations: moved {moved:.3e} rms")
    assert moved <= 1e-12, (inner, moved)


def test_separable_rectangle_moves_under_laplace():
    seed = cfr.rectangle(33, 25, bend=0.0)
    mesh = cfr.single_block_mesh(seed)
    smooth.mesh(mesh, 5, solver.Option.hip())
    moved = _rms(mesh.blocks[0].points.data, seed)
    print(f"... under laplace, bicgstab, 5 outer iterations: moved {moved:.3e} rms")
    assert moved > 1e-2


def test_one_shot_call_takes_the_field():
    # tm_smooth_mesh with the kind: the bent rectangle keeps its wall spacing (laplace loses it more than tenfold at mid-chord)
    seed = cfr.rectangle(33, 25, bend=cfr.BEND)
    mesh = cfr.single_block_mesh(seed)
    smooth.mesh(mesh, 12, solver.Option.hip(), TM())
    ratio = cfr.first_cell_height_ratio(mesh.blocks[0].points.data, seed)
    assert ratio.min() >= 0.8 and ratio.max() <= 1.1, (ratio.min(), ratio.max())
    mesh = cfr.single_block_mesh(seed)
    smooth.mesh(mesh, 12, solver.Option.hip())
    assert cfr.first_cell_height_ratio(mesh.blocks[0].points.data, seed)[15] > 10


# ------------------------------------------------------------------ 3. Picard parity
PARITY_MESHES = {
    "bent_rectangle": lambda: cfr.single_block_mesh(cfr.rectangle(33, 25, bend=cfr.BEND)),
    "two_by_two_17": lambda: configs.two_by_two(17),
    "channel_33x17_sliding": lambda: configs.periodic_channel(33, 17),
    "strip3_reversed": lambda: configs.strip(3, 17, 13, reverse_odd=True),
    "T106": _t106,
}
ITERATES = 6


@functools.lru_cache(maxsize=None)
def _oracle_iterates(name, prescribed):
    """(seed blocks, field, the oracle's exact Picard iterates holding that field) -- computed once per mesh, shared by the inner modes.
    The field is the DEVICE's (read back from a handle) or the prescribed one: both sides iterate with the same numbers."""
    mesh = PARITY_MESHES[name]()
    seed = [b.copy() for b in _blocks(mesh)]
    if prescribed:
        field = np.concatenate([f.reshape(-1, 2) for f in _smooth_random_field(mesh, 7)])
    else:
        with smooth.Smoother(mesh, solver.Option.hip(), TM()) as sm:
            field = sm.control_function()
    om = OracleMesh(mesh)
    with cfr.field_in_oracle(field):
        hist, iterates = oracle.picard_exact(om, ITERATES, keep_iterates=True)
    assert all(np.isfinite(b).all() for b in iterates[-1])
    return seed, field, [np.concatenate([b.reshape(-1, 2) for b in it]) for it in iterates]


def _device_iterates(name, inner, algorithm, field=None):
    mesh = PARITY_MESHES[name]()
    out = []
    with smooth.Smoother(mesh, solver.Option.hip(inner=INNER[inner], max_inner=20000), algorithm) as sm:
        if field is not None:
            sm.set_control_function(field)
        for _ in range(ITERATES):
            st = sm.iterate(1)
            assert st["not_converged"] == 0, (name, inner, st)
            sm.download()
            out.append(mesh_flat(mesh).copy())
    return out


@pytest.mark.parametrize("name,inner", [(n, i) for n in PARITY_MESHES for i in ("bicgstab", "gmres")] +
                         [("bent_rectangle", "mg_bicgstab"), ("two_by_two_17", "mg_bicgstab")])
def test_every_picard_iterate_equals_the_exact_oracle_with_the_same_field(name, inner):
    seed, field, ref = _oracle_iterates(name, False)
    got = _device_iterates(name, inner, TM())
    rms = [_rms(g, r) for g, r in zip(got, ref)]
    print(f"{name}, {inner}: rms against the exact iterates {' '.join(f'{v:.1e}' for v in rms)}; max |P|, |Q| {np.abs(field).max(axis=0)}")
    assert max(rms) <= 1e-10, (name, inner, rms)


@pytest.mark.parametrize("name", ["two_by_two_17", "channel_33x17_sliding"])
def test_every_picard_iterate_with_a_prescribed_field(name):
    seed, field, ref = _oracle_iterates(name, True)
    assert np.abs(field).max() <= 0.5
    mesh = PARITY_MESHES[name]()
    shaped, at = [], 0
    for b in mesh.blocks:                       # the front end's per-block form of the same field
        n = b.points.size[0] * b.points.size[1]
        shaped.append(field[at:at + n].reshape(b.points.size[0], b.points.size[1], 2))
        at += n
    got = _device_iterates(name, "bicgstab", wcf.Algorithm.prescribed(shaped))
    rms = [_rms(g, r) for g, r in zip(got, ref)]
    print(f"{name}, prescribed field, bicgstab: rms against the exact iterates {' '.join(f'{v:.1e}' for v in rms)}")
    assert max(rms) <= 1e-10, (name, rms)
    # and it is not the Laplace iteration
    lap = PARITY_MESHES[name]()
    smooth.mesh(lap, ITERATES, solver.Option.hip())
    assert _rms(mesh_flat(lap), ref[-1]) > 1e-4


# ------------------------------------------------------------------ 4. assembled system
def test_assembled_system_with_a_prescribed_field_equals_the_oracle_bit_for_bit():
    mesh = configs.two_by_two(17)
    fields = _smooth_random_field(mesh, 11)
    flat = np.concatenate([f.reshape(-1, 2) for f in fields])
    om = OracleMesh(mesh)
    with cfr.field_in_oracle(flat):
        s = oracle.System(om)
    s.fill(0)
    s.fill_x_specific()
    vx = s.lhs_values.copy()
    s.fill_y_specific()
    vy = s.lhs_values.copy()
    with smooth.Smoother(mesh, solver.Option.hip(), wcf.Algorithm.prescribed(fields)) as sm:
        Ap, Ai, Ax, Ay = sm.assemble_csr()
        rhs = sm.rhs()
    with smooth.Smoother(configs.two_by_two(17), solver.Option.hip()) as lap:
        zero = lap.assemble_csr()[2]
    assert np.array_equal(Ap, s.lhs_p) and np.array_equal(Ai, s.lhs_i)
    assert np.array_equal(Ax, vx), f"{np.count_nonzero(Ax != vx)} of {len(vx)} x-system values differ"
    assert np.array_equal(Ay, vy), f"{np.count_nonzero(Ay != vy)} y-system values differ"
    assert np.array_equal(rhs, np.stack([s.rhs_x, s.rhs_y], axis=1))
    assert not np.array_equal(Ax, zero)        # the field is in the coefficients


# ------------------------------------------------------------------ 5. entry points
def test_set_then_get_is_bit_identical_and_refreshes_the_assembled_system():
    mesh = configs.two_by_two(9)
    fields = _smooth_random_field(mesh, 3)
    flat = np.concatenate([f.reshape(-1, 2) for f in fields])
    with smooth.Smoother(mesh, solver.Option.hip(), wcf.Algorithm.prescribed([np.zeros_like(f) for f in fields])) as sm:
        assert np.array_equal(sm.control_function(), np.zeros((sm.dof, 2)))     # a prescribed handle starts from zero
        before = sm.assemble_csr()[2]
        sm.set_control_function(fields)
        assert np.array_equal(sm.control_function(), flat)
        assert not np.array_equal(sm.assemble_csr()[2], before)
        sm.set_control_function(-flat)                                           # the flat form of the getter
        assert np.array_equal(sm.control_function(), -flat)
    with smooth.Smoother(mesh, solver.Option.hip(), TM()) as sm:                 # allowed on a Thomas-Middlecoff handle: overrides
        evaluated = sm.control_function()
        sm.set_control_function(flat)
        assert np.array_equal(sm.control_function(), flat)
        sm.update_control_function()                                             # ... until the next update
        assert np.array_equal(sm.control_function(), evaluated)


def test_update_evaluates_the_current_coordinates_and_upload_evaluates_the_uploaded_ones():
    # the field is a function of the blocks' EDGES: it changes where they move -- the interfaces of the 2 x 2 mesh
    mesh = configs.two_by_two(17)
    with smooth.Smoother(mesh, solver.Option.hip(), TM()) as sm:
        frozen = sm.control_function()
        assert cfr.check_against_reference(frozen, _blocks(mesh)) <= 1.0
        sm.iterate(3)
        assert np.array_equal(sm.control_function(), frozen)                     # frozen over the outer iterations
        sm.download()
        sm.update_control_function()
        now = sm.control_function()
        assert cfr.check_against_reference(now, _blocks(mesh)) <= 1.0
        assert not np.array_equal(now, frozen)
    # upload: other coordinates in the same arrays
    mesh = cfr.single_block_mesh(cfr.rectangle(33, 25, bend=cfr.BEND))
    with smooth.Smoother(mesh, solver.Option.hip(), TM()) as sm:
        now = sm.control_function()
        mesh.blocks[0].points.data[...] = cfr.bent_clustered(33, 25)
        sm.upload()
        up = sm.control_function()
        assert cfr.check_against_reference(up, _blocks(mesh)) <= 1.0
        assert not np.array_equal(up, now)


def test_error_codes():
    lib = _capi.lib()
    mesh = configs.two_by_two(9)
    md = _capi.MeshDesc(mesh)
    opt = solver.Option.hip().c_struct()
    n = sum(b.points.size[0] * b.points.size[1] for b in mesh.blocks)
    pq = np.zeros((n, 2))

    def create(cf):
        h = C.c_void_p()
        assert lib.tm_smoother_create(md.ref(), C.byref(opt), C.byref(cf), None, None, C.byref(h)) == 0, lib.tm_last_error()
        return h

    h = create(wcf.Algorithm.laplace().c_struct())
    assert lib.tm_smoother_set_control_function(h, _capi.f64ptr(pq)) == _capi.TM_E_UNSUPPORTED
    assert lib.tm_smoother_update_control_function(h) == _capi.TM_E_UNSUPPORTED
    lib.tm_smoother_destroy(h)
    plate = configs.plate(15, 9)                      # a White handle needs the O4H layout
    pmd = _capi.MeshDesc(plate)
    h = C.c_void_p()
    white = wcf.Algorithm(wcf.White(0.02)).c_struct()
    assert lib.tm_smoother_create(pmd.ref(), C.byref(opt), C.byref(white), None, None, C.byref(h)) == 0
    ppq = np.zeros((int(lib.tm_smoother_dof(h)), 2))
    assert lib.tm_smoother_set_control_function(h, _capi.f64ptr(ppq)) == _capi.TM_E_UNSUPPORTED
    assert lib.tm_smoother_update_control_function(h) == _capi.TM_E_UNSUPPORTED
    lib.tm_smoother_destroy(h)
    # prescribed: update is refused, a NaN is refused and leaves the field as it was
    h = create(wcf.Algorithm.prescribed([]).c_struct())
    assert lib.tm_smoother_update_control_function(h) == _capi.TM_E_UNSUPPORTED
    good = np.full((n, 2), 0.25)
    assert lib.tm_smoother_set_control_function(h, _capi.f64ptr(good)) == 0
    for bad_value in (np.nan, np.inf):
        bad = good.copy()
        bad[n // 2, 1] = bad_value
        assert lib.tm_smoother_set_control_function(h, _capi.f64ptr(bad)) == _capi.TM_E_ARG
        back = np.empty((n, 2))
        assert lib.tm_smoother_control_function(h, _capi.f64ptr(back)) == 0
        assert np.array_equal(back, good)
    assert lib.tm_smoother_set_control_function(h, None) == _capi.TM_E_ARG
    lib.tm_smoother_destroy(h)
    # the one-shot call has no way to pass a field
    st = _capi.tm_stats()
    pre = wcf.Algorithm.prescribed([]).c_struct()
    before = mesh_flat(mesh).copy()
    assert lib.tm_smooth_mesh(md.ref(), 1, C.byref(opt), C.byref(pre), C.byref(st)) == _capi.TM_E_ARG
    assert b"prescribed" in lib.tm_last_error() and np.array_equal(mesh_flat(mesh), before)
    # an unknown kind is still an argument error
    unknown = _capi.tm_control_fn(4, 0, 0.0, 0.0)
    assert lib.tm_smoother_create(md.ref(), C.byref(opt), C.byref(unknown), None, None, C.byref(h)) == _capi.TM_E_ARG


def test_workspace_bytes_count_the_field_and_its_scratch():
    lib = _capi.lib()
    mesh = configs.two_by_two(9)
    md = _capi.MeshDesc(mesh)
    opt = solver.Option.hip().c_struct()
    sizes = {}
    for name, algo in (("laplace", wcf.Algorithm.laplace()), ("prescribed", wcf.Algorithm.prescribed([])), ("tm", TM())):
        cf, b = algo.c_struct(), C.c_uint64(0)
        assert lib.tm_smoother_workspace_bytes(md.ref(), C.byref(opt), C.byref(cf), None, C.byref(b)) == 0
        sizes[name] = b.value
    n = sum(b.points.size[0] * b.points.size[1] for b in mesh.blocks)
    edges = sum(2 * (b.points.size[0] + b.points.size[1]) for b in mesh.blocks)
    assert sizes["prescribed"] - sizes["laplace"] >= 16 * n                      # the (P, Q) vector
    assert sizes["tm"] - sizes["prescribed"] >= 8 * edges                        # + 2 (ni + nj) doubles per block (and the block table)


def test_refine_and_reference_modes_run_with_the_field():
    # TM_OPT_REFINE refines against the assembled system, TM_INNER_REFERENCE_GMRES solves it: both hold the field from the first iteration
    seed = cfr.rectangle(33, 25, bend=0.0)
    for opt in (solver.Option.hip(refine=True), solver.Option.hip(inner=solver.Inner.reference_gmres)):
        mesh = cfr.single_block_mesh(seed)
        with smooth.Smoother(mesh, opt, TM()) as sm:
            sm.iterate(3)
            sm.download()
        moved = _rms(mesh.blocks[0].points.data, seed)
        # the separable rectangle is a fixed point; the reference mode stops at its own loose tolerance (1e-6 relative), which the seed meets at once
        assert moved <= 1e-12, (opt, moved)


def test_export_and_write_hand_out_the_field_planes(tmp_path):
    mesh = cfr.single_block_mesh(cfr.bent_clustered(12, 9))
    ni, nj = 12, 9
    with smooth.Smoother(mesh, solver.Option.hip(), TM()) as sm:
        dev = sm.control_function().reshape(ni, nj, 2)
        x, y, p, q = (np.empty(ni * nj) for _ in range(4))
        _capi.check(_capi.lib().tm_smoother_export_soa(sm._h, 0, _capi.f64ptr(x), _capi.f64ptr(y), _capi.f64ptr(p), _capi.f64ptr(q)))
        sm.write(str(tmp_path / "field.xyz"))
    assert np.array_equal(p.reshape(nj, ni).T, dev[..., 0]) and np.array_equal(q.reshape(nj, ni).T, dev[..., 1])
    # the function file beside the grid file: int32 nblocks | (ni, nj, nvar) | P plane | Q plane, i fastest
    raw = open(str(tmp_path / "field.f"), "rb").read()
    assert np.array_equal(np.frombuffer(raw[:16], dtype="<i4"), [1, ni, nj, 2])
    planes = np.frombuffer(raw[16:], dtype="<f8").reshape(2, nj, ni)
    assert np.array_equal(planes[0].T, dev[..., 0]) and np.array_equal(planes[1].T, dev[..., 1])


def test_cli_runs_t106_with_the_field_and_the_quality_report(tmp_path):
    cfg = os.path.join("examples", "T106", "T106.json")
    env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = str(tmp_path / "t106_tm.xyz")
    r = subprocess.run([sys.executable, "-m", "turbomesh_amd", cfg, "--hip", "--control", "thomas-middlecoff", "--quality", "--iterations", "2", "--output", out],
                       capture_output=True, text=True, timeout=300, cwd=GOLD, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "INFO(quality)" in r.stderr and os.path.getsize(out) > 0


def test_host_harness_runs_a_thomas_middlecoff_job():
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "turbomesh_amd", "tm_harness")
    r = subprocess.run([exe, "tm", "33", "25", "5"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "thomas_middlecoff max|P|" in r.stdout


# ------------------------------------------------------------------ 6. ranks
def test_three_virtual_ranks_equal_one_handle_bit_for_bit():
    # the field is block-local and every row reads it at its own node: no halo.  The existing virtual-rank helper takes the control function
    # through its hooks class (HooksBase has the argument); relaxation sweeps are bit-exact across ranks, as with Laplace
    from tests.test_gpu_virtual_ranks import ThreadHooks, _run_ranks

    def builder():
        return configs.strip(3, 17, 13, reverse_odd=True)

    opt = solver.Option.hip(inner=solver.Inner.relax)
    ref = builder()
    smooth.mesh(ref, 25, opt, TM())
    got = _run_ranks(builder, [0, 1, 2], opt, 25, hooks_cls=functools.partial(ThreadHooks, control=TM()))
    assert np.array_equal(mesh_flat(got), mesh_flat(ref))
    lap = builder()
    smooth.mesh(lap, 25, opt)
    assert not np.array_equal(mesh_flat(lap), mesh_flat(ref))
