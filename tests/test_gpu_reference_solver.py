"""TM_INNER_REFERENCE_GMRES on the device: the reference's route as its example inputs write it -- per outer iteration the assembled, unscaled
system, GMRES(30) left-preconditioned with ILU(0) (or the diagonal), the stop test ||M^-1 (b - A x)|| <= max(1e-8, 1e-6 ||b||) -- against the
FAITHFUL oracle stepped the same way (tests/reference_yardstick.py).

The device and the oracle share the matrix, the mat-vec and M^-1 bit for bit; they differ in the summation order of every dot product and
norm.  How far that may move an iterate is measured on the reference itself: the bound for iterate k is max(1e-10, 3 * self_k(u)), self_k(u)
the oracle's distance from its own run started u = round(sqrt(dof)) ulps away (reference_yardstick).  Every figure is printed before it is
asserted (pytest -s); tools/reference_solve_parity.py writes them to profiles/reference_solve_parity.txt."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle
from tests import reference_yardstick as ry
from tests.conftest import OracleMesh, mesh_flat
from tests.meshes import TOPOLOGIES
from tests.test_gpu_ilu0 import device_ilu0
from turbomesh_amd import _capi
from turbomesh_amd.smoothing import smooth, solver, wall_control_function as wcf

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ILU0, DIAGONAL = solver.Preconditioner.ilu0, solver.Preconditioner.diagonal
ORACLE_PC = {ILU0: oracle.PRECOND_ILU0, DIAGONAL: oracle.PRECOND_DIAGONAL}


def option(pc=ILU0, **kw):
    return solver.Option.hip(inner=solver.Inner.reference_gmres, preconditioner=pc, **kw)


def algorithm(control):
    return None if control is None else wcf.Algorithm(wcf.White(control[1], control[2]))


def dof_of(mesh):
    return sum(b.points.data.shape[0] * b.points.data.shape[1] for b in mesh.blocks)


def device_run(mesh, control, iters, pc=ILU0):
    """one iterate(1) at a time -> per outer iteration: (x, y) counts, coordinates, stats"""
    out = []
    with smooth.Smoother(mesh, option(pc), algorithm(control)) as sm:
        assert sm.inner == solver.Inner.reference_gmres
        for _ in range(iters):
            st = sm.iterate(1)
            sm.download()
            out.append((sm.inner_counts(), mesh_flat(mesh).copy(), st))
    return out


def compare(name, pc=ILU0):
    """-> number of solves whose count differs from the oracle's; asserts everything else of test A for one case"""
    mesh, control, iters = ry.case(name, None)          # TFI on the device: bit-identical to the oracle's (tests/test_o4h.py, test_gpu_tfi.py)
    ref_mesh, _, _ = ry.case(name)
    assert all(a.points.data.tobytes() == b.points.data.tobytes() for a, b in zip(mesh.blocks, ref_mesh.blocks))
    base = ry.run(OracleMesh(ref_mesh), iters, oracle.SOLVER_GMRES, ORACLE_PC[pc], control)
    u = ry.ulps_of(dof_of(ref_mesh))
    _, self_k = ry.self_distance(ref_mesh, control, iters, u, pc=ORACLE_PC[pc], base=base)
    bound = ry.bounds(self_k)
    dev = device_run(mesh, control, iters, pc)
    differing, first_differing = 0, None
    for k, ((cx, cy), xy, st) in enumerate(dev):
        d_k = ry.rms(xy, base[1][k])
        print(f"{name} [{pc.name}] k={k}: counts device {cx}+{cy}={cx + cy} oracle {base[0][k]}; d_k {d_k:.3e} bound {bound[k]:.3e} (self_k({u}) {self_k[k]:.3e}); "
              f"residual device {st['last_residual']:.9e} oracle {base[2][k]:.9e}")
        assert st["not_converged"] == 0 and st["outer_iterations"] == 1 and st["inner_iterations"] == cx + cy
        if cx + cy != base[0][k]:
            differing += 1
            assert name not in ry.EXAMPLES, f"{name}: solve {k} took {cx + cy} inner iterations, the reference {base[0][k]}"
            assert abs(cx + cy - base[0][k]) <= 1, f"{name}: solve {k} differs by more than one column: {cx + cy} against {base[0][k]}"
            if first_differing is None:
                first_differing = k
        if first_differing is None:   # one column more or less moves the solution by O(tol): the coordinate bound holds up to the first differing solve
            assert d_k <= bound[k], f"{name}: iterate {k} is {d_k:.3e} RMS from the faithful oracle's, bound {bound[k]:.3e}"
            assert st["last_residual"] == pytest.approx(base[2][k], rel=1e-6), (name, k)
    return differing


@pytest.mark.parametrize("name", ry.EXAMPLES)
def test_a_example_inputs_as_written(name):
    # T106 / LS89, 10 iterations, White, GMRES(30) + ILU(0): the counts of all ten solves equal the reference's, every iterate within the bound
    assert compare(name) == 0


def test_a_topologies_ilu0():
    # the ten test topologies, 3 iterations, Laplace.  Over all 50 solves of the set (20 of them on the examples, where none may differ) at
    # most 10 % may differ from the oracle's count, by one column at most
    differing = sum(compare(name) for name in TOPOLOGIES)
    assert differing <= 5, differing


def test_a_topologies_diagonal():
    # the same with the reference's diagonal preconditioner, z_i = r_i * (1 / a_ii).  Not on T106: the faithful GMRES + diagonal run is itself
    # unstable there (its counts change under a perturbation of one ulp from iteration 5 on, self-distance 5e-7), so there is no yardstick
    differing = sum(compare(name, DIAGONAL) for name in TOPOLOGIES)
    assert differing <= 3, differing   # 10 % of its 30 solves


@pytest.mark.parametrize("name", ["T106", "strip2_40x300"])
def test_b_it_is_the_reference_route_not_the_exact_one(name):
    mesh, control, iters = ry.case(name, None)
    faithful, exact = OracleMesh(mesh), OracleMesh(mesh)
    ry.run(faithful, iters, oracle.SOLVER_GMRES, oracle.PRECOND_ILU0, control)
    oracle.picard_exact(exact, iters, control=control)
    xy = device_run(mesh, control, iters)[-1][1]
    to_faithful, faithful_to_exact = ry.rms(xy, faithful.flat()), ry.rms(faithful.flat(), exact.flat())
    print(f"{name}: device to faithful oracle {to_faithful:.3e}, faithful oracle to exact-solve oracle {faithful_to_exact:.3e}")
    assert 100.0 * to_faithful <= faithful_to_exact


def test_c_seam_1_equals_the_handle_bit_for_bit():
    a, b = TOPOLOGIES["channel_periodic_sliding"](None), TOPOLOGIES["channel_periodic_sliding"](None)
    st = smooth.mesh(a, 3, option())
    with smooth.Smoother(b, option()) as sm:
        for _ in range(3):
            sm.iterate(1)
        sm.download()
    assert st["outer_iterations"] == 3 and st["not_converged"] == 0 and st["inner_iterations"] > 0
    assert mesh_flat(a).tobytes() == mesh_flat(b).tobytes()


def test_c_iterate_until_update_stops_where_the_oracle_does():
    mesh = TOPOLOGIES["single_perturbed_33"](None)
    om = OracleMesh(mesh)
    s = oracle.System(om)
    steps = 0
    while steps < 50:   # the oracle stepped the same way: an outer iteration, then the test on its update
        s.fill(steps)
        s.solve(oracle.SOLVER_GMRES, oracle.PRECOND_ILU0)
        _, dx2, dy2 = s.commit()
        steps += 1
        if np.sqrt((dx2 + dy2) / s.dof) <= 1e-6:
            break
    s.close()
    with smooth.Smoother(mesh, option()) as sm:
        reached, st = sm.iterate_until_update(1e-6, 50)
        print(f"single_perturbed_33: device {st['outer_iterations']} outer iterations, oracle {steps}; last update {np.sqrt((st['last_dx2'] + st['last_dy2']) / sm.dof):.3e}, "
              f"last counts {sm.inner_counts()}")
        assert reached and st["outer_iterations"] == steps == 7


def test_c_rank_hooks_are_refused():
    mesh = TOPOLOGIES["strip3_9x12"](None)
    owner = (C.c_int32 * len(mesh.blocks))()
    hooks = _capi.tm_comm_hooks(None, 0, 1, owner, _capi.EXCHANGE_FN(lambda *a: 0), _capi.ALLREDUCE_FN(lambda *a: 0), _capi.EXCHANGE_WAIT_FN(), None, 0)
    with pytest.raises(_capi.TmError) as e:
        smooth.Smoother(mesh, option(), hooks=hooks)
    assert e.value.code == _capi.TM_E_UNSUPPORTED
    md, opt, cf, n = _capi.MeshDesc(mesh), option().c_struct(), wcf.Algorithm.laplace().c_struct(), C.c_uint64(0)
    assert _capi.lib().tm_smoother_workspace_bytes(md.ref(), C.byref(opt), C.byref(cf), C.byref(hooks), C.byref(n)) == _capi.TM_E_UNSUPPORTED


def test_c_the_iteration_cap_is_a_warning():
    mesh = TOPOLOGIES["single_perturbed_33"](None)
    with smooth.Smoother(mesh, option(max_inner=2)) as sm:
        st = sm.iterate(2)   # no exception: GMRES.zig:422 only warns
        assert st["not_converged"] > 0 and max(sm.inner_counts()) == 2
        sm.download()
    assert np.isfinite(mesh_flat(mesh)).all()


def test_c_inner_counts_of_the_other_modes():
    mesh = TOPOLOGIES["single_perturbed_33"](None)
    with smooth.Smoother(mesh, solver.Option.hip(inner=solver.Inner.bicgstab)) as sm:
        st = sm.iterate(1)
        x, y = sm.inner_counts()
        assert x == y == st["inner_iterations"] > 0
    with smooth.Smoother(mesh, solver.Option.hip(inner=solver.Inner.relax)) as sm:
        sm.iterate(2)
        assert sm.inner_counts() == (0, 0)


def test_d_cli_runs_the_t106_input_as_written(tmp_path):
    from turbomesh_amd import output

    cfg = os.path.join("examples", "T106", "T106.json")
    env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = str(tmp_path / "t106_reference.xyz")
    r = subprocess.run([sys.executable, "-m", "turbomesh_amd", cfg, "--hip", "reference", "--iterations", "2", "--output", out], capture_output=True, text=True,
                       timeout=600, cwd=GOLD, env=env)
    assert r.returncode == 0, r.stderr
    assert "inner strategy: reference_gmres" in r.stderr and "preconditioner: ilu0" in r.stderr, r.stderr[-2000:]
    mesh, control, _ = ry.case("T106", None)
    with smooth.Smoother(mesh, option(), algorithm(control)) as sm:
        sm.iterate(2)
        sm.download()
    mine = str(tmp_path / "t106_handle.xyz")
    mesh.write(mine)
    for a, b in zip(output.read_plot3d(out), output.read_plot3d(mine)):
        assert (a[0], a[1]) == (b[0], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


@pytest.mark.parametrize("name", ry.EXAMPLES)
def test_e_packed_substitutions_on_the_example_systems(name):
    # 25 k - 50 k rows, 2000+ levels of ~10 rows: where fetching a level ahead can go wrong.  Factor and M^-1 r bit for bit, x- and y-system
    mesh, control, _ = ry.case(name)
    s = oracle.System(OracleMesh(mesh), control)
    s.fill(0)
    for fill in (s.fill_x_specific, s.fill_y_specific):
        fill()
        p, ci, v = s.lhs_p.copy(), s.lhs_i.copy(), s.lhs_values.copy()
        rhs = np.random.default_rng(7).standard_normal(len(p) - 1)
        lu_ref, z_ref = oracle.csr_ilu0(len(p) - 1, p, ci, v, rhs)
        lu, z = device_ilu0(p, ci, v, rhs)
        assert np.array_equal(lu, lu_ref), f"{name}: factor differs in {np.count_nonzero(lu != lu_ref)} of {len(lu)} entries"
        assert np.array_equal(z, z_ref), f"{name}: M^-1 r differs in {np.count_nonzero(z != z_ref)} of {len(z)} rows, max {np.abs(z - z_ref).max():.2e}"
        assert np.isfinite(z).all()
    s.close()
