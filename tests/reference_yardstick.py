"""The yardstick of the reference-route tests (TM_INNER_REFERENCE_GMRES): the FAITHFUL oracle stepped as the reference's smooth.mesh does
(fill, GMRES(30) + ILU(0) or diagonal with the reference's hard-wired tolerances, commit), and the oracle's distance from ITSELF under a
perturbation of its start coordinates -- how far a re-ordered dot product may move an iterate is a property of the algorithm, so the bound
the device run is held to is measured on the reference, not chosen.

    self_k(u)   RMS distance at iterate k between two oracle runs, the second started from coordinates whose INTERIOR nodes are multiplied
                by 1 + u * 2.2e-16 * s, s in {-1, 0, 1} drawn with numpy.random.default_rng(1), blocks visited in order (perimeter nodes
                untouched: connectionDataCheck compares them at 1e-15)
    u           round(sqrt(dof)): the random-walk size, in ulps, of re-ordering a dof-term sum
    bound_k     max(1e-10, 3 * self_k(u)): 1e-10 RMS is the project's parity bar, the factor 3 the one tests/test_gpu_benchsize.py uses over
                the oracle's distance from itself

Shared by tests/test_reference_solver_cpu.py, tests/test_gpu_reference_solver.py and tools/reference_solve_parity.py."""
import numpy as np

from oracle import oracle
from tests.conftest import OracleMesh, oracle_tfi
from tests.meshes import TOPOLOGIES

PARITY_RMS = 1e-10
FACTOR = 3.0
EXAMPLES = ("T106", "LS89")


def case(name, tfi=oracle_tfi):
    """(mesh, control for the oracle, outer iterations) of a named case: the two example inputs as their JSON writes them (10 iterations,
    White), the ten test topologies (3 iterations, Laplace)."""
    if name in EXAMPLES:
        from tests.test_o4h import load

        inp, mesh = load(name, tfi)
        w = inp.wall_control_function.white
        return mesh, ("white", w.ds_target, w.theta_target), 10
    return TOPOLOGIES[name](tfi), None, 3


def run(om, iters, solver, pc, control):
    """-> (inner count x + y per outer iteration, iterates, commit() residuals); leaves the last iterate in om"""
    s = oracle.System(om, control)
    counts, its, res = [], [], []
    for k in range(iters):
        s.fill(k)
        it, _ = s.solve(solver, pc)
        res.append(s.commit()[0])
        counts.append(it)
        its.append(om.flat().copy())
    s.close()
    return counts, its, res


def perturb(om, rng, u):
    for b in om.blocks:
        inner = b[1:-1, 1:-1, :]
        inner *= 1.0 + u * 2.2e-16 * rng.integers(-1, 2, size=inner.shape)


def rms(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


def ulps_of(dof):
    return int(round(np.sqrt(dof)))


def self_distance(mesh, control, iters, u, pc=oracle.PRECOND_ILU0, base=None):
    """-> (counts of the perturbed run, [self_k(u)]); base = run(...) of the unperturbed mesh if the caller has it already"""
    if base is None:
        base = run(OracleMesh(mesh), iters, oracle.SOLVER_GMRES, pc, control)
    om = OracleMesh(mesh)
    perturb(om, np.random.default_rng(1), u)
    counts, its, _ = run(om, iters, oracle.SOLVER_GMRES, pc, control)
    return counts, [rms(a, b) for a, b in zip(its, base[1])]


def bounds(self_k):
    return [max(PARITY_RMS, FACTOR * s) for s in self_k]
