"""CPU: the yardstick of the refinement tests held against exact arithmetic and against itself (tests/refine_reference.py).

Measured here (container, scipy / SuperLU, x86-64 longdouble):
    residual_ld against exact rationals on sampled rows of the T106 system: at most 0.054 of the bound below (1744 rows)
    picard_refined, COLAMD against MMD_AT_PLUS_A, RMS per iterate: T106 5.3e-12 at iterate 10, at most 6.4e-12 (iterate 8); LS89 at most 1.0e-15"""
import numpy as np
import pytest

from tests import refine_reference as rr
from tests import reference_yardstick as ry
from tests.conftest import OracleMesh


def test_longdouble_residual_against_exact_rationals_on_t106():
    # x = the fp64-rounded LU solution, so that the residual is pure cancellation.  Bound: the final rounding to fp64 (2^-52 |r|, one ulp) and
    # <= 10 longdouble operations of relative error 2^-64 each on terms bounded by s = sum |a x| + |b|: 10 * 2^-64 < 2^-60
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla

    mesh, control, _ = ry.case("T106")
    p, i, vx, _, bx, _ = rr.system_of(OracleMesh(mesh), control)
    n = len(p) - 1
    x = spla.splu(sp.csr_matrix((vx, i, p), shape=(n, n)).tocsc()).solve(bx)
    rows = np.unique(np.concatenate([np.arange(0, n, 17), np.flatnonzero(np.diff(p) != 9)[::5]]))   # every 17th row and a fifth of the perimeter rows
    exact, s = rr.residual_exact(p, i, vx, x, bx, rows)
    got = rr.residual_ld(p, i, vx, x, bx)[rows]
    bound = 2.0 ** -52 * np.abs(exact) + 2.0 ** -60 * s
    worst = float((np.abs(got - exact) / bound).max())
    print(f"[refine yardstick] T106: {len(rows)} rows, worst |ld - exact| / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("name,bar", [("T106", 1e-10), ("LS89", 1e-13)])
def test_two_refined_exact_solvers_agree_over_the_jsons_ten_iterations(name, bar):
    # with a solve that deserves the name "exact" the elimination order no longer shows: the flat 1e-10 bar is reachable on T106
    mesh, control, iters = ry.case(name)
    a = rr.picard_refined(OracleMesh(mesh), iters, control, "COLAMD")
    b = rr.picard_refined(OracleMesh(mesh), iters, control, "MMD_AT_PLUS_A")
    d = [ry.rms(u, v) for u, v in zip(a, b)]
    print(f"[refined self-distance] {name}: " + " ".join(f"{x:.1e}" for x in d))
    assert max(d) <= bar, d
