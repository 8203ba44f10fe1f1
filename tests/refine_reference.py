"""The yardstick of the refinement tests (TM_OPT_REFINE, tm_csr_residual, tm_smoother_residual), plain numpy / scipy / fractions.

    residual_exact   b - A x of a CSR system as exact rationals (fp64 inputs make every product and sum exact), rounded once
    residual_ld      the same in numpy.longdouble, for whole meshes (pinned against residual_exact in tests/test_refine_reference_cpu.py)
    lu_refined       sparse LU + iterative refinement with the longdouble residual until the update is below one ulp of the solution:
                     the exact solution rounded to fp64, to within an ulp, whatever the elimination order
    picard_refined   the exact Picard iteration of oracle.picard_exact with lu_refined in place of the plain LU solve

Shared by tests/test_refine_reference_cpu.py, tests/test_gpu_refine.py and tools/refine_timing.py."""
from fractions import Fraction

import numpy as np

from oracle import oracle

EPS = 2.0 ** -52


def residual_exact(p, i, v, x, b, rows=None):
    """-> (r, s): r[k] = b - sum_j a_kj x_j of row rows[k] (all rows by default) in exact rational arithmetic, rounded once to fp64 (float() of
    a Fraction rounds correctly); s[k] = sum_j |a_kj x_j| + |b_k|, the scale the error bounds of a computed residual are relative to."""
    rows = range(len(p) - 1) if rows is None else rows
    r, s = np.empty(len(rows)), np.empty(len(rows))
    for k, row in enumerate(rows):
        acc = Fraction(float(b[row]))
        mag = abs(acc)
        for q in range(p[row], p[row + 1]):
            t = Fraction(float(v[q])) * Fraction(float(x[i[q]]))
            acc -= t
            mag += abs(t)
        r[k] = float(acc)
        s[k] = float(mag)
    return r, s


def residual_ld(p, i, v, x, b):
    """b - A x with products and sums in numpy.longdouble (64-bit significand on x86-64), rounded to fp64 at the end."""
    p = np.asarray(p)
    prod = np.asarray(v, dtype=np.longdouble) * np.asarray(x, dtype=np.longdouble)[np.asarray(i)]
    row = np.repeat(np.arange(len(p) - 1), np.diff(p))
    acc = np.asarray(b, dtype=np.longdouble).copy()
    np.subtract.at(acc, row, prod)   # in CSR order within a row
    return np.asarray(acc, dtype=np.float64)


def lu_refined(A, b, permc_spec="COLAMD", max_steps=10):
    """-> (x, steps): A x = b by splu, refined with the longdouble residual until max|d| <= 2^-53 max|x| (an update that no longer changes
    the leading digits of x) or max_steps."""
    import scipy.sparse.linalg as spla

    A = A.tocsr()
    A.sort_indices()
    lu = spla.splu(A.tocsc(), permc_spec=permc_spec)
    x = lu.solve(np.asarray(b, dtype=np.float64))
    steps = 0
    for steps in range(1, max_steps + 1):
        d = lu.solve(residual_ld(A.indptr, A.indices, A.data, x, b))
        x = x + d
        if np.abs(d).max() <= 0.5 * EPS * np.abs(x).max():
            break
    return x, steps


def picard_refined(mesh, iterations, control=None, permc_spec="COLAMD"):
    """oracle.picard_exact with every solve refined (lu_refined).  Mutates mesh.blocks in place; -> list of the iterates, each (dof, 2)."""
    s = oracle.System(mesh, control)
    iterates = []
    for n in range(iterations):
        s.fill(n)
        s.fill_x_specific()
        x, _ = lu_refined(s.csr(), s.rhs_x.copy(), permc_spec)
        s.fill_y_specific()
        y, _ = lu_refined(s.csr(), s.rhs_y.copy(), permc_spec)
        s.x_new[:] = x
        s.y_new[:] = y
        s.commit()
        iterates.append(np.concatenate([b.reshape(-1, 2) for b in mesh.blocks], axis=0).copy())
    s.close()
    return iterates


def system_of(mesh, control=None):
    """The oracle-assembled system of a mesh's coordinates at outer iteration 0: (Ap, Ai, Ax_x, Ax_y, bx, by) as copies."""
    s = oracle.System(mesh, control)
    s.fill(0)
    s.fill_x_specific()
    p, i, vx = np.array(s.lhs_p, dtype=np.int32), np.array(s.lhs_i, dtype=np.int32), s.lhs_values.copy()
    s.fill_y_specific()
    vy = s.lhs_values.copy()
    bx, by = s.rhs_x.copy(), s.rhs_y.copy()
    s.close()
    return p, i, vx, vy, bx, by
