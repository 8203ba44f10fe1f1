"""Reference for the certificate of high-order hexahedra (include/tm_hip.h, "high-order hexahedra: certificate"), in exact
fractions.Fraction arithmetic and by a route the library does not take:

  * the Jacobian J = Xu . (Xv x Xw) of an element is evaluated at points by exact Lagrange interpolation of its (p+1)^3 fine nodes (no
    Bernstein form involved): `Sampler`;
  * its exact Bernstein coefficients come from its values at 3p points per direction -- J has degree 3p-1 per direction, so these values
    determine it -- converted with the exact Lagrange -> Bernstein matrix of degree 3p-1: `exact_bezier`.  The library instead converts the
    nodes to control points and multiplies Bernstein forms;
  * `children` and `decide` restate the subdivision and the breadth-first verdict; `guard_factor` restates G3(p).

With coordinates on a dyadic grid every quantity is rational, so what is found here owes nothing to rounding.
"""
from fractions import Fraction as Fr
from math import comb

import numpy as np

from tests.ho_certify_reference import _as, _split0, lagrange_rows, lagrange_to_bernstein, norm_inf

PROVEN, INVALID, UNDECIDED = 0, 1, 2


def product_weight(a, b, k, i):
    """w^{a,b}[k][i] = C(a,i) C(b,k-i) / C(a+b,k), 0 outside 0 <= k-i <= b."""
    if not (0 <= i <= a and 0 <= k - i <= b):
        return Fr(0)
    return Fr(comb(a, i) * comb(b, k - i), comb(a + b, k))


def product_weights(a, b):
    return [[product_weight(a, b, k, i) for i in range(a + 1)] for k in range(a + b + 1)]


def weight_pairs(p):
    """The (a, b) of the tables wA and wB in the order the library packs them."""
    return [(p, p), (p - 1, p), (p, p - 1)], [(p - 1, 2 * p), (p, 2 * p - 1)]


def guard_factor(p):
    """G3(p) = 9 p (6p+20) L^3 + 99p + 52, L = ||M||_inf (exact)."""
    lam = norm_inf(p)
    return 9 * p * (6 * p + 20) * lam ** 3 + 99 * p + 52


def apply3(A, B, C, X):
    """Y[a][b][c] = sum A[a][m] B[b][n] C[c][l] X[m][n][l] on object arrays."""
    Y = np.tensordot(A, X, axes=(1, 0))      # (a, n, l)
    Y = np.tensordot(B, Y, axes=(1, 1))      # (b, a, l)
    Y = np.tensordot(C, Y, axes=(1, 2))      # (c, b, a)
    return Y.transpose(2, 1, 0)


class Sampler:
    """Exact J of an element at the tensor grid pts x pts x pts, by Lagrange interpolation.  Xe: (p+1, p+1, p+1, 3), Xe[m, n, l] the fine
    node at (u, v, w) = (m, n, l)."""

    def __init__(self, p, pts):
        self.L, self.dL = lagrange_rows(p, pts)

    def __call__(self, Xe):
        X = _as(Fr, Xe)
        L, dL = self.L, self.dL
        du = [apply3(dL, L, L, X[..., s]) for s in range(3)]
        dv = [apply3(L, dL, L, X[..., s]) for s in range(3)]
        dw = [apply3(L, L, dL, X[..., s]) for s in range(3)]
        return (du[0] * (dv[1] * dw[2] - dw[1] * dv[2]) + du[1] * (dv[2] * dw[0] - dw[2] * dv[0]) + du[2] * (dv[0] * dw[1] - dw[0] * dv[1]))


_CONVERT = {}


def exact_bezier(Xe, p):
    """The exact (3p, 3p, 3p) Bernstein coefficients of J on [0, p]^3."""
    n = 3 * p
    if p not in _CONVERT:
        _CONVERT[p] = (Sampler(p, [Fr(k * p, n - 1) for k in range(n)]), lagrange_to_bernstein(n - 1))
    sampler, M = _CONVERT[p]
    return apply3(M, M, M, sampler(Xe))


def elevate_degree(B2, p):
    """The exact 2-D coefficients B2 (2p, 2p) of a Jacobian that does not depend on w, as (3p, 3p, 3p) coefficients: degree elevation from
    2p-1 to 3p-1 in u and v, constant in w."""
    n2, n3 = 2 * p, 3 * p
    E = np.empty((n3, n2), dtype=object)
    for k in range(n3):
        for i in range(n2):
            E[k, i] = product_weight(n2 - 1, n3 - n2, k, i)    # times the constant 1 of degree p
    flat = E.dot(B2).dot(E.T)
    out = np.empty((n3, n3, n3), dtype=object)
    for c in range(n3):
        out[:, :, c] = flat
    return out


def _split_axis(B, axis, half):
    lo, hi = _split0(np.moveaxis(B, axis, 0).copy(), half)
    return np.moveaxis(lo, 0, axis).copy(), np.moveaxis(hi, 0, axis).copy()


def children(B, half=Fr(1, 2)):
    """The eight children of a patch, child q = (u half) + 2 (v half) + 4 (w half)."""
    out = [None] * 8
    for a, Bu in enumerate(_split_axis(B, 0, half)):
        for b, Bv in enumerate(_split_axis(Bu, 1, half)):
            for c, Bw in enumerate(_split_axis(Bv, 2, half)):
                out[a + 2 * b + 4 * c] = Bw
    return out


def corners(P):
    return [P[a, b, c] for a in (0, -1) for b in (0, -1) for c in (0, -1)]


def decide(B, o, g, max_depth, nodal_valid=True):
    """Breadth first: dict(status, depth, lo, hi)."""
    level = [B * o]
    leaves_lo, leaves_hi = [], []
    for L in range(max_depth + 1):
        invalid, undecided = (L == 0 and not nodal_valid), []
        lo_l, hi_l, plo, phi = [], [], [], []
        for P in level:
            flat = list(P.reshape(-1))
            mn, mx = min(flat), max(flat)
            lo_l.append(mn)
            hi_l.append(mx)
            if any(not (c > 0) for c in corners(P)):
                invalid = True
            elif mn > g:
                plo.append(mn)
                phi.append(mx)
            else:
                undecided.append(P)
        if invalid or not undecided or L == max_depth:
            status = INVALID if invalid else (PROVEN if not undecided else UNDECIDED)
            return dict(status=status, depth=L, lo=min(leaves_lo + lo_l) - g, hi=max(leaves_hi + hi_l) + g)
        leaves_lo += plo
        leaves_hi += phi
        level = [c for P in undecided for c in children(P)]


def element(X, Y, Z, p, e, f, g):
    """(p+1, p+1, p+1, 3) fine nodes of element (e, f, g) of a block given as (nk, nj, ni) planes, indexed [m][n][l]."""
    sl = (slice(g * p, g * p + p + 1), slice(f * p, f * p + p + 1), slice(e * p, e * p + p + 1))
    return np.stack([np.asarray(A)[sl].transpose(2, 1, 0) for A in (X, Y, Z)], axis=-1)


def derivative_extremes(Xe, p):
    """m[q][d]: the largest |derivative coefficient| of component q along direction d, exactly (for R3)."""
    M = lagrange_to_bernstein(p)
    X = _as(Fr, Xe)
    out = []
    for q in range(3):
        C = apply3(M, M, M, X[..., q] - X[0, 0, 0, q])
        out.append([max(abs(v) for v in np.diff(C, axis=d).reshape(-1)) for d in range(3)])
    return out


def guard(Xe, p):
    """g = G3(p) 2^-53 R3 exactly (Fraction)."""
    m = derivative_extremes(Xe, p)
    R3 = sum(m[0]) * sum(m[1]) * sum(m[2])
    return guard_factor(p) * Fr(1, 2 ** 53) * R3, R3, m


def dyadic_block(ni, nj, nk, amplitude, seed, quantum=256, scale=(1.0, 1.0, 1.0)):
    """A unit-cell grid (times `scale` per axis) with uniform perturbations of +-amplitude cells, every coordinate a multiple of
    1/quantum; three (nk, nj, ni) arrays."""
    rng = np.random.default_rng(seed)
    k, j, i = np.meshgrid(np.arange(nk, dtype=np.float64), np.arange(nj, dtype=np.float64), np.arange(ni, dtype=np.float64), indexing="ij")
    out = []
    for base, s in zip((i, j, k), scale):
        out.append(np.round((base + rng.uniform(-amplitude, amplitude, base.shape)) * s * quantum) / quantum)
    return tuple(out)
