"""Reference for the high-order certificate (include/tm_hip.h, "high-order elements: certificate"), written from the definition alone and
generic in its number type:

  * fractions.Fraction: exact.  With coordinates on a dyadic grid every quantity is rational, so the status found here is ground truth
    that owes nothing to rounding (guard 0);
  * numpy longdouble (80-bit on x86-64): the definition with its guard, the way ho_reference.py mirrors K13.

The Lagrange -> Bernstein matrix is the exact inverse of the collocation matrix V[m][i] = B_i^p(m/p); the Jacobian is ALSO evaluated
without any Bernstein form (exact Lagrange interpolation at sample points), which is what the coefficient hull is checked against.
"""
from fractions import Fraction as Fr
from math import comb

import numpy as np

LD = np.longdouble
PROVEN, INVALID, UNDECIDED = 0, 1, 2


def _obj(rows):
    a = np.empty((len(rows), len(rows[0])), dtype=object)
    for i, r in enumerate(rows):
        for j, v in enumerate(r):
            a[i, j] = v
    return a


def lagrange_to_bernstein(p):
    """M[i][m] as Fractions: C = M X for the Bernstein coefficients C of the interpolant of X at the nodes m/p.  Gauss-Jordan on the
    collocation matrix V[m][i] = C(p,i) (m/p)^i (1 - m/p)^(p-i)."""
    n = p + 1
    A = [[Fr(comb(p, i) * m ** i * (p - m) ** (p - i), p ** p) for i in range(n)] + [Fr(int(r == m)) for r in range(n)] for m in range(n)]
    for c in range(n):
        piv = next(r for r in range(c, n) if A[r][c] != 0)
        A[c], A[piv] = A[piv], A[c]
        d = A[c][c]
        A[c] = [v / d for v in A[c]]
        for r in range(n):
            if r != c and A[r][c] != 0:
                k = A[r][c]
                A[r] = [v - k * w for v, w in zip(A[r], A[c])]
    return _obj([row[n:] for row in A])


def weights(p):
    """(wu[k][i], wv[l][j]) as Fractions, zero outside 0 <= k-i <= p and 0 <= l-j <= p-1."""
    N = 2 * p
    c = lambda n, k: comb(n, k) if 0 <= k <= n else 0
    wu = _obj([[Fr(c(p - 1, i) * c(p, k - i), comb(N - 1, k)) for i in range(p)] for k in range(N)])
    wv = _obj([[Fr(c(p, j) * c(p - 1, l - j), comb(N - 1, l)) for j in range(p + 1)] for l in range(N)])
    return wu, wv


def norm_inf(p):
    return max(sum(abs(v) for v in row) for row in lagrange_to_bernstein(p))


def guard_factor(p):
    """G(p) = 2 p (4p+14) L^2 + 18p + 4, L = ||M||_inf (exact)."""
    lam = norm_inf(p)
    return 2 * p * (4 * p + 14) * lam * lam + 18 * p + 4


class Tables:
    """The tables of order p in the number type `num` (Fr or LD)."""

    def __init__(self, p, num):
        self.p, self.num = p, num
        conv = (lambda v: v) if num is Fr else (lambda v: LD(v.numerator) / LD(v.denominator))
        self.conv = conv
        to = np.vectorize(conv, otypes=[object])
        self.M = to(lagrange_to_bernstein(p))
        wu, wv = weights(p)
        self.wu, self.wv = to(wu), to(wv)
        self.G = conv(guard_factor(p))
        self.half = Fr(1, 2) if num is Fr else LD(0.5)


def _as(num, X):
    """float array -> object array of `num` (exact for both types)."""
    f = (lambda v: Fr(float(v))) if num is Fr else (lambda v: LD(v))
    return np.vectorize(f, otypes=[object])(np.asarray(X, dtype=np.float64))


def jacobian_bezier(Xe, T):
    """(B, S, R): the (2p, 2p) Bernstein coefficients of the Jacobian of the element with source nodes Xe (p+1, p+1, 2),
    S = max|xu| max|yv| + max|xv| max|yu| and R = (max|xu| + max|xv|) (max|yu| + max|yv|) = S + the cross products; the guard is
    g = G(p) 2^-53 R."""
    p = T.p
    d = _as(T.num, Xe)
    d = d - d[0:1, 0:1, :]
    C = [T.M.dot(d[:, :, s]).dot(T.M.T) for s in range(2)]
    xu, yu = C[0][1:, :] - C[0][:-1, :], C[1][1:, :] - C[1][:-1, :]          # (p, p+1)
    xv, yv = C[0][:, 1:] - C[0][:, :-1], C[1][:, 1:] - C[1][:, :-1]          # (p+1, p)
    N = 2 * p
    B = np.empty((N, N), dtype=object)
    zero = T.conv(Fr(0))
    for k in range(N):
        for l in range(N):
            b = zero
            for i in range(max(0, k - p), min(p - 1, k) + 1):
                s = zero
                for j in range(max(0, l - p + 1), min(p, l) + 1):
                    t = xu[i, j] * yv[k - i, l - j] - yu[i, j] * xv[k - i, l - j]
                    s = s + T.wv[l, j] * t
                b = b + T.wu[k, i] * s
            B[k, l] = b
    mx = lambda a: max(abs(v) for v in a.reshape(-1))
    return B, mx(xu) * mx(yv) + mx(xv) * mx(yu), (mx(xu) + mx(xv)) * (mx(yu) + mx(yv))


def _split0(b, half):
    n = b.shape[0]
    lo, hi = b.copy(), b.copy()
    for r in range(1, n):
        lo[r:] = (lo[r - 1:n - 1] + lo[r:]) * half
        hi[:n - r] = (hi[:n - r] + hi[1:n - r + 1]) * half
    return lo, hi


def children(B, half):
    """The four children of a patch, child 2*qu + qv: split at the midpoint in u (axis 0), then in v."""
    out = []
    for h in _split0(B, half):
        l, r = _split0(h.T.copy(), half)
        out += [l.T.copy(), r.T.copy()]
    return out


def decide(B, o, g, max_depth, nodal_valid=True):
    """Breadth first: dict(status, depth, lo, hi, min_abs) -- min_abs the smallest |coefficient| of any visited patch."""
    level = [B * o]
    leaves_lo, leaves_hi = [], []
    min_abs = None
    for L in range(max_depth + 1):
        invalid, undecided = (L == 0 and not nodal_valid), []
        lo_l, hi_l, plo, phi = [], [], [], []
        for P in level:
            flat = list(P.reshape(-1))
            mn, mx = min(flat), max(flat)
            m_abs = min(abs(v) for v in flat)
            min_abs = m_abs if min_abs is None else min(min_abs, m_abs)
            lo_l.append(mn)
            hi_l.append(mx)
            corners = (P[0, 0], P[0, -1], P[-1, 0], P[-1, -1])
            if any(not (c > 0) for c in corners):
                invalid = True
            elif mn > g:
                plo.append(mn)
                phi.append(mx)
            else:
                undecided.append(P)
        if invalid or not undecided or L == max_depth:
            status = INVALID if invalid else (PROVEN if not undecided else UNDECIDED)
            return dict(status=status, depth=L, lo=min(leaves_lo + lo_l) - g, hi=max(leaves_hi + hi_l) + g, min_abs=min_abs)
        leaves_lo += plo
        leaves_hi += phi
        half = Fr(1, 2) if isinstance(B[0, 0], Fr) else LD(0.5)
        level = [c for P in undecided for c in children(P, half)]


def lagrange_rows(p, pts):
    """(L, dL): exact values and u-derivatives of the Lagrange polynomials of the nodes 0 .. p at the points pts (Fractions), (len, p+1)."""
    L = np.empty((len(pts), p + 1), dtype=object)
    dL = np.empty((len(pts), p + 1), dtype=object)
    for a, u in enumerate(pts):
        for m in range(p + 1):
            t = Fr(1)
            for n in range(p + 1):
                if n != m:
                    t *= (u - n) / Fr(m - n)
            dsum = Fr(0)
            for k in range(p + 1):
                if k == m:
                    continue
                pr = Fr(1, m - k)
                for n in range(p + 1):
                    if n != m and n != k:
                        pr *= (u - n) / Fr(m - n)
                dsum += pr
            L[a, m], dL[a, m] = t, dsum
    return L, dL


class Sampler:
    """Exact J of an element at the tensor grid pts x pts, by Lagrange interpolation (no Bernstein form involved)."""

    def __init__(self, p, pts):
        self.L, self.dL = lagrange_rows(p, pts)

    def __call__(self, Xe):
        X = _as(Fr, Xe)
        xu, yu = (self.dL.dot(X[:, :, s]).dot(self.L.T) for s in range(2))
        xv, yv = (self.L.dot(X[:, :, s]).dot(self.dL.T) for s in range(2))
        return xu * yv - xv * yu


def jacobian_at(Xe, p, u, v):
    """Exact J of the element at the one point (u, v), u, v in [0, p] as Fractions."""
    Lu, dLu = lagrange_rows(p, [u])
    Lv, dLv = lagrange_rows(p, [v])
    X = _as(Fr, Xe)
    xu, yu = (dLu.dot(X[:, :, s]).dot(Lv.T)[0, 0] for s in range(2))
    xv, yv = (Lu.dot(X[:, :, s]).dot(dLv.T)[0, 0] for s in range(2))
    return xu * yv - xv * yu


def dyadic_points(p, n):
    """k p / n, k = 0 .. n."""
    return [Fr(k * p, n) for k in range(n + 1)]


def element(X, p, e, f):
    return np.asarray(X)[e * p:e * p + p + 1, f * p:f * p + p + 1]


def stretched_block(p, ratio, seed, quantum=256):
    """One element of order p with aspect ratio `ratio` (a power of two), long side along (3, 1), short side along (-1, 3), nodes
    displaced by up to 0.05 of the short cell; every coordinate a multiple of 1/quantum.  Thin cells at an angle to the axes: the
    cross products max|xu| max|yu| + max|xv| max|yv| exceed S by the ratio."""
    rng = np.random.default_rng(seed)
    m, n = np.meshgrid(np.arange(p + 1, dtype=np.float64), np.arange(p + 1, dtype=np.float64), indexing="ij")
    X = np.stack([3.0 * ratio * m - n, 1.0 * ratio * m + 3.0 * n], axis=-1) + rng.uniform(-0.05, 0.05, (p + 1, p + 1, 2))
    return np.round(X * quantum) / quantum


def dyadic_block(ni, nj, amplitude, seed, quantum=256):
    """A unit-cell grid with uniform perturbations of +-amplitude cells, every coordinate a multiple of 1/quantum."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(ni, dtype=np.float64), np.arange(nj, dtype=np.float64), indexing="ij")
    X = np.stack([i, j], axis=-1) + rng.uniform(-amplitude, amplitude, (ni, nj, 2))
    return np.round(X * quantum) / quantum
