"""Reference of the revolution mapping (include/tm_hip.h, "cuts on stream surfaces of revolution") in numpy longdouble, written from
the definition:

    tables_ref(u, x, r, interpolation)        per cut the (N-1, 8) coefficients and their bars; the spline by SOLVING the system
    node_values(blocks, u, coef, rref)        x_c, r_c, theta_c and P_c of every node from the LIBRARY's fp64 coefficients, in longdouble
    surf_ref(blocks, A, u, coef, rref)        (X, Y, Z), (bar_X, bar_Y, bar_Z), R as (nk, nj, ni) longdouble arrays
    outside_ref(blocks, u)                    per cut the number of nodes whose first coordinate lies outside the table

eps = 2^-52.  Bars, as the issue derives them:
    coefficients   4 eps sum_m |L_m| |v_m|, coef = sum_m L_m v_m the coefficient as a linear function of the knot values (one rounding to
                   fp64 is eps/2 of it; long-double accumulation over <= 256 knots lies far below)
    bar_X, bar_R   eps sum_c |A_kc| ((K+1) |x_c| + 8 P_c),  P_c = |a| + |t| (|b| + |t| (|c| + |t| |d|)): K+1 for the sum over the cuts, 8
                   for t and the six operations of the Horner form
    bar_Theta      (K+2) eps sum_c |A_kc| |theta_c|
    bar_Y = bar_Z  bar_R + |R| (bar_Theta + 5 eps), the 5 eps the sincos term of tests/stack_reference.py"""
import numpy as np

from tests import stack_reference as sr

LD = np.longdouble
EPS = sr.EPS


def _linear_maps(u, interpolation):
    """L (N-1, 4, N): the coefficients a, b, c, d of every interval as linear functions of the knot values."""
    z = np.asarray(u, dtype=np.float64).astype(LD)
    N = z.size
    G = sr.second_derivative_map(z) if interpolation == "cubic" and N > 2 else np.zeros((N, N), dtype=LD)
    eye = np.eye(N, dtype=LD)
    L = np.zeros((N - 1, 4, N), dtype=LD)
    for n in range(N - 1):
        h = z[n + 1] - z[n]
        L[n, 0] = eye[n]
        L[n, 1] = (eye[n + 1] - eye[n]) / h - h * (2 * G[n] + G[n + 1]) / 6
        L[n, 2] = G[n] / 2
        L[n, 3] = (G[n + 1] - G[n]) / (6 * h)
    return L


def tables_ref(u, x, r, interpolation):
    """Per cut (coef, bar), both (N-1, 8) longdouble, columns ax bx cx dx ar br cr dr."""
    out = []
    for uc, xc, rc in zip(u, x, r):
        L = _linear_maps(uc, interpolation)
        vx, vr = np.asarray(xc, dtype=np.float64).astype(LD), np.asarray(rc, dtype=np.float64).astype(LD)
        coef = np.concatenate([L @ vx, L @ vr], axis=1)
        bar = 4 * EPS * np.concatenate([np.abs(L) @ np.abs(vx), np.abs(L) @ np.abs(vr)], axis=1)
        out.append((coef, bar))
    return out


def locate(u, un):
    """The largest n <= N-2 with u[n] <= un, 0 when un < u[0]."""
    u = np.asarray(u, dtype=np.float64)
    return np.clip(np.searchsorted(u, un, side="right") - 1, 0, u.size - 2)


def node_values(blocks, u, coef, rref):
    """Per cut, in PLOT3D order (nj, ni): x_c, r_c, theta_c, P_x, P_r -- each (K, nj, ni) longdouble."""
    xs, rs, ths, px, pr = [], [], [], [], []
    for b, uc, cf, rr in zip(blocks, u, coef, rref):
        b = np.asarray(b, dtype=np.float64)
        un, vn = b[..., 0].T, b[..., 1].T
        uc = np.asarray(uc, dtype=np.float64)
        n = locate(uc, un)
        t = un.astype(LD) - uc[n].astype(LD)
        c = np.asarray(cf, dtype=np.float64).astype(LD)[n]   # (nj, ni, 8)
        at = np.abs(t)
        for q, vals, ps in ((0, xs, px), (4, rs, pr)):
            vals.append(c[..., q] + t * (c[..., q + 1] + t * (c[..., q + 2] + t * c[..., q + 3])))
            ps.append(np.abs(c[..., q]) + at * (np.abs(c[..., q + 1]) + at * (np.abs(c[..., q + 2]) + at * np.abs(c[..., q + 3]))))
        ths.append(vn.astype(LD) / LD(np.float64(rr)))
    return tuple(np.stack(a) for a in (xs, rs, ths, px, pr))


def surf_ref(blocks, A, u, coef, rref):
    A = np.asarray(A, dtype=np.float64).astype(LD)
    aA = np.abs(A)
    K = A.shape[1]
    x, r, th, px, pr = node_values(blocks, u, coef, rref)
    sum_ = lambda M, v: np.einsum("kc,cji->kji", M, v)   # noqa: E731
    X, R, T = sum_(A, x), sum_(A, r), sum_(A, th)
    bX = EPS * sum_(aA, (K + 1) * np.abs(x) + 8 * px)
    bR = EPS * sum_(aA, (K + 1) * np.abs(r) + 8 * pr)
    bT = (K + 2) * EPS * sum_(aA, np.abs(th))
    bY = bR + np.abs(R) * (bT + 5 * EPS)
    return (X, R * np.sin(T), R * np.cos(T)), (bX, bY, bY), R, bR


def outside_ref(blocks, u):
    return np.array([int(np.count_nonzero((np.asarray(b)[..., 0] < uc[0]) | (np.asarray(b)[..., 0] > uc[-1]))) for b, uc in zip(blocks, u)], dtype=np.uint64)


# ------------------------------------------------------------------ inputs shared by the CPU and the GPU tests
def rrefs(K):
    return 1.0 + 0.25 * np.arange(K, dtype=np.float64)


def knots(N, seed, lo=-0.6, hi=2.0):
    """N randomly spaced knots over [lo, hi], the ends included."""
    rng = np.random.default_rng(7000 + seed)
    return np.concatenate([[lo], np.sort(rng.uniform(lo, hi, N - 2)), [hi]]) if N > 2 else np.array([lo, hi])


def curves(u, c, rref):
    """The issue's meridional curves on the knots u of cut c."""
    u = np.asarray(u, dtype=np.float64)
    return u + 0.05 * (c + 1) * np.sin(2 * u), rref * (1 + 0.3 * np.tanh(1.5 * (u - 0.5)))


NS = (2, 3, 65, 256)


def tables(K, seed=0, ns=NS):
    """K tables with N mixed from `ns` within the call: (u, x, r, rref), lists of per-cut arrays."""
    rr = rrefs(K)
    u = [knots(ns[(c + seed) % len(ns)], seed + 17 * c) for c in range(K)]
    xr = [curves(u[c], c, rr[c]) for c in range(K)]
    return u, [a for a, _ in xr], [b for _, b in xr], rr
