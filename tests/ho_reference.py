"""Reference for the high-order elevation (include/tm_hip.h, "high-order elements"), written from the definitions alone in numpy
longdouble (80-bit on x86-64): node distributions, the tables T and D, Y = T X T^T per element with its derivatives, the Jacobian, the
element and block records, and the error bars the tests hold the library to.

Bars (u = 2^-53):
  nodes      |Y - Y_ref| <= (2p+6) u sum |T_a| |T_b| |X|: p+1 terms per dot product (p additions and a multiplication each), two nested
             dot products, and the rounding of both tables -- 2(p+1) + 2 roundings along the longest path, rounded up to 2p+6.
  Jacobian   |J - J_ref| <= (4p+16) u (S_xu S_yv + S_xv S_yu), S the absolute-value contraction of that derivative: each factor carries
             (2p+6) u relative to its S, a product two of them plus its own rounding, the difference one more: 2(2p+6) + 2 <= 4p+16.
"""
import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53
PI = LD("3.14159265358979323846264338327950288")


def gauss_lobatto(p):
    """Ascending roots of (1 - x^2) P'_p(x) in longdouble: Newton on (x^2 - 1) P'_p = p (x P_p - P_{p-1}), derivative p (p+1) P_p."""
    x = np.zeros(p + 1, dtype=LD)
    x[0], x[p] = LD(-1), LD(1)
    for a in range(1, p):
        z = -np.cos(PI * LD(a) / LD(p))
        for _ in range(100):
            p0, p1 = LD(1), z
            for k in range(2, p + 1):
                p0, p1 = p1, ((2 * k - 1) * z * p1 - (k - 1) * p0) / k
            dz = (z * p1 - p0) / ((p + 1) * p1)
            z = z - dz
            if abs(dz) <= LD("1e-20"):
                break
        x[a] = z
    return x


def nodes(p, distribution, prescribed=None):
    """The fp64 nodes t_0 = 0 .. t_p = 1."""
    if distribution == "equidistant":
        t = (np.arange(p + 1, dtype=LD) / LD(p)).astype(np.float64)
    elif distribution == "gauss_lobatto":
        t = ((LD(1) + gauss_lobatto(p)) / LD(2)).astype(np.float64)
    else:
        t = np.asarray(prescribed, dtype=np.float64).copy()
    t[0], t[p] = 0.0, 1.0
    return t


def tables(p, distribution, prescribed=None):
    """(T, D) in longdouble, NOT rounded: T[a][m] = prod_{n != m} (u_a - n)/(m - n), D its derivative at u_a; u_a = p t_a, and u_a = a
    exactly for the equidistant distribution."""
    if distribution == "equidistant":
        u = np.arange(p + 1, dtype=LD)
    else:
        u = LD(p) * nodes(p, distribution, prescribed).astype(LD)
    T = np.zeros((p + 1, p + 1), dtype=LD)
    D = np.zeros((p + 1, p + 1), dtype=LD)
    for a in range(p + 1):
        for m in range(p + 1):
            t = LD(1)
            for n in range(p + 1):
                if n != m:
                    t = t * ((u[a] - n) / LD(m - n))
            d = LD(0)
            for k in range(p + 1):
                if k == m:
                    continue
                pr = LD(1) / LD(m - k)
                for n in range(p + 1):
                    if n != m and n != k:
                        pr = pr * ((u[a] - n) / LD(m - n))
                d = d + pr
            T[a, m], D[a, m] = t, d
    return T, D


def elements_of(X, p):
    """(Ei, Ej, p+1, p+1, 2) longdouble: source nodes of every element."""
    ni, nj = X.shape[:2]
    assert (ni - 1) % p == 0 and (nj - 1) % p == 0
    Ei, Ej = (ni - 1) // p, (nj - 1) // p
    i = (np.arange(Ei)[:, None] * p + np.arange(p + 1)[None, :])
    j = (np.arange(Ej)[:, None] * p + np.arange(p + 1)[None, :])
    return X.astype(LD)[i[:, None, :, None], j[None, :, None, :]]


def _contract(A, Xe, B):
    """R[e, f, a, b, c] = sum_m sum_n A[a, m] B[b, n] Xe[e, f, m, n, c]"""
    return np.einsum("am,efmnc,bn->efabc", A, Xe, B)


class Reference:
    """Everything the tests compare against, for one block X (ni, nj, 2) and one elevation."""

    def __init__(self, X, p, distribution, prescribed=None):
        self.p = p
        T, D = tables(p, distribution, prescribed)
        Xe = elements_of(X, p)
        self.Ei, self.Ej = Xe.shape[:2]
        self.Ye = _contract(T, Xe, T)
        du, dv = _contract(D, Xe, T), _contract(T, Xe, D)
        self.J = du[..., 0] * dv[..., 1] - dv[..., 0] * du[..., 1]          # (Ei, Ej, p+1, p+1)
        aT, aD, aX = np.abs(T), np.abs(D), np.abs(Xe)
        self.bar_Ye = (2 * p + 6) * U * _contract(aT, aX, aT)
        s_u, s_v = _contract(aD, aX, aT), _contract(aT, aX, aD)
        self.bar_J = (4 * p + 16) * U * (s_u[..., 0] * s_v[..., 1] + s_v[..., 0] * s_u[..., 1])
        # the structured array: a seam node from the element above it, the last node from the last element
        ni, nj = X.shape[:2]
        self.Y = np.zeros((ni, nj, 2), dtype=LD)
        self.bar_Y = np.zeros((ni, nj, 2), dtype=LD)
        for e in range(self.Ei):
            for f in range(self.Ej):
                na = p + 1 if e == self.Ei - 1 else p
                nb = p + 1 if f == self.Ej - 1 else p
                self.Y[e * p:e * p + na, f * p:f * p + nb] = self.Ye[e, f, :na, :nb]
                self.bar_Y[e * p:e * p + na, f * p:f * p + nb] = self.bar_Ye[e, f, :na, :nb]
        # orientation of the mesh of element corners
        C = X.astype(LD)[::p, ::p]
        A_, B_, C_, D_ = C[:-1, :-1], C[1:, :-1], C[1:, 1:], C[:-1, 1:]
        area = LD(0.5) * ((C_[..., 0] - A_[..., 0]) * (D_[..., 1] - B_[..., 1]) - (D_[..., 0] - B_[..., 0]) * (C_[..., 1] - A_[..., 1]))
        s = area.sum()
        self.orientation = 0 if abs(s) <= area.size * U * np.abs(area).sum() else (1 if s > 0 else -1)
        o = LD(1 if self.orientation >= 0 else -1)
        self.jmin = (o * self.J).min(axis=(2, 3))
        self.jmax = (o * self.J).max(axis=(2, 3))
        self.delta = self.bar_J.max(axis=(2, 3))                              # per element: how far Jmin / Jmax may be off
        finite = np.isfinite(self.J).all(axis=(2, 3))
        self.valid = finite & (self.jmin > 0)
        self.invalid = int((~self.valid).sum())
        with np.errstate(all="ignore"):
            self.sj = np.where(self.valid, self.jmin / self.jmax, np.nan)

    def decided(self):
        """Elements whose validity does not depend on rounding: |Jmin| clear of zero by the bar."""
        return np.abs(self.jmin) > self.delta

    def sj_interval(self):
        """(lo, hi) per element: what Jmin / Jmax can be when both are within delta of the reference (plus the division's rounding)."""
        d = self.delta
        with np.errstate(all="ignore"):
            lo = (self.jmin - d) / (self.jmax + d)
            hi = (self.jmin + d) / (self.jmax - d)
        return lo * (1 - 2 * U), hi * (1 + 2 * U)


def worst_ratio(got, ref, bar):
    """max |got - ref| / bar over entries with a non-zero bar; entries with a zero bar must be equal."""
    err = np.abs(got.astype(LD) - ref)
    zero = bar == 0
    assert np.all(err[zero] == 0)
    return float((err[~zero] / bar[~zero]).max()) if (~zero).any() else 0.0


def fold(X, p):
    """A copy of X with element (0, 0) folded: rows 1 and 2 of its interior nodes swapped; at p = 2 (one interior node) the centre
    node pushed three times past its neighbour along i."""
    Y = X.copy()
    if p == 2:
        Y[1, 1] = Y[1, 1] + 3.0 * (Y[2, 1] - Y[1, 1])
    else:
        Y[[1, 2], 1:p] = Y[[2, 1], 1:p]
    return Y


def prescribed_nodes(p):
    """A strictly increasing set that is neither equidistant nor Gauss-Lobatto."""
    t = (np.arange(p + 1) / p) ** 1.3
    t[0], t[p] = 0.0, 1.0
    return t
