"""Reference for the high-order hexahedra of stacked blocks (include/tm_hip.h, "high-order hexahedra of stacked blocks"), written from
the definition alone in numpy longdouble (80-bit on x86-64): Y = (T x T x T) F per element with its three derivatives, the Jacobian, the
orientation from the corner hexahedra, the element and block records, and the error bars the tests hold the library to.  Nodes and
tables are those of tests/ho_reference.py (the definition says: unchanged).

Bars (u = 2^-53), derived as in tests/ho_reference.py:
  nodes      one stage is a dot product of p+1 terms: a multiplication and p additions along the longest path, and the table entry was
             rounded once -- p+2 roundings per stage.  Two stages gave 2(p+2) = 2p+4, held as 2p+6 (the margin of 2 pays the products of
             roundings, which the first-order count leaves out).  Three stages give 3(p+2) = 3p+6, held with the same margin per stage
             as 3p+9:   |Y - Y_ref| <= (3p+9) u sum |C_c| |B_b| |A_a| |F|.
             The same bound holds for each derivative with its table D in the place of one T; S_* below is that absolute contraction.
  Jacobian   J is a sum of six triple products d1*d2*d3, one factor from each of d/du, d/dv, d/dw.  Each factor carries (3p+9) u relative
             to its S; a triple product adds its two multiplications, the inner difference one rounding, the outer difference and sum two
             more: 3(3p+9) + 5 = 9p+32 relative to the product of the three S, and the six products are summed:
             |J - J_ref| <= (9p+32) u (S_xu (S_yv S_zw + S_yw S_zv) + S_xv (S_yu S_zw + S_yw S_zu) + S_xw (S_yu S_zv + S_yv S_zu)).
"""
import numpy as np

from tests import ho_reference as hr

LD = np.longdouble
U = hr.U


def elements_of(X, Y, Z, p):
    """(Ei, Ej, Eg, p+1, p+1, p+1, 3) longdouble: the fine nodes F[m][n][l] of every element, from (nk, nj, ni) planes."""
    nk, nj, ni = X.shape
    assert (ni - 1) % p == 0 and (nj - 1) % p == 0 and (nk - 1) % p == 0 and nk >= p + 1
    F = np.stack([X, Y, Z], axis=-1).astype(LD).transpose(2, 1, 0, 3)            # [i, j, k, component]
    idx = lambda E: np.arange(E)[:, None] * p + np.arange(p + 1)[None, :]         # noqa: E731
    i, j, k = idx((ni - 1) // p), idx((nj - 1) // p), idx((nk - 1) // p)
    return F[i[:, None, None, :, None, None], j[None, :, None, None, :, None], k[None, None, :, None, None, :]]


def _contract(A, B, Cc, Fe):
    """R[e, f, g, a, b, c, q] = sum_m sum_n sum_l A[a, m] B[b, n] C[c, l] F[e, f, g, m, n, l, q]"""
    return np.einsum("am,bn,cl,efgmnlq->efgabcq", A, B, Cc, Fe)


def hexahedron_volume(x):
    """The exact volume of the trilinear hexahedron, x[..., a + 2b + 4c, :] its corners (the expression of "3-D quality of stacked
    blocks")."""
    det = lambda p, q, r: np.einsum("...i,...i->...", p, np.cross(q, r))          # noqa: E731
    d71, d60, d72, d30, d50, d74 = x[..., 7, :] - x[..., 1, :], x[..., 6, :] - x[..., 0, :], x[..., 7, :] - x[..., 2, :], x[..., 3, :] - x[..., 0, :], \
        x[..., 5, :] - x[..., 0, :], x[..., 7, :] - x[..., 4, :]
    return (det(d71 + d60, d72, d30) + det(d60, d72 + d50, d74) + det(d71, d50, d74 + d30)) / LD(12)


class Reference:
    """Everything the tests compare against, for one 3-D block (X, Y, Z as (nk, nj, ni) arrays) and one elevation."""

    def __init__(self, X, Y, Z, p, distribution, prescribed=None):
        self.p = p
        T, D = hr.tables(p, distribution, prescribed)
        Fe = elements_of(X, Y, Z, p)
        self.Ei, self.Ej, self.Eg = Fe.shape[:3]
        self.Ye = _contract(T, T, T, Fe)
        du, dv, dw = _contract(D, T, T, Fe), _contract(T, D, T, Fe), _contract(T, T, D, Fe)
        x, y, z = 0, 1, 2
        self.J = (du[..., x] * (dv[..., y] * dw[..., z] - dw[..., y] * dv[..., z]) - dv[..., x] * (du[..., y] * dw[..., z] - dw[..., y] * du[..., z])
                  + dw[..., x] * (du[..., y] * dv[..., z] - dv[..., y] * du[..., z]))                                   # (Ei, Ej, Eg, p+1, p+1, p+1)
        aT, aD, aF = np.abs(T), np.abs(D), np.abs(Fe)
        self.bar_Ye = (3 * p + 9) * U * _contract(aT, aT, aT, aF)
        su, sv, sw = _contract(aD, aT, aT, aF), _contract(aT, aD, aT, aF), _contract(aT, aT, aD, aF)
        self.bar_J = (9 * p + 32) * U * (su[..., x] * (sv[..., y] * sw[..., z] + sw[..., y] * sv[..., z]) + sv[..., x] * (su[..., y] * sw[..., z] + sw[..., y] * su[..., z])
                                        + sw[..., x] * (su[..., y] * sv[..., z] + sv[..., y] * su[..., z]))
        # the structured array (nk, nj, ni, 3): a seam node from the element above it, the last node of a line from the last element
        nk, nj, ni = X.shape
        self.Y = np.zeros((nk, nj, ni, 3), dtype=LD)
        self.bar_Y = np.zeros((nk, nj, ni, 3), dtype=LD)
        for e in range(self.Ei):
            for f in range(self.Ej):
                for g in range(self.Eg):
                    na, nb, nc = (p + 1 if e == self.Ei - 1 else p), (p + 1 if f == self.Ej - 1 else p), (p + 1 if g == self.Eg - 1 else p)
                    dst = (slice(g * p, g * p + nc), slice(f * p, f * p + nb), slice(e * p, e * p + na))
                    self.Y[dst] = self.Ye[e, f, g, :na, :nb, :nc].transpose(2, 1, 0, 3)
                    self.bar_Y[dst] = self.bar_Ye[e, f, g, :na, :nb, :nc].transpose(2, 1, 0, 3)
        # orientation: the hexahedra of element corners, corner a + 2b + 4c
        corners = np.stack([Fe[:, :, :, a * p, b * p, c * p, :] for c in (0, 1) for b in (0, 1) for a in (0, 1)], axis=-2)
        V = hexahedron_volume(corners)
        s = V.sum()
        self.orientation = 0 if abs(s) <= V.size * U * np.abs(V).sum() else (1 if s > 0 else -1)
        o = LD(1 if self.orientation >= 0 else -1)
        ax = (3, 4, 5)
        self.jmin, self.jmax = (o * self.J).min(axis=ax), (o * self.J).max(axis=ax)
        self.delta = self.bar_J.max(axis=ax)                                  # per element: how far Jmin / Jmax may be off
        self.valid = np.isfinite(self.J).all(axis=ax) & (self.jmin > 0)
        self.invalid = int((~self.valid).sum())
        with np.errstate(all="ignore"):
            self.sj = np.where(self.valid, self.jmin / self.jmax, np.nan)     # (Ei, Ej, Eg)

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


def bent_block(ni, nj, nk, seed=0):
    """A smooth, bent, right-handed block well clear of the origin in none of its coordinates: (X, Y, Z) as (nk, nj, ni) float64."""
    rng = np.random.default_rng(seed)
    k, j, i = np.meshgrid(np.arange(nk) / 8.0, np.arange(nj) / 8.0, np.arange(ni) / 8.0, indexing="ij")
    a = rng.uniform(0.02, 0.05, size=6)
    X = i + a[0] * np.sin(1.3 * j + 0.4) + a[1] * k * k
    Y = j + a[2] * np.cos(0.9 * i) + a[3] * np.sin(1.1 * k)
    Z = k + a[4] * i * j + a[5] * np.sin(0.7 * i + 0.5 * j)
    return X, Y, Z
