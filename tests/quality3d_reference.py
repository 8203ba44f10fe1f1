"""Reference of the 3-D quality report (include/tm_hip.h, "3-D quality of stacked blocks") in numpy longdouble, written from the header
text: corners, the exact trilinear volume, orientation, classes, histogram, aspect, spanwise growth.

    report(X, Y, Z)   X, Y, Z: (nk, nj, ni) arrays (PLOT3D order).  Returns a dict with the fields of tm_quality3d, `field` (per-cell min of
                      o*s as (nk-1, nj-1, ni-1) longdouble, NaN for degenerate cells) and `near_boundary`: the number of non-degenerate cells
                      whose min o*s (or min o*J relative to the edge product) lies within 1e-12 of a histogram edge k/10 or of the class
                      boundary 0 -- where an fp64 evaluation may legitimately land in the neighbouring bin or class.
"""
import numpy as np

LD = np.longdouble


def _det(p, q, r):
    return (p[..., 0] * (q[..., 1] * r[..., 2] - q[..., 2] * r[..., 1]) + p[..., 1] * (q[..., 2] * r[..., 0] - q[..., 0] * r[..., 2])
            + p[..., 2] * (q[..., 0] * r[..., 1] - q[..., 1] * r[..., 0]))


def _len(d):
    return np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])


def report(X, Y, Z):
    P = np.stack([np.asarray(a, dtype=np.float64).astype(LD) for a in (X, Y, Z)], axis=-1)   # [k, j, i, xyz]
    nk, nj, ni = P.shape[:3]
    cells = (ni - 1) * (nj - 1) * (nk - 1)

    def node(a, b, c):   # corner (a, b, c) of every cell, [k, j, i, xyz]
        return P[c:nk - 1 + c, b:nj - 1 + b, a:ni - 1 + a]

    J, S, prod = [], [], []
    with np.errstate(divide="ignore", invalid="ignore"):
        for c in (0, 1):
            for b in (0, 1):
                for a in (0, 1):
                    here = node(a, b, c)
                    u = (node(1 - a, b, c) - here) * (1 - 2 * a)
                    v = (node(a, 1 - b, c) - here) * (1 - 2 * b)
                    w = (node(a, b, 1 - c) - here) * (1 - 2 * c)
                    j = _det(u, v, w)
                    p = (_len(u) * _len(v)) * _len(w)
                    J.append(j)
                    prod.append(p)
                    S.append(j / p)
    J, S, prod = np.array(J), np.array(S), np.array(prod)
    x = [node(m & 1, (m >> 1) & 1, m >> 2) for m in range(8)]
    V = (_det((x[7] - x[1]) + (x[6] - x[0]), x[7] - x[2], x[3] - x[0]) + _det(x[6] - x[0], (x[7] - x[2]) + (x[5] - x[0]), x[7] - x[4])
         + _det(x[7] - x[1], x[5] - x[0], (x[7] - x[4]) + (x[3] - x[0]))) / 12
    sumV, sumA = V.sum(), np.abs(V).sum()
    o = 0
    if abs(sumV) > cells * LD(2.0) ** -53 * sumA:
        o = 1 if sumV > 0 else -1
    oo = 1 if o >= 0 else -1
    degenerate = np.any((prod == 0) | ~np.isfinite(prod) | ~np.isfinite(J), axis=0)
    minJ, minS = (oo * J).min(axis=0), (oo * S).min(axis=0)
    inverted = ~degenerate & (minJ <= 0)
    valid = ~degenerate & ~inverted
    field = np.where(degenerate, LD(np.nan), minS)
    out = {"cells": cells, "degenerate": int(degenerate.sum()), "inverted": int(inverted.sum()), "orientation": o, "field": field}
    any_cell = bool((~degenerate).any())
    if any_cell:
        flat = np.where(degenerate, LD(np.inf), minS).reshape(-1)
        worst = int(np.argmin(flat))   # first occurrence: the lowest (k, j, i)
        out["min_scaled_jacobian"] = flat[worst]
        out["worst"] = (worst % (ni - 1), (worst // (ni - 1)) % (nj - 1), worst // ((ni - 1) * (nj - 1)))
    else:
        out["min_scaled_jacobian"], out["worst"] = LD(np.nan), (0, 0, 0)
    bins = np.minimum((minS[valid] * 10).astype(np.int64), 9)
    out["hist"] = tuple(int(n) for n in np.bincount(bins, minlength=10)) if bins.size else (0,) * 10
    edges = np.arange(0, 10, dtype=LD) / 10
    live = minS[~degenerate]
    out["near_boundary"] = int((np.abs(live[:, None] - edges[None, :]).min(axis=1) <= LD(1e-12)).sum()) if live.size else 0
    # aspect: the sums of the four edges of each direction
    Li = _len(x[1] - x[0]) + _len(x[3] - x[2]) + _len(x[5] - x[4]) + _len(x[7] - x[6])
    Lj = _len(x[2] - x[0]) + _len(x[3] - x[1]) + _len(x[6] - x[4]) + _len(x[7] - x[5])
    Lk = _len(x[4] - x[0]) + _len(x[5] - x[1]) + _len(x[6] - x[2]) + _len(x[7] - x[3])
    with np.errstate(divide="ignore", invalid="ignore"):
        aspect = np.maximum(np.maximum(Li, Lj), Lk) / np.minimum(np.minimum(Li, Lj), Lk)
    out["max_aspect"] = aspect[~degenerate].max() if any_cell else LD(np.nan)
    # growth of consecutive k-edges along every spanwise line
    g = LD(1)
    if nk >= 3:
        lk = _len(P[1:] - P[:-1])
        l0, l1 = lk[:-1], lk[1:]
        ok = (l0 != 0) & (l1 != 0)
        if ok.any():
            g = max(g, (np.maximum(l0, l1)[ok] / np.minimum(l0, l1)[ok]).max())
    out["max_growth_k"] = g
    out["min_volume"] = (oo * V)[~degenerate].min() if any_cell else LD(np.nan)
    out["max_volume"] = (oo * V)[~degenerate].max() if any_cell else LD(np.nan)
    out["total_volume"] = oo * sumV
    out["sum_abs_volume"] = sumA
    return out
