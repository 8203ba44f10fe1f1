"""The face-based view and the finite-volume metrics of include/tm_hip.h ("faces of the welded mesh") in plain Python / numpy, written from
the definition with the TOPOLOGICAL rule: a face is a set of node ids that occurs on a side of one cell (boundary) or of two cells (interior)
of weld_reference.weld_cells.  Owner, neighbour, order and rings are restated from the definition.  Shares no code with the library.

The metrics are formed in longdouble, and every value carries a bound on what IEEE fp64 arithmetic in the definition's order of operations
can differ from it by -- class EV, a running first-order error bound:
    a +- b   e = e_a + e_b, then the rounding of the result          a * b   e = |a| e_b + |b| e_a + e_a e_b, then the rounding
    a / b    e = (e_a + |a / b| e_b) / (|b| - e_b), then the rounding    sqrt a  e = e_a / (sqrt(a - e_a) + sqrt a), then the rounding
    rounding of a result r with propagated bound e: U (|r| + e), U = 2^-53; scaling by a power of two, negation, |.|, max: no rounding.
The inputs (welded coordinates) are exact.  The reference's own rounding is 2^-64 per operation, 2^-11 of each fp64 rounding term: every
bound is widened by 1 + 2^-10 for it (OWN).  No other tolerance appears."""
import numpy as np

from tests import weld_boundary_reference as WB
from tests import weld_reference as R

LD = np.longdouble
U = LD(2.0) ** -53
OWN = 1.0 + 2.0 ** -10
COS_70 = LD(0.3420201433256687)   # the constant of the definition: cos 70 degrees as a double
HEX_LOCAL = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
# local side -> positions in the cell's corner ring of the two nodes A -> B of the side, counter-clockwise in index space
SIDE_RING = {R.I_MIN: (0, 1), R.J_MAX: (1, 2), R.I_MAX: (2, 3), R.J_MIN: (3, 0)}


class OwnNeighbour(Exception):
    pass


def cell_blocks(mesh, nk):
    out = []
    for b, (ni, nj) in enumerate(R.sizes_of(mesh)):
        out += [b] * ((ni - 1) * (nj - 1) * (nk - 1 if nk >= 2 else 1))
    return out


def side_faces(c, o, layered):
    """the faces cell c (corner ids in VTK order) shows on its local sides 0 .. 3 (0 .. 5): tuples of ids in ring order"""
    out = []
    for side in range(4):
        a, b = SIDE_RING[side]
        if o < 0:
            a, b = b, a
        out.append((c[a], c[b], c[b + 4], c[a + 4]) if layered else (c[a], c[b]))
    if layered:
        out.append((c[0], c[3], c[2], c[1]) if o >= 0 else (c[0], c[1], c[2], c[3]))   # hub rule: a along j
        out.append((c[4], c[5], c[6], c[7]) if o >= 0 else (c[4], c[7], c[6], c[5]))   # shroud rule: a along i
    return out


def faces(mesh, m, nk=0, orientation=None):
    """-> dict faces (n, 2 | 4), owner (n,), neighbour (ninternal,), cell_faces (cells, 4 | 6), ninternal, boundary (WB.boundary's dict)"""
    layered = nk >= 2
    cells = R.weld_cells(mesh, m, 1, nk, HEX_LOCAL if layered else None).tolist()
    blocks = cell_blocks(mesh, nk)
    o_of = lambda b: 1 if orientation is None or orientation[b] >= 0 else -1
    shown, places_of = [], {}
    for c, ids in enumerate(cells):
        shown.append(side_faces(ids, o_of(blocks[c]), layered))
        for side, ring in enumerate(shown[c]):
            places_of.setdefault(frozenset(ring), []).append((c, side))
    interior = []
    for key, places in places_of.items():
        assert len(places) <= 2, "a face of more than two cells"
        if len(places) == 2:
            (c0, s0), (c1, s1) = sorted(places)
            if c0 == c1:
                raise OwnNeighbour(f"cell {c0} is its own neighbour across sides {s0} and {s1}")
            interior.append((c0, c1, s0, s1))
    interior.sort()
    fpc = 6 if layered else 4
    rows, owner, neighbour = [], [], []
    cell_faces = np.full((len(cells), fpc), -1, dtype=np.int32)
    for t, (c0, c1, s0, s1) in enumerate(interior):
        rows.append(shown[c0][s0])
        owner.append(c0)
        neighbour.append(c1)
        cell_faces[c0, s0] = cell_faces[c1, s1] = t
    ninternal = len(interior)
    bnd = WB.boundary(mesh, m, 1, nk, orientation)
    for t, ring in enumerate(bnd["faces"].tolist()):
        places = places_of[frozenset(ring)]
        assert len(places) == 1, "a boundary face of the range rule lies in two cells"
        c, side = places[0]
        assert tuple(ring) == tuple(shown[c][side]), "a boundary face is not its owner's face on that side"
        rows.append(tuple(ring))
        owner.append(c)
        cell_faces[c, side] = ninternal + t
    assert (cell_faces >= 0).all()
    return {"faces": np.array(rows, dtype=np.int32).reshape(len(rows), 4 if layered else 2), "owner": np.array(owner, dtype=np.int32),
            "neighbour": np.array(neighbour, dtype=np.int32), "cell_faces": cell_faces, "ninternal": ninternal, "boundary": bnd}


# ------------------------------------------------------------------ values with a running bound on the fp64 result
class EV:
    """v: the value in longdouble; e: a bound on |fp64 result of the same operations - v|"""

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=LD)
        self.e = np.zeros(self.v.shape, dtype=LD) if e is None else np.asarray(e, dtype=LD)
        if np.isnan(self.e).any():   # 0 * inf behind a denominator that its own bound reaches: no bound can be given
            self.e = np.where(np.isnan(self.e), LD(np.inf), self.e)

    @staticmethod
    def _rounded(v, e):
        return EV(v, e + U * (np.abs(v) + e))

    @staticmethod
    def of(x):
        return x if isinstance(x, EV) else EV(LD(x))

    def __add__(self, o):
        o = EV.of(o)
        return EV._rounded(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = EV.of(o)
        return EV._rounded(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        o = EV.of(o)
        return EV._rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    def __truediv__(self, o):
        o = EV.of(o)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = self.v / o.v
            den = np.abs(o.v) - o.e
            e = np.where(den > 0, (self.e + np.abs(q) * o.e) / den, LD(np.inf))
        return EV._rounded(q, e)

    def __neg__(self):
        return EV(-self.v, self.e)

    def scale(self, c):
        """by a power of two (or a sign): exact"""
        return EV(self.v * LD(c), self.e * abs(LD(c)))

    def abs(self):
        return EV(np.abs(self.v), self.e)

    def sqrt(self):
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.sqrt(self.v)
            lo = np.sqrt(np.maximum(self.v - self.e, 0))
            e = np.where(r + lo > 0, self.e / (r + lo), np.sqrt(self.e))
        return EV._rounded(r, e)

    def take(self, idx):
        return EV(self.v[idx], self.e[idx])

    def bar(self):
        return (self.e * LD(OWN)).astype(np.float64)


def emax(items):
    """max of the values; its bound is the largest bound (|max a - max b| <= max |a_i - b_i|)"""
    v, e = items[0].v, items[0].e
    for x in items[1:]:
        v, e = np.maximum(v, x.v), np.maximum(e, x.e)
    return EV(v, e)


def where(cond, a, b):
    return EV(np.where(cond, a.v, b.v), np.where(cond, a.e, b.e))


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross_half(a, b):
    return [(a[1] * b[2] - a[2] * b[1]).scale(0.5), (a[2] * b[0] - a[0] * b[2]).scale(0.5), (a[0] * b[1] - a[1] * b[0]).scale(0.5)]


def face_geometry(dim, P):
    """P[k][c]: EV over the faces, node k, component c -> (S, Cf) as lists of three EV"""
    zero = EV(np.zeros(P[0][0].v.shape))
    if dim == 2:
        A, B = P
        return [B[1] - A[1], -(B[0] - A[0]), zero], [(A[0] + B[0]).scale(0.5), (A[1] + B[1]).scale(0.5), zero]
    A, B, C, D = P
    u = [C[c] - A[c] for c in range(3)]
    v = [D[c] - B[c] for c in range(3)]
    S = cross_half(u, v)
    m = [(((A[c] + B[c]) + C[c]) + D[c]).scale(0.25) for c in range(3)]
    r = [[P[k][c] - m[c] for c in range(3)] for k in range(4)]
    W, acc = zero, [zero, zero, zero]
    for k in range(4):
        a, b = r[k], r[(k + 1) % 4]
        n = cross_half(a, b)
        w = ((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]).sqrt()
        W = W + w
        acc = [acc[c] + w * ((a[c] + b[c]) / 3.0) for c in range(3)]
    return S, [where(W.v > 0, m[c] + acc[c] / W, m[c]) for c in range(3)]


def metrics(f, points):
    """f: the dict of faces(); points (n, 2 | 3) -> dict of EV: volume, closedness (cells,), centre [3] (cells,), area [3], face_centre [3],
    cos (faces,), skewness (internal faces,)"""
    F, owner, nb, cf, ni = f["faces"], f["owner"].astype(np.int64), f["neighbour"].astype(np.int64), f["cell_faces"].astype(np.int64), f["ninternal"]
    dim = 2 if F.shape[1] == 2 else 3
    pts = np.asarray(points, dtype=LD)
    P = [[EV(pts[F[:, k], c]) if c < dim else EV(np.zeros(len(F))) for c in range(3)] for k in range(F.shape[1])]
    S, Cf = face_geometry(dim, P)
    nc, fpc = cf.shape
    cell = np.arange(nc)
    zero = EV(np.zeros(nc))
    Sk = [[S[c].take(cf[:, k]) for c in range(3)] for k in range(fpc)]
    Ck = [[Cf[c].take(cf[:, k]) for c in range(3)] for k in range(fpc)]
    sign = [np.where(owner[cf[:, k]] == cell, 1.0, -1.0).astype(LD) for k in range(fpc)]
    mean = [zero, zero, zero]
    for k in range(fpc):
        mean = [mean[c] + Ck[k][c] for c in range(3)]
    mean = [mean[c] / float(fpc) for c in range(3)]
    base = EV(LD(2) / LD(3), U * LD(2) / LD(3)) if dim == 2 else EV(LD(0.75))   # 2/3 is rounded once as a constant; 3/4 is exact
    V, mom, net, mag = zero, [zero] * 3, [zero] * 3, [zero] * 3
    for k in range(fpc):
        r = [Ck[k][c] - mean[c] for c in range(3)]
        t = dot(Sk[k], r) / float(dim)
        v = EV(t.v * sign[k], t.e)   # the sign is exact
        V = V + v
        mom = [mom[c] + v * (base * r[c]) for c in range(3)]
        signed = [EV(Sk[k][c].v * sign[k], Sk[k][c].e) for c in range(3)]
        net = [net[c] + signed[c] for c in range(3)]
        mag = [mag[c] + Sk[k][c].abs() for c in range(3)]
    centre = [where(V.v != 0, mean[c] + mom[c] / V, mean[c]) for c in range(3)]
    top, bottom = emax([x.abs() for x in net]), emax(mag)
    closed = where(bottom.v > 0, top / bottom, zero)
    # faces
    nf = len(F)
    interior = np.arange(nf) < ni
    other = np.concatenate([nb, np.zeros(nf - ni, dtype=np.int64)])
    Cown = [centre[c].take(owner) for c in range(3)]
    Cnb = [where(interior, centre[c].take(other), Cf[c]) for c in range(3)]
    d = [Cnb[c] - Cown[c] for c in range(3)]
    cos = dot(d, S) / (dot(d, d).sqrt() * dot(S, S).sqrt())
    e = [Cf[c] - Cown[c] for c in range(3)]
    ratio = dot(S, e) / dot(S, d)
    mvec = [e[c] - ratio * d[c] for c in range(3)]
    skew = dot(mvec, mvec).sqrt() / dot(d, d).sqrt()
    return {"volume": V, "closedness": closed, "centre": centre, "area": S, "face_centre": Cf, "cos": cos, "skewness": skew.take(np.arange(ni))}


def total_volume(V):
    """(sum in longdouble, bar of a sequential fp64 sum of the fp64 volumes against it): the terms' own bounds plus (n - 1) roundings of
    partial sums that are at most sum (|V| + e)"""
    n = len(V.v)
    size = (np.abs(V.v) + V.e).sum()
    return V.v.sum(), float((V.e.sum() + (n - 1) * U * size) * LD(OWN))


def extreme(x, largest):
    """(value, index) of the extreme with the smallest index at a tie; NaN never wins"""
    v = np.where(np.isnan(x.v), -np.inf if largest else np.inf, x.v)
    i = int(np.argmax(v) if largest else np.argmin(v))
    return x.v[i], i
