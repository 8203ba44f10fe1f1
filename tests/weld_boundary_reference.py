"""The boundary of the welded mesh of include/tm_hip.h ("boundary of the welded mesh") in plain Python / numpy, written from the definition
with the TOPOLOGICAL rule: a segment is a boundary face when its fine edges belong to exactly one cell of the welded order-1 mesh.
Classification by ranges, loops by union-find, terms and sums in longdouble.  Shares no code with the library."""
import numpy as np

from tests import weld_reference as R

LD = np.longdouble
U = 2.0 ** -53
PERIODIC, UNASSIGNED, HUB, SHROUD = 16, 17, 18, 19
# rounding of one term relative to its magnitude M (the sum of the absolute values of the products it is formed from; |t| itself where
# nothing cancels), in units of 2^-53 -- DESIGN.md section 4, K19:
#   plane    normal: one subtraction, 1.  length: dx, dy (1 each), squares (1), sum (1), sqrt (halves the 4, adds 1) -> 3, 4 with the
#            second-order terms.  moment: two products (1 each on M) and a subtraction (1 on |t| <= M) -> 2.
#   stacked  normal component: differences (2), product (1), subtraction (1), halving exact -> 4, 5 with second order.  measure: the
#            components carry 5 on Mx + My + Mz, squares, sums and sqrt 3 more -> 8.  moment: centroid (3 sums, the quarter exact), the
#            component (5), product (1), two sums (2) -> 11.
C_PLANE = (4.0, 1.0, 1.0, 0.0, 2.0)
C_STACKED = (8.0, 5.0, 5.0, 5.0, 11.0)


def quad_order(p):
    return R.quad_order(p)


def _covers(r, b, side, e, p):
    lo, hi = min(int(r.start), int(r.end)), max(int(r.start), int(r.end))
    return int(r.block) == b and int(r.side) == side and lo <= e * p and (e + 1) * p <= hi


def _edge_counts(mesh, m):
    cnt = {}
    for c in R.weld_cells(mesh, m, 1).tolist():
        for a, b in zip(c, c[1:] + c[:1]):
            k = (min(a, b), max(a, b))
            cnt[k] = cnt.get(k, 0) + 1
    return cnt


def side_positions(side, p, e, o):
    """positions along the side of the local nodes a = 0 .. p: counter-clockwise in index space, reversed for o = -1"""
    ascending = side in (R.I_MIN, R.J_MAX)
    pos = [e * p + a for a in range(p + 1)] if ascending else [(e + 1) * p - a for a in range(p + 1)]
    return pos[::-1] if o < 0 else pos


def boundary(mesh, m, order=1, nk=0, orientation=None):
    """-> dict: faces (n, npf), face_patch, origin (n, 4), patches [dict kind, source, partner, translation, begin, faces], loops, irregular."""
    p = order
    sizes = R.sizes_of(mesh)
    off, _ = R.offsets_of(sizes)
    nodes_out = int(m.max()) + 1
    o_of = [1 if orientation is None or orientation[b] >= 0 else -1 for b in range(len(sizes))]
    cnt = _edge_counts(mesh, m)
    idof = lambda b, i, j: int(m[off[b] + j * sizes[b][0] + i])

    def seg_ids(b, side, e, o):
        ni, nj = sizes[b]
        return [idof(b, *R.side_node(ni, nj, side, q)) for q in side_positions(side, p, e, o)]

    periodic = [(c, k) for k, c in enumerate(mesh.connections) if c.periodicity is not None]
    nbcs = len(mesh.boundary_conditions)
    patches = [dict(kind=int(bc.kind), source=k, partner=-1, translation=(0.0, 0.0)) for k, bc in enumerate(mesh.boundary_conditions)]
    for n, (c, k) in enumerate(periodic):
        t = (float(c.periodicity[0]), float(c.periodicity[1]))
        patches.append(dict(kind=PERIODIC, source=k, partner=nbcs + 2 * n + 1, translation=t))
        patches.append(dict(kind=PERIODIC, source=k, partner=nbcs + 2 * n, translation=(-t[0], -t[1])))
    unassigned = len(patches)
    patches.append(dict(kind=UNASSIGNED, source=-1, partner=-1, translation=(0.0, 0.0)))
    # every segment: boundary by the topological rule, its patch by the ranges
    seg_patch = {}
    for b, (ni, nj) in enumerate(sizes):
        for side in range(4):
            length = ni if side in (R.I_MIN, R.I_MAX) else nj
            for e in range((length - 1) // p):
                ids = seg_ids(b, side, e, 1)
                uses = {cnt[(min(x, y), max(x, y))] for x, y in zip(ids, ids[1:])}
                assert len(uses) == 1, "a segment partly inside the mesh"
                if uses == {2}:
                    continue
                assert uses == {1}
                q = unassigned
                hit = [nbcs + 2 * n + s for n, (c, _) in enumerate(periodic) for s in range(2) if _covers(c.ranges[s], b, side, e, p)]
                if hit:
                    q = hit[0]
                else:
                    hit = [k for k, bc in enumerate(mesh.boundary_conditions) if _covers(bc.range, b, side, e, p)]
                    if hit:
                        q = hit[0]
                seg_patch[(b, side, e)] = q
    lists = [[] for _ in patches]
    for n, (c, _) in enumerate(periodic):
        for s in range(2):
            r = c.ranges[s]
            step = -1 if int(r.start) > int(r.end) else 1
            for t in range((abs(int(r.end) - int(r.start))) // p):
                e = min(int(r.start) + step * t * p, int(r.start) + step * (t + 1) * p) // p
                key = (int(r.block), int(r.side), e)
                if seg_patch.get(key) == nbcs + 2 * n + s and key not in lists[nbcs + 2 * n + s]:
                    lists[nbcs + 2 * n + s].append(key)
    for key in sorted(seg_patch):
        if patches[seg_patch[key]]["kind"] != PERIODIC:
            lists[seg_patch[key]].append(key)
    layered = nk >= 2
    Eg = (nk - 1) // p if layered else 1
    local = quad_order(p)
    faces, face_patch, origin = [], [], []
    for q, keys in enumerate(lists):
        patches[q]["begin"] = len(faces)
        for g in range(Eg):
            for (b, side, e) in keys:
                ids = seg_ids(b, side, e, o_of[b])
                if not layered:
                    faces.append([ids[0], ids[p]] + ids[1:p])
                else:
                    faces.append([(g * p + c) * nodes_out + ids[a] for a, c in local])
                face_patch.append(q)
                origin.append((b, side, e, g))
        patches[q]["faces"] = len(faces) - patches[q]["begin"]
    if layered:
        for cap, kind in ((0, HUB), (1, SHROUD)):
            patches.append(dict(kind=kind, source=-1, partner=-1, translation=(0.0, 0.0), begin=len(faces)))
            for b, (ni, nj) in enumerate(sizes):
                Ei = (ni - 1) // p
                for f in range((nj - 1) // p):
                    for e in range(Ei):
                        a_along_i = (cap == 1) == (o_of[b] > 0)
                        row = []
                        for a, bp in local:
                            di, dj = (a, bp) if a_along_i else (bp, a)
                            row.append(cap * (nk - 1) * nodes_out + idof(b, e * p + di, f * p + dj))
                        faces.append(row)
                        face_patch.append(len(patches) - 1)
                        origin.append((b, 4 + cap, f * Ei + e, (Eg - 1) * cap))
            patches[-1]["faces"] = len(faces) - patches[-1]["begin"]
    # loops and irregular nodes of the plane boundary
    parent, degree = {}, {}

    def find(k):
        parent.setdefault(k, k)
        while parent[k] != k:
            parent[k] = parent[parent[k]]
            k = parent[k]
        return k

    for (b, side, e) in seg_patch:
        ids = seg_ids(b, side, e, 1)
        for x in (ids[0], ids[-1]):
            degree[x] = degree.get(x, 0) + 1
        parent[find(ids[0])] = find(ids[-1])
    npf = (p + 1) ** 2 if layered else p + 1
    return dict(faces=np.array(faces, dtype=np.int32).reshape(-1, npf), face_patch=np.array(face_patch, dtype=np.int32),
                origin=np.array(origin, dtype=np.int32).reshape(-1, 4), patches=patches, loops=len({find(k) for k in list(parent)}),
                irregular=sum(1 for d in degree.values() if d != 2))


def one_cell_edges(mesh, m):
    """The edges (sorted id pairs) of the welded order-1 mesh that lie in exactly one cell."""
    return {k for k, n in _edge_counts(mesh, m).items() if n == 1}


def measures(faces, face_patch, npatches, points, order, layered):
    """Per patch in longdouble: sums (npatches, 5) = measure, n_x, n_y, n_z, moment; abs (npatches, 5) = sum |t|; mag (npatches, 5) = sum of the
    terms' magnitudes M; terms (npatches,) = fine sub-faces."""
    p = order
    P = np.asarray(points, dtype=LD)
    sums, abss, mags = (np.zeros((npatches, 5), dtype=LD) for _ in range(3))
    terms = np.zeros(npatches, dtype=np.int64)
    F = np.asarray(faces)
    if not layered:
        at = lambda a: 0 if a == 0 else 1 if a == p else a + 1
        for a in range(p):
            A, B = P[F[:, at(a)]], P[F[:, at(a + 1)]]
            dx, dy = B[:, 0] - A[:, 0], B[:, 1] - A[:, 1]
            t = np.stack([np.sqrt(dx * dx + dy * dy), dy, -dx, np.zeros_like(dx), A[:, 0] * B[:, 1] - B[:, 0] * A[:, 1]], axis=1)
            M = np.abs(t)
            M[:, 4] = np.abs(A[:, 0] * B[:, 1]) + np.abs(B[:, 0] * A[:, 1])
            for q in range(npatches):
                sel = face_patch == q
                sums[q] += t[sel].sum(axis=0)
                abss[q] += np.abs(t[sel]).sum(axis=0)
                mags[q] += M[sel].sum(axis=0)
                terms[q] += int(sel.sum())
        return sums, abss, mags, terms
    where = {ab: k for k, ab in enumerate(quad_order(p))}
    for c in range(p):
        for a in range(p):
            A, B, Cc, D = (P[F[:, where[ab]]] for ab in ((a, c), (a + 1, c), (a + 1, c + 1), (a, c + 1)))
            u, v = Cc - A, D - B
            n = LD(0.5) * np.cross(u, v)
            Mn = LD(0.5) * np.stack([np.abs(u[:, 1] * v[:, 2]) + np.abs(u[:, 2] * v[:, 1]), np.abs(u[:, 2] * v[:, 0]) + np.abs(u[:, 0] * v[:, 2]),
                                     np.abs(u[:, 0] * v[:, 1]) + np.abs(u[:, 1] * v[:, 0])], axis=1)
            cen = LD(0.25) * (A + B + Cc + D)
            cen_abs = LD(0.25) * (np.abs(A) + np.abs(B) + np.abs(Cc) + np.abs(D))
            t = np.concatenate([np.sqrt((n * n).sum(axis=1))[:, None], n, (cen * n).sum(axis=1)[:, None]], axis=1)
            M = np.concatenate([Mn.sum(axis=1)[:, None], Mn, (cen_abs * Mn).sum(axis=1)[:, None]], axis=1)
            for q in range(npatches):
                sel = face_patch == q
                sums[q] += t[sel].sum(axis=0)
                abss[q] += np.abs(t[sel]).sum(axis=0)
                mags[q] += M[sel].sum(axis=0)
                terms[q] += int(sel.sum())
    return sums, abss, mags, terms


def bar_between_orders_of_summation(terms, abss):
    """|device - host| <= 2 (n - 1) 2^-53 sum |t|: identical terms, two orders of summation"""
    return 2.0 * np.maximum(terms - 1, 0)[:, None] * U * abss.astype(np.float64) * (1.0 + 2.0 ** -40)


def bar_against_reference(terms, abss, mags, layered):
    """the bar above plus c 2^-53 sum M for the rounding of the terms themselves"""
    c = np.array(C_STACKED if layered else C_PLANE)
    return bar_between_orders_of_summation(terms, abss) + c[None, :] * U * mags.astype(np.float64) * (1.0 + 2.0 ** -40)


def values_of(patches):
    return np.array([[r.measure, r.normal[0], r.normal[1], r.normal[2], r.moment] for r in patches], dtype=np.float64)


def signed_cell_areas(mesh, m, points, orientation):
    """sum over blocks of o_b * (sum of the shoelace areas of the block's order-1 cells on the welded points), in longdouble, and the sum of
    the absolute values of the products (for the error of this sum itself)."""
    P = np.asarray(points, dtype=LD)
    sizes = R.sizes_of(mesh)
    cells = R.weld_cells(mesh, m, 1)
    total, mag, at = LD(0), LD(0), 0
    for b, (ni, nj) in enumerate(sizes):
        n = (ni - 1) * (nj - 1)
        c = P[cells[at:at + n]]
        at += n
        x, y = c[:, :, 0], c[:, :, 1]
        xn, yn = np.roll(x, -1, axis=1), np.roll(y, -1, axis=1)
        total += LD(orientation[b]) * LD(0.5) * (x * yn - xn * y).sum()
        mag += LD(0.5) * (np.abs(x * yn) + np.abs(xn * y)).sum()
    return total, mag
