"""The welded numbering of include/tm_hip.h ("welded unstructured mesh") in plain Python / numpy, written from the definition alone: a
dictionary union-find over (block, i, j) keys.  Shares no code with the library."""
import numpy as np

I_MIN, I_MAX, J_MIN, J_MAX = 0, 1, 2, 3


def sizes_of(mesh):
    return [tuple(int(v) for v in b.points.size) for b in mesh.blocks]


def offsets_of(sizes):
    off, at = [], 0
    for ni, nj in sizes:
        off.append(at)
        at += ni * nj
    return off, at


def side_node(ni, nj, side, pos):
    side = int(side)
    if side == I_MIN:
        return pos, 0
    if side == I_MAX:
        return pos, nj - 1
    if side == J_MIN:
        return 0, pos
    return ni - 1, pos


def range_nodes(sizes, r):
    """[(block, i, j)] of a range, in the order of its pairs."""
    ni, nj = sizes[r.block]
    start, end = int(r.start), int(r.end)
    step = -1 if start > end else 1
    return [(int(r.block),) + side_node(ni, nj, r.side, p) for p in range(start, end + step, step)]


def weld_map(mesh):
    """-> (map int32[N], info dict) by first-occurrence numbering of the classes."""
    sizes = sizes_of(mesh)
    off, N = offsets_of(sizes)
    flat = lambda key: off[key[0]] + key[2] * sizes[key[0]][0] + key[1]
    parent = {}

    def find(k):
        parent.setdefault(k, k)
        while parent[k] != k:
            parent[k] = parent[parent[k]]
            k = parent[k]
        return k

    periodic = 0
    for c in mesh.connections:
        a, b = range_nodes(sizes, c.ranges[0]), range_nodes(sizes, c.ranges[1])
        assert len(a) == len(b)
        if c.periodicity is not None:
            periodic += len(a)
            continue
        for ka, kb in zip(a, b):
            ra, rb = find(ka), find(kb)
            if ra != rb:
                parent[ra] = rb
    members = {}
    for k in list(parent):
        members.setdefault(find(k), []).append(flat(k))
    owner = np.arange(N, dtype=np.int64)
    count = {2: 0, 3: 0, 4: 0, 5: 0}
    largest = 1
    for ms in members.values():
        owner[ms] = min(ms)
        if len(ms) >= 2:
            count[min(len(ms), 5)] += 1
            largest = max(largest, len(ms))
    is_owner = owner == np.arange(N)
    ids = np.cumsum(is_owner) - 1          # id of an owner = owners before it
    m = ids[owner].astype(np.int32)
    info = {"nodes_in": N, "nodes_out": int(is_owner.sum()), "classes_2": count[2], "classes_3": count[3], "classes_4": count[4],
            "classes_5_up": count[5], "max_class": largest, "periodic_pairs": periodic}
    return m, info, owner


def periodic_pairs(mesh, m):
    sizes = sizes_of(mesh)
    off, _ = offsets_of(sizes)
    flat = lambda key: off[key[0]] + key[2] * sizes[key[0]][0] + key[1]
    out = []
    for c in mesh.connections:
        if c.periodicity is None:
            continue
        a, b = range_nodes(sizes, c.ranges[0]), range_nodes(sizes, c.ranges[1])
        out.append((np.array([[m[flat(x)], m[flat(y)]] for x, y in zip(a, b)], dtype=np.int32), (float(c.periodicity[0]), float(c.periodicity[1]))))
    return out


def flat_planes(blocks):
    """blocks: per block a tuple of (nj, ni) or (nk, nj, ni) arrays -> (ncomp, nk, N) array in flat order."""
    ncomp = len(blocks[0])
    nk = blocks[0][0].shape[0] if blocks[0][0].ndim == 3 else 1
    return np.stack([np.concatenate([np.asarray(b[c]).reshape(nk, -1) for b in blocks], axis=1) for c in range(ncomp)])


def mesh_planes(mesh):
    return [(b.points.data[:, :, 0].T, b.points.data[:, :, 1].T) for b in mesh.blocks]


def weld_points(m, owner, blocks):
    """-> (points (nk * nodes_out, ncomp) layer-major, max_gap, gap_node)."""
    P = flat_planes(blocks)                       # (ncomp, nk, N)
    ncomp, nk, N = P.shape
    nodes_out = int(m.max()) + 1
    own = np.flatnonzero(owner == np.arange(N))
    out = np.empty((ncomp, nk, nodes_out))
    out[:, :, m[own]] = P[:, :, own]
    with np.errstate(invalid="ignore"):
        gap = np.abs(P - P[:, :, owner])
    gap = np.where(np.isnan(gap), 0.0, gap).max(axis=0).reshape(-1)      # (nk * N), index k * N + n
    node = int(np.argmax(gap))                    # the first index of the maximum
    return out.reshape(ncomp, -1).T.copy(), float(gap[node]), (node if gap[node] > 0 else 0)


def periodic_gap(mesh, m, points, nk=1):
    nodes_out = int(m.max()) + 1
    g = 0.0
    for pairs, t in periodic_pairs(mesh, m):
        for k in range(nk):
            for d in range(2):
                g = max(g, float(np.abs(points[k * nodes_out + pairs[:, 0], d] + t[d] - points[k * nodes_out + pairs[:, 1], d]).max()))
    return g


def quad_order(p):
    o = [(0, 0), (p, 0), (p, p), (0, p)]
    o += [(a, 0) for a in range(1, p)] + [(p, b) for b in range(1, p)] + [(a, p) for a in range(1, p)] + [(0, b) for b in range(1, p)]
    o += [(a, b) for b in range(1, p) for a in range(1, p)]
    return o


def weld_cells(mesh, m, order, nk=0, local=None):
    """Quadrilaterals (nk < 2) or hexahedra; local: the local node order ((a, b) or (a, b, c) tuples), default the quadrilateral's."""
    sizes = sizes_of(mesh)
    off, _ = offsets_of(sizes)
    nodes_out = int(m.max()) + 1
    p = order
    local = local if local is not None else quad_order(p)
    rows = []
    for (ni, nj), o in zip(sizes, off):
        for g in range((nk - 1) // p if nk >= 2 else 1):
            for f in range((nj - 1) // p):
                for e in range((ni - 1) // p):
                    rows.append([(g * p + (l[2] if len(l) > 2 else 0)) * nodes_out + m[o + (f * p + l[1]) * ni + e * p + l[0]] for l in local])
    return np.array(rows, dtype=np.int32)


def edges_of_quads(cells4):
    """Number of distinct edges of linear quadrilaterals (corner ids in ring order)."""
    e = set()
    for c in np.asarray(cells4)[:, :4].tolist():
        for a, b in zip(c, c[1:] + c[:1]):
            e.add((min(a, b), max(a, b)))
    return len(e)
