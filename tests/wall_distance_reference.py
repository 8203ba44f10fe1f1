"""Reference for the wall distance of the welded mesh (include/tm_hip.h, "wall distance of the welded mesh"), written from the definition
in numpy longdouble over ALL pairs; it does not import the library.

The image of a query point is part of the definition and is formed in float64 in the stated order; everything behind it is longdouble.
A 2-D face is a segment.  A 3-D face is the triangles (A, B, C) and (A, C, D), and the distance to a triangle is formed here as the
minimum over its three edges and the in-plane foot point where that lies inside -- on purpose not the region form of the library."""
import numpy as np

LD = np.longdouble
EPS = LD(2.0) ** -53


def image_points(dim, pts, image):
    """P' of every point under one image (t0, t1, t2, c, s), float64, in the expression order of the definition."""
    t0, t1, t2, c, s = (np.float64(v) for v in image)
    x, y = pts[:, 0], pts[:, 1]
    if dim == 2:
        return np.stack([x - t0, y - t1], axis=1)
    z = pts[:, 2]
    return np.stack([x - t0, (c * y + s * z) - t1, (-s * y + c * z) - t2], axis=1)


def _dot(u, v):
    return (u * v).sum(axis=-1)


def segment_d2(P, A, B):
    """P (n, 1, d), A and B (1, m, d) longdouble -> (n, m) squared distances to the segments"""
    a = B - A
    L = _dot(a, a)
    p = P - A
    t = _dot(p, a)
    safe = np.where(L > 0, L, LD(1))
    s = np.clip(t / safe, LD(0), LD(1))
    s = np.where(L > 0, s, LD(0))
    q = p - s[..., None] * a
    return _dot(q, q)


def triangle_d2(P, A, B, C):
    d2 = np.minimum(np.minimum(segment_d2(P, A, B), segment_d2(P, B, C)), segment_d2(P, C, A))
    ab, ac = B - A, C - A
    n = np.cross(ab, ac)
    nn = _dot(n, n)
    ok = nn > 0
    safe = np.where(ok, nn, LD(1))
    ap = P - A
    h = _dot(ap, n)
    foot = ap - (h / safe)[..., None] * n   # relative to A, in the plane
    # inside when the foot lies on the inner side of all three edges
    inside = ok & (_dot(np.cross(ab, foot), n) >= 0) & (_dot(np.cross(C - B, foot - ab), n) >= 0) & (_dot(np.cross(A - C, foot - ac), n) >= 0)
    return np.where(inside, np.minimum(d2, h * h / safe), d2)


def pairs(dim, faces, pts, images, rows=None):
    """d2_ref and rho2, both (points, faces, images) longdouble, of the points `rows` (default all).  rho2 = the largest squared distance
    from P' to the nodes of the face + its longest squared edge (for a quadrilateral the four sides and the diagonal A-C)."""
    faces = np.asarray(faces)
    pts = np.asarray(pts, dtype=np.float64)
    sel = pts if rows is None else pts[rows]
    V = [pts[faces[:, k], :dim].astype(LD)[None] for k in range(faces.shape[1])]
    edges = [(0, 1)] if dim == 2 else [(0, 1), (1, 2), (2, 3), (3, 0), (0, 2)]
    longest = np.max([_dot(V[b] - V[a], V[b] - V[a]) for a, b in edges], axis=0).astype(np.float64)
    V64 = [v.astype(np.float64) for v in V]
    d2 = np.empty((len(sel), len(faces), len(images)), dtype=LD)
    rho2 = np.empty_like(d2)
    for m, image in enumerate(images):
        P = image_points(dim, sel, image).astype(LD)[:, None, :]
        if dim == 2:
            d2[:, :, m] = segment_d2(P, V[0], V[1])
        else:
            d2[:, :, m] = np.minimum(triangle_d2(P, V[0], V[1], V[2]), triangle_d2(P, V[0], V[2], V[3]))
        P64 = P.astype(np.float64)   # rho2 only scales the bar: float64 is enough for it
        rho2[:, :, m] = np.max([_dot(P64 - v, P64 - v) for v in V64], axis=0) + longest
    return d2, rho2


def check(dim, faces, pts, images, distance, face, image, G, rows=None, chunk=1024):
    """The two bars of the tests for the points `rows`: |distance^2 - min d2_ref| and d2_ref(returned face, image) - min d2_ref, both at
    most G 2^-53 rho2 of the returned pair (rho2 of the pair that attains the minimum for the first, whichever is larger).  Returns the
    worst ratio to 2^-53 rho2 seen, for the record."""
    rows = np.arange(len(pts)) if rows is None else np.asarray(rows)
    worst = 0.0
    for at in range(0, len(rows), chunk):
        r = rows[at:at + chunk]
        d2, rho2 = pairs(dim, faces, pts, images, r)
        flat = d2.reshape(len(r), -1)
        k = flat.argmin(axis=1)
        lo = flat[np.arange(len(r)), k]
        rho_lo = rho2.reshape(len(r), -1)[np.arange(len(r)), k]
        got = distance[r].astype(LD) ** 2   # the square of a rounded square root: 2 * 2^-53 d2 more, inside the rounding-up of G (DESIGN)
        rho_got = rho2[np.arange(len(r)), face[r], image[r]]
        bar = EPS * np.maximum(rho_lo, rho_got)
        e1 = np.abs(got - lo)
        e2 = d2[np.arange(len(r)), face[r], image[r]] - lo
        assert (e1 <= G * bar).all(), (float((e1 / bar).max()), G)
        assert (e2 <= G * bar).all(), (float((e2 / bar).max()), G)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(bar > 0, np.maximum(e1, e2) / np.where(bar > 0, bar, 1), 0)
        worst = max(worst, float(ratio.max()))
    return worst
