"""Reference of the spanwise stacking (include/tm_hip.h, "3-D from 2-D cuts") in numpy longdouble, written from the definition:

    weights_ref(span, layers, interpolation)       the (nk, K) weight matrix; the spline by SOLVING the system of the second derivatives
    stack_ref(blocks, A, mapping, span, layers)    X, Y, Z as (nk, nj, ni) longdouble arrays
    stack_bar(blocks, A, mapping, span, layers)    the bars of the issue for X, Y, Z, same shapes

eps = 2^-52.  Values: (K+1) eps sum_c |A_kc| |v_c| (the classical dot-product bound; the weights' own error is judged separately).
Cylindrical y, z: r ((K+2) eps sum_c |A_kc| |theta_c| + 5 eps) -- the division theta_c = y_c / z_c adds one rounding to the K+1, and
5 eps = 4 ulp of sin / cos (OpenCL's fp64 bound, which ocml documents) + the rounding of the product with r."""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52


def _solve(T, R):
    """Gaussian elimination with partial pivoting in longdouble (numpy.linalg has no longdouble); R may have several columns."""
    T, R = np.array(T, dtype=LD), np.array(R, dtype=LD)
    n = T.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(T[k:, k])))
        if p != k:
            T[[k, p]], R[[k, p]] = T[[p, k]], R[[p, k]]
        for r in range(k + 1, n):
            f = T[r, k] / T[k, k]
            if f != 0:
                T[r, k:] -= f * T[k, k:]
                R[r] -= f * R[k]
    X = np.zeros_like(R)
    for k in range(n - 1, -1, -1):
        X[k] = (R[k] - T[k, k + 1:] @ X[k + 1:]) / T[k, k]
    return X


def second_derivative_map(z):
    """G (K, K): M = G v for the natural spline through (z_c, v_c): rows 0 and K-1 say M = 0, row m the continuity of S' at cut m."""
    z = np.asarray(z, dtype=LD)
    K = z.size
    T, D = np.zeros((K, K), dtype=LD), np.zeros((K, K), dtype=LD)
    T[0, 0] = T[K - 1, K - 1] = 1
    for m in range(1, K - 1):
        h0, h1 = z[m] - z[m - 1], z[m + 1] - z[m]
        T[m, m - 1], T[m, m], T[m, m + 1] = h0 / 6, (h0 + h1) / 3, h1 / 6
        D[m, m - 1], D[m, m], D[m, m + 1] = 1 / h0, -(1 / h0 + 1 / h1), 1 / h1
    return _solve(T, D)


def weights_ref(span, layers, interpolation):
    z64, s64 = np.asarray(span, dtype=np.float64), np.asarray(layers, dtype=np.float64)
    z = z64.astype(LD)
    K = z.size
    G = second_derivative_map(z) if interpolation == "cubic" else None
    A = np.zeros((s64.size, K), dtype=LD)
    eye = np.eye(K, dtype=LD)
    for k, s in enumerate(s64):
        hit = np.nonzero(z64 == s)[0]
        if hit.size:
            A[k, hit[0]] = 1
            continue
        c = max(q for q in range(K - 1) if z64[q] <= s)
        h = z[c + 1] - z[c]
        s = LD(s)
        if interpolation == "linear":
            t = (s - z[c]) / h
            A[k, c], A[k, c + 1] = 1 - t, t
        else:
            a, b = (z[c + 1] - s) / h, (s - z[c]) / h
            A[k] = a * eye[c] + b * eye[c + 1] + ((a ** 3 - a) * G[c] + (b ** 3 - b) * G[c + 1]) * h * h / 6
    return A


def _planes(blocks):
    """K blocks (ni, nj, 2) -> x, y as (K, nj, ni) longdouble (PLOT3D order)."""
    v = np.stack([np.asarray(b, dtype=np.float64) for b in blocks]).astype(LD)
    return np.transpose(v[..., 0], (0, 2, 1)), np.transpose(v[..., 1], (0, 2, 1))


def stack_ref(blocks, A, mapping, span=None, layers=None):
    A = np.asarray(A).astype(LD)
    x, y = _planes(blocks)
    X = np.einsum("kc,cji->kji", A, x)
    nk = A.shape[0]
    s = np.asarray(layers, dtype=np.float64).astype(LD)
    if mapping == "planar":
        return X, np.einsum("kc,cji->kji", A, y), np.broadcast_to(s[:, None, None], X.shape).copy()
    th = np.einsum("kc,cji->kji", A, y / np.asarray(span, dtype=np.float64).astype(LD)[:, None, None])
    r = s[:, None, None]
    assert nk == s.size
    return X, r * np.sin(th), r * np.cos(th)


def stack_bar(blocks, A, mapping, span=None, layers=None):
    A = np.abs(np.asarray(A).astype(LD))
    K = A.shape[1]
    x, y = _planes(blocks)
    bx = (K + 1) * EPS * np.einsum("kc,cji->kji", A, np.abs(x))
    if mapping == "planar":
        return bx, (K + 1) * EPS * np.einsum("kc,cji->kji", A, np.abs(y)), np.zeros_like(bx)
    th = np.abs(y / np.asarray(span, dtype=np.float64).astype(LD)[:, None, None])
    r = np.abs(np.asarray(layers, dtype=np.float64).astype(LD))[:, None, None]
    b = r * ((K + 2) * EPS * np.einsum("kc,cji->kji", A, th) + 5 * EPS)
    return bx, b, b


def worst_ratio(got, ref, bar):
    """max |got - ref| / bar over the entries (0 where both vanish); the assertion is ratio <= 1."""
    d = np.abs(np.asarray(got).astype(LD) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(d == 0, LD(0), d / bar)
    return float(np.max(q))


# ------------------------------------------------------------------ inputs shared by the CPU and the GPU tests
def spans(K, kind, z0=1.0):
    """uniform: K equidistant positions from z0; nonuniform: intervals alternating 1 : 100 (ratio of neighbours up to 100)."""
    if kind == "uniform":
        return z0 + 0.25 * np.arange(K, dtype=np.float64)
    h = np.array([1.0 if c % 2 == 0 else 100.0 for c in range(K - 1)]) * 0.013
    return z0 + np.concatenate([[0.0], np.cumsum(h)])


def layers_with_cuts(span, nk, seed=0):
    """nk layer positions inside the span, in no particular order: the first cut, a random position, the last cut, then the interior cuts
    and random positions in turn (random positions alone once the cuts are used up); a single layer is a random position.  Every cut is
    among them when nk >= 2 K - 1."""
    span = np.asarray(span, dtype=np.float64)
    rng = np.random.default_rng(1000 + seed)
    rand = lambda: float(rng.uniform(span[0], span[-1]))   # noqa: E731
    interior = list(span[1:-1])
    s = [rand()] if nk == 1 else [span[0], rand(), span[-1]][:nk]
    while len(s) < nk:
        s.append(interior.pop(0) if interior else rand())
        if len(s) < nk:
            s.append(rand())
    s = np.array(s)
    rng.shuffle(s)
    return np.clip(s, span[0], span[-1])
