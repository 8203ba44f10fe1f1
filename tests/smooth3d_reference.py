"""One Jacobi sweep of the 3-D Winslow equations and the Thomas-Middlecoff control field of include/tm_hip.h ("elliptic smoothing of
stacked blocks") in numpy longdouble, written from the definition and sharing no code with the library.  Every value carries a bound on
what IEEE fp64 arithmetic in the definition's order of operations can differ from it by: fv_reference.EV, the running first-order error
bound of the K21 reference.  That bound -- widened by 1 + 2^-10 for the reference's own rounding -- is the bar of
every comparison per node and component; no other tolerance appears.

Arrays are (nk, nj, ni), PLOT3D order; results cover the interior nodes, shape (nk-2, nj-2, ni-2).  Also the blocks the tests share."""
import numpy as np

from tests.fv_reference import EV, LD

LAPLACE, THOMAS_MIDDLECOFF, PRESCRIBED = "laplace", "thomas-middlecoff", "prescribed"


def _ev(a):
    return a if isinstance(a, EV) else EV(np.asarray(a, dtype=np.float64).astype(LD))


def _shift(A, di, dj, dk):
    nk, nj, ni = A.v.shape
    sl = (slice(1 + dk, nk - 1 + dk), slice(1 + dj, nj - 1 + dj), slice(1 + di, ni - 1 + di))
    return EV(A.v[sl], A.e[sl])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def sweep(planes, omega=1.0, f=None):
    """planes: X, Y, Z as fp64 arrays (exact inputs) or EV; f: None (Laplace) or three interior-shaped arrays / EV.
    -> (out: three EV, frozen: bool array decided on the reference's values, J: EV)"""
    P = [_ev(a) for a in planes]
    at = lambda di, dj, dk: [_shift(A, di, dj, dk) for A in P]   # noqa: E731
    c = at(0, 0, 0)
    ip, im, jp, jm, kp, km = at(1, 0, 0), at(-1, 0, 0), at(0, 1, 0), at(0, -1, 0), at(0, 0, 1), at(0, 0, -1)
    half = lambda a, b: [(a[n] - b[n]).scale(0.5) for n in range(3)]   # noqa: E731
    r1, r2, r3 = half(ip, im), half(jp, jm), half(kp, km)
    s1, s2, s3 = ([a[n] + b[n] for n in range(3)] for a, b in ((ip, im), (jp, jm), (kp, km)))
    g11, g22, g33, g12, g13, g23 = _dot(r1, r1), _dot(r2, r2), _dot(r3, r3), _dot(r1, r2), _dot(r1, r3), _dot(r2, r3)
    a11 = g22 * g33 - g23 * g23
    a22 = g11 * g33 - g13 * g13
    a33 = g11 * g22 - g12 * g12
    a12 = g13 * g23 - g12 * g33
    a13 = g12 * g23 - g13 * g22
    a23 = g12 * g13 - g23 * g11
    mixed = lambda pp, pm, mp, mm: [(((pp[n] - pm[n]) - mp[n]) + mm[n]).scale(0.25) for n in range(3)]   # noqa: E731
    m12 = mixed(at(1, 1, 0), at(1, -1, 0), at(-1, 1, 0), at(-1, -1, 0))
    m13 = mixed(at(1, 0, 1), at(1, 0, -1), at(-1, 0, 1), at(-1, 0, -1))
    m23 = mixed(at(0, 1, 1), at(0, 1, -1), at(0, -1, 1), at(0, -1, -1))
    den = ((a11 + a22) + a33).scale(2.0)
    inv = EV(np.ones(den.v.shape, dtype=LD)) / den
    frozen = ~(np.isfinite(den.v) & (den.v > 0))
    out = []
    for n in range(3):
        num = ((a11 * s1[n] + a22 * s2[n]) + a33 * s3[n]) + ((a12 * m12[n] + a13 * m13[n]) + a23 * m23[n]).scale(2.0)
        if f is not None:
            f1, f2, f3 = (_ev(a) for a in f)
            num = num + (((a11 * f1) * r1[n] + (a22 * f2) * r2[n]) + (a33 * f3) * r3[n])
        frozen |= ~np.isfinite(num.v)
        new = num * inv
        out.append(c[n] + (new - c[n]) * _ev(omega))
    J = (r1[0] * (r2[1] * r3[2] - r2[2] * r3[1]) + r1[1] * (r2[2] * r3[0] - r2[0] * r3[2])) + r1[2] * (r2[0] * r3[1] - r2[1] * r3[0])
    return out, frozen, J


# (k, j, i) -> (q, p, t) of direction d and back
_TO = {0: (0, 1, 2), 1: (0, 2, 1), 2: (1, 2, 0)}
_BACK = {0: (0, 1, 2), 1: (0, 2, 1), 2: (2, 0, 1)}


def _line_phi(R):
    """R: three EV of shape (q, p, t) -> phi at t = 1 .. n-2, shape (q, p, n-2)"""
    rm = [EV(A.v[..., :-2], A.e[..., :-2]) for A in R]
    r0 = [EV(A.v[..., 1:-1], A.e[..., 1:-1]) for A in R]
    rp = [EV(A.v[..., 2:], A.e[..., 2:]) for A in R]
    d1 = [(rp[n] - rm[n]).scale(0.5) for n in range(3)]
    d2 = [(rp[n] - r0[n]) - (r0[n] - rm[n]) for n in range(3)]
    dd = _dot(d1, d1)
    ok = np.isfinite(dd.v) & (dd.v != 0)
    safe = EV(np.where(ok, dd.v, LD(1)), np.where(ok, dd.e, LD(0)))
    phi = -(_dot(d1, d2) / safe)
    return EV(np.where(ok, phi.v, LD(0)), np.where(ok, phi.e, LD(0)))


def control_field(planes):
    """-> f1, f2, f3 as EV over the interior nodes"""
    out = []
    for d in range(3):
        R = [EV(np.transpose(_ev(a).v, _TO[d]), np.transpose(_ev(a).e, _TO[d])) for a in planes]
        nq, np_, nt = R[0].v.shape
        phi = _line_phi(R)
        cut = lambda q, p: EV(phi.v[q, p, :], phi.e[q, p, :])   # noqa: E731
        mid, lo, hi = slice(1, -1), slice(0, 1), slice(-1, None)
        Fp0, Fp1, Fq0, Fq1 = cut(mid, lo), cut(mid, hi), cut(lo, mid), cut(hi, mid)
        E00, E10, E01, E11 = cut(lo, lo), cut(lo, hi), cut(hi, lo), cut(hi, hi)
        u = _ev(np.arange(1, np_ - 1, dtype=np.float64)[None, :, None]) / _ev(float(np_ - 1))
        v = _ev(np.arange(1, nq - 1, dtype=np.float64)[:, None, None]) / _ev(float(nq - 1))
        one = _ev(1.0)
        um, vm = one - u, one - v
        f = (((um * Fp0 + u * Fp1) + vm * Fq0) + v * Fq1) - ((((um * vm) * E00 + (u * vm) * E10) + (um * v) * E01) + (u * v) * E11)
        out.append(EV(np.transpose(f.v, _BACK[d]), np.transpose(f.e, _BACK[d])))
    return out


def worst_ratio(got, ref):
    """largest |got - ref| / bar over the entries (a zero error counts as 0 whatever the bar); <= 1 passes"""
    err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - ref.v)
    bar = ref.bar().astype(LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, LD(0), err / bar)
    assert not np.isnan(ratio).any()
    return float(ratio.max())


def interior(A):
    return np.asarray(A)[1:-1, 1:-1, 1:-1]


# ------------------------------------------------------------------ blocks
def tanh_one_sided(n, beta):
    u = np.linspace(0.0, 1.0, n)
    return 1.0 + np.tanh(beta * (u - 1.0)) / np.tanh(beta)


def bent_clustered3(ni, nj, nk):
    """The 3-D analogue of control_field_reference.bent_clustered: all six faces curved, nodes clustered towards j = 0 and k = 0, two-sided
    in i; smooth maps, no two nodes coincide."""
    ui = np.linspace(-1.0, 1.0, ni)
    a = (0.5 * (1.0 + np.tanh(1.5 * ui) / np.tanh(1.5)))[None, None, :]
    b = tanh_one_sided(nj, 2.0)[None, :, None]
    c = tanh_one_sided(nk, 1.6)[:, None, None]
    X = -0.3 + 1.7 * a + 0.11 * np.sin(2.0 * b + 0.3) * (1 + a) + 0.06 * np.cos(2.0 * c) * b
    Y = 0.2 + 0.9 * b + 0.07 * np.sin(3.0 * a) * (1.0 - b) + 0.05 * a * a * b + 0.08 * np.sin(2.5 * c + 0.2) * (1 + a)
    Z = 0.1 + 1.1 * c + 0.09 * np.sin(2.0 * a + 1.0) * (1.0 - c) + 0.06 * b * b * c + 0.04 * a * b
    return tuple(np.ascontiguousarray(np.broadcast_to(A, (nk, nj, ni))) for A in (X, Y, Z))


# a non-orthogonal affine map; small integers, so the image of an integer lattice is exact in fp64
AFFINE = np.array([[1.0, 0.25, 0.125], [0.5, 1.0, -0.25], [-0.125, 0.375, 1.0]])
ORIGIN = np.array([0.5, -1.0, 2.0])


def affine_of(U, V, W):
    """the affine image of the tensor-product block (U(i), V(j), W(k)) as (nk, nj, ni) planes"""
    u, v, w = np.asarray(U)[None, None, :], np.asarray(V)[None, :, None], np.asarray(W)[:, None, None]
    shape = (w.size, v.size, u.size)
    return tuple(np.ascontiguousarray(np.broadcast_to(ORIGIN[c] + AFFINE[c, 0] * u + AFFINE[c, 1] * v + AFFINE[c, 2] * w, shape)) for c in range(3))


def affine_lattice(ni=9, nj=8, nk=7):
    return affine_of(np.arange(ni, dtype=np.float64), np.arange(nj, dtype=np.float64), np.arange(nk, dtype=np.float64))


def noisy_lattice(ni=9, nj=8, nk=7, amplitude=0.6, seed=7):
    """the affine lattice, every lattice coordinate of every interior node moved by +amplitude or -amplitude cells (seeded coin flips).
    Two-valued on purpose: the record counts the sign of the Jacobian of the CENTRAL differences, which uniform noise of the same
    amplitude turns negative at no node in sixty seeds, while it inverts over a hundred hexahedra either way."""
    rng = np.random.default_rng(seed)
    I, J, K = np.meshgrid(np.arange(ni, dtype=np.float64), np.arange(nj, dtype=np.float64), np.arange(nk, dtype=np.float64), indexing="ij")
    lat = [np.ascontiguousarray(A.transpose(2, 1, 0)) for A in (I, J, K)]
    for A in lat:
        A[1:-1, 1:-1, 1:-1] += amplitude * rng.choice([-1.0, 1.0], size=(nk - 2, nj - 2, ni - 2))
    return tuple(np.ascontiguousarray(ORIGIN[c] + AFFINE[c, 0] * lat[0] + AFFINE[c, 1] * lat[1] + AFFINE[c, 2] * lat[2]) for c in range(3))


def clustered_tensor(ni=17, nj=13, nk=9):
    """(X(i), Y(j), Z(k)) under the affine map: X uniform, Y one-sided tanh towards j = 0, Z a power law"""
    return affine_of(np.linspace(0.0, 1.0, ni), tanh_one_sided(nj, 3.0), np.linspace(0.0, 1.0, nk) ** 1.5)


def first_cell(planes):
    """mean length of the first edge at j = 0 over the interior (i, k)"""
    X, Y, Z = planes
    d = np.sqrt((X[:, 1] - X[:, 0]) ** 2 + (Y[:, 1] - Y[:, 0]) ** 2 + (Z[:, 1] - Z[:, 0]) ** 2)
    return float(d[1:-1, 1:-1].mean())
