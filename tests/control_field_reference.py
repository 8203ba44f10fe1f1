"""Reference of the Thomas-Middlecoff control field in numpy longdouble, written from the definition (include/tm_hip.h), and
the meshes the control-field tests share.

Edge function of a polyline e[0..n-1], interior points k = 1..n-2:
    d1 = (e[k+1] - e[k-1]) / 2,  d2 = e[k+1] - 2 e[k] + e[k-1],  f[k] = -(d1.d2) / (d1.d1)   (0 where d1.d1 == 0)
    f[0] = f[1], f[n-1] = f[n-2];  n < 3: f = 0
Blend, r[i][j] stored (ni, nj, 2) with j fastest, P with i and Q with j:
    phi_lo = f(r[.][0]), phi_hi = f(r[.][nj-1]), psi_lo = f(r[0][.]), psi_hi = f(r[ni-1][.])
    P[i][j] = (1-t) phi_lo[i] + t phi_hi[i], t = j/(nj-1);   Q[i][j] = (1-s) psi_lo[j] + s psi_hi[j], s = i/(ni-1)

The "absolute" variant has |d1x d2x| + |d1y d2y| in the numerator (no sign), blended the same way: the scale the rounding errors of the
signed expression are relative to -- the bar of the device comparison is 16 eps x absolute + eps |reference| per node and component."""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


def _second_difference(e):
    """e[k+1] - 2 e[k] + e[k-1] for k = 1..n-2, the expression of the definition evaluated WITHOUT rounding (rational arithmetic on the
    fp64 coordinates) and then rounded once to longdouble.  Summed in longdouble the expression carries an error of 2^-64 |e|, and along an
    edge of nearly uniform points |d2| is down to 1e-16 |e| -- the reference would be wrong in the sixth digit where the bar is 16 eps."""
    from fractions import Fraction

    e64 = np.asarray(e, dtype=np.float64)
    out = np.zeros((e64.shape[0] - 2, 2), dtype=LD)
    for k in range(1, e64.shape[0] - 1):
        for c in range(2):
            d = Fraction(float(e64[k + 1, c])) - 2 * Fraction(float(e64[k, c])) + Fraction(float(e64[k - 1, c]))
            hi = float(d)
            out[k - 1, c] = LD(hi) + LD(float(d - Fraction(hi)))
    return out


def edge_function(e, absolute=False):
    assert np.asarray(e).dtype == np.float64   # the coordinates as the device holds them
    e = np.asarray(e, dtype=LD)
    n = e.shape[0]
    f = np.zeros(n, dtype=LD)
    if n < 3:
        return f
    d1 = (e[2:] - e[:-2]) / LD(2)
    d2 = _second_difference(e)
    den = d1[:, 0] * d1[:, 0] + d1[:, 1] * d1[:, 1]
    num = np.abs(d1[:, 0] * d2[:, 0]) + np.abs(d1[:, 1] * d2[:, 1]) if absolute else -(d1[:, 0] * d2[:, 0] + d1[:, 1] * d2[:, 1])
    ok = den != 0
    f[1:-1][ok] = num[ok] / den[ok]
    f[0], f[-1] = f[1], f[-2]
    return f


def block_field(r, absolute=False):
    """(ni, nj, 2) longdouble: [..., 0] = P, [..., 1] = Q."""
    r = np.asarray(r, dtype=np.float64)
    ni, nj = r.shape[:2]
    phi_lo, phi_hi = edge_function(r[:, 0], absolute), edge_function(r[:, nj - 1], absolute)
    psi_lo, psi_hi = edge_function(r[0, :], absolute), edge_function(r[ni - 1, :], absolute)
    t = (np.arange(nj, dtype=LD) / LD(nj - 1))[None, :]
    s = (np.arange(ni, dtype=LD) / LD(ni - 1))[:, None]
    out = np.empty((ni, nj, 2), dtype=LD)
    out[..., 0] = (LD(1) - t) * phi_lo[:, None] + t * phi_hi[:, None]
    out[..., 1] = (LD(1) - s) * psi_lo[None, :] + s * psi_hi[None, :]
    return out


def mesh_field(blocks, absolute=False):
    """Flat (dof, 2) longdouble over a list of (ni, nj, 2) arrays, block after block: the layout of tm_smoother_control_function."""
    return np.concatenate([block_field(b, absolute).reshape(-1, 2) for b in blocks], axis=0)


def check_against_reference(dev, blocks):
    """The bar of the device comparison; returns the largest |dev - ref| / bar over the nodes (<= 1 passes)."""
    ref, scale = mesh_field(blocks), mesh_field(blocks, absolute=True)
    bar = 16 * LD(EPS) * scale + LD(EPS) * np.abs(ref)
    err = np.abs(np.asarray(dev, dtype=LD) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, LD(0), err / bar)
    return float(ratio.max())


# ------------------------------------------------------------------ meshes
def tanh_two_sided(n, beta=2.0):
    u = np.linspace(-1.0, 1.0, n)
    return 0.5 * (1.0 + np.tanh(beta * u) / np.tanh(beta))


def tanh_one_sided(n, beta=2.5):
    u = np.linspace(0.0, 1.0, n)
    return 1.0 + np.tanh(beta * (u - 1.0)) / np.tanh(beta)


# The "bent rectangle" of the tests: wall clustering and bend chosen so that Laplace smoothing lets the first cell at the wall grow about
# 25-fold at mid-chord (the loss the field is there to prevent), with a bend of 7.5 % of the height
BEND = 0.075
WALL_BETA = 3.25


def rectangle(ni=33, nj=25, bend=0.0):
    """(ni, nj, 2): i lines tanh-clustered towards both ends, j lines towards the lower wall j = 0, the lower wall bent by
    bend * sin(pi x) (the bend decays linearly to the flat upper wall).  bend = 0: separable, x = x(i), y = y(j)."""
    x, y = tanh_two_sided(ni), tanh_one_sided(nj, WALL_BETA)
    r = np.empty((ni, nj, 2))
    r[..., 0] = x[:, None]
    wall = bend * np.sin(np.pi * x)[:, None]
    r[..., 1] = wall + (1.0 - wall) * y[None, :]
    return r


def bent_clustered(ni, nj, seed=0):
    """A block whose four edges are all curved and non-uniformly spaced, interior by transfinite interpolation of smooth maps (no
    two nodes coincide): what the field pin runs on at every size."""
    a = tanh_two_sided(ni, 1.5 + 0.1 * seed)[:, None] if ni > 2 else np.linspace(0, 1, ni)[:, None]
    b = tanh_one_sided(nj, 2.0)[None, :] if nj > 2 else np.linspace(0, 1, nj)[None, :]
    r = np.empty((ni, nj, 2))
    r[..., 0] = -0.3 + 1.7 * a + 0.11 * np.sin(2.0 * b + 0.3) * (1 + a)
    r[..., 1] = 0.2 + 0.9 * b + 0.07 * np.sin(3.0 * a) * (1.0 - b) + 0.05 * a * a * b
    return r


def first_cell_height_ratio(r, seed):
    """Height of the first cell at the lower wall j = 0 against the seed's, per interior i."""
    h = np.linalg.norm(r[1:-1, 1] - r[1:-1, 0], axis=1)
    h0 = np.linalg.norm(seed[1:-1, 1] - seed[1:-1, 0], axis=1)
    return h / h0


def single_block_mesh(r):
    from turbomesh_amd import configs
    from turbomesh_amd.discrete import Mesh

    m = Mesh()
    m.addBlock("block_0", configs.block_from_array(np.ascontiguousarray(r).copy()))
    return m


class OracleBlocks:
    """Duck-typed oracle mesh of unconnected blocks given as arrays."""

    def __init__(self, blocks):
        self.blocks = [np.array(b, dtype=np.float64, order="C", copy=True) for b in blocks]
        self.connections = []
        self.bcs = []


class field_in_oracle:
    """Context manager: inside it every oracle.System (oracle.picard_exact builds its own) starts with `field` -- a flat (dof, 2) array, or
    a callable(blocks) evaluated on the mesh the System is created for -- written into its control_function view.  With the Laplace
    algorithm the oracle allocates that array as zeros, reads it in every fill and never updates it: the exact Picard iteration of a
    frozen prescribed field."""

    def __init__(self, field):
        self.field = field

    def __enter__(self):
        from oracle import oracle

        field = self.field
        self._oracle, self._orig = oracle, oracle.System

        class FieldSystem(self._orig):
            def __init__(self, mesh, control=None):
                super().__init__(mesh, None)
                f = field(mesh.blocks) if callable(field) else field
                self.control_function[:] = np.asarray(f, dtype=np.float64)

        oracle.System = FieldSystem
        return self

    def __exit__(self, *exc):
        self._oracle.System = self._orig


def tm_field64(blocks):
    """The reference field rounded to fp64 (what goes into the oracle)."""
    return mesh_field(blocks).astype(np.float64)
