"""Spanwise stacking: K smoothed 2-D cuts -> the blocks of a 3-D mesh (include/tm_hip.h, "3-D from 2-D cuts"; the reference's roadmap
items "extension to 3D based on meshed 2d cuts" and "rotational configurations").

A layer k of a 3-D block is a fixed linear combination of the same node in the K cuts, v[k] = sum_c A[k][c] v_c: linear or
natural-cubic-spline weights from the span positions alone, planar (x, y, s) or cylindrical (x, r sin(theta), r cos(theta)) output.

    st = Stack(span=[0.0, 0.5, 1.0], layers=layers_from([0.0, 0.5, 1.0], 33))
    X, Y, Z = st.block(cuts, b)            # cuts: a list of Mesh (uploaded per call) or of Smoother (resident coordinates)
    st.mesh3d(cuts).write("blade.xyz")     # multi-block 3-D PLOT3D

Cuts meshed in the unrolled plane (u, v) of stream surfaces of revolution -- contoured end walls, mixed-flow and radial stages -- take
mapping="revolution" and one meridional table x(u), r(u) per cut ("cuts on stream surfaces of revolution" in the header):

    sf = Surfaces(u=[u0, u1], x=[x0, x1], r=[r0, r1], rref=[0.3, 0.5])       # meridional_from_contour gives u from a contour (x, r)
    st = Stack(span, layers, mapping="revolution", surfaces=sf)

Curved hexahedra of order p <= 4 come from the same cuts ("high-order hexahedra of stacked blocks" in the header, kernel K16), the layers
agglomerated in span as the nodes are in-plane; the layer count minus one must be a multiple of p like the cell counts of the blocks:

    X, Y, Z, q, sj = st.elevate(cuts, highorder.Elevation(2), b)          # planes, quality.HoQuality3d, scaled Jacobian per element
    st.mesh3d_ho(cuts, highorder.Elevation(2, "equidistant")).write("blade.vtk")

Those hexahedra are judged at their nodes; Stack.certify bounds their Jacobian on the whole element ("high-order hexahedra: certificate" in
the header, kernel K17):

    cert, status, bounds = st.certify(cuts, highorder.Elevation(2), b, max_depth=2)   # quality.HoCertificate3d, (Eg, Ej, Ei) status, (lo, hi)

Evaluated on the MI355X (kernels K11, K16, K17); `host=True` evaluates the same definition on the CPU (lists of Mesh only)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Tuple

import numpy as np

from . import _capi
from . import clustering as cluster

INTERPOLATION = {"linear": _capi.TM_STACK_LINEAR, "cubic": _capi.TM_STACK_CUBIC}
MAPPING = {"planar": _capi.TM_STACK_PLANAR, "cylindrical": _capi.TM_STACK_CYLINDRICAL, "revolution": _capi.TM_STACK_REVOLUTION}
SURFACE_INTERPOLATION = {"linear": _capi.TM_SURF_LINEAR, "cubic": _capi.TM_SURF_CUBIC}


def layers_from(span, nk, clustering=None):
    """nk layer coordinates over the span of the cuts: s_k = z0 + u_k (z_{K-1} - z0), u = clustering.create(clustering, nk) (uniform by
    default); the end layers are z0 and z_{K-1} exactly, so they reproduce the end cuts.  nk = 1 gives the single layer z0."""
    z = np.asarray(span, dtype=np.float64)
    if z.ndim != 1 or z.size < 2:
        raise ValueError("span: at least two cut positions")
    if nk < 1:
        raise ValueError("at least one layer")
    if nk == 1:
        return np.array([z[0]])
    u = np.asarray(cluster.create(clustering if clustering is not None else cluster.Uniform(), nk), dtype=np.float64)
    s = np.clip(z[0] + u * (z[-1] - z[0]), z[0], z[-1])
    s[0], s[-1] = z[0], z[-1]
    return s


def meridional_from_contour(x, r, rref):
    """The conformal parameter u of a meridional contour polyline (x_n, r_n): u_0 = 0, u_n = u_{n-1} + rref dm ln(r_n / r_{n-1}) /
    (r_n - r_{n-1}) with dm the segment's length (the factor is 1 / r_n where the two radii are equal) -- rref times the integral of
    dm / r along straight segments.  Host only, in longdouble, rounded once.  With it a cut meshed angle-preserving in (u, v = rref theta)
    maps angle-preserving onto the surface; the u column of a hub or shroud table comes from here."""
    LD = np.longdouble
    x, r = np.asarray(x, dtype=np.float64).astype(LD).reshape(-1), np.asarray(r, dtype=np.float64).astype(LD).reshape(-1)
    if x.size != r.size or x.size < 2:
        raise ValueError("a contour needs at least two points (x_n, r_n)")
    if not np.all(r > 0) or not float(rref) > 0:
        raise ValueError("radii and the reference radius must be > 0")
    dx, dr = np.diff(x), np.diff(r)
    dm = np.sqrt(dx * dx + dr * dr)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(dr == 0, 1 / r[1:], np.log(r[1:] / r[:-1]) / np.where(dr == 0, LD(1), dr))
    u = np.concatenate([[LD(0)], np.cumsum(LD(np.float64(rref)) * dm * f)])
    return np.asarray(u, dtype=np.float64)


class Surfaces:
    """tm_stack_surfaces: one meridional table per cut, lists of per-cut arrays u (strictly increasing), x, r (> 0), 2 .. 256 knots each,
    the counts may differ between cuts.  rref: one reference radius per cut (None: the span coordinates of the Stack, which must then be
    > 0).  interpolation: of x(u) and r(u) along the curve, "linear" or "cubic" (the natural spline)."""

    def __init__(self, u, x, r, rref=None, interpolation="cubic"):
        if interpolation not in SURFACE_INTERPOLATION:
            raise ValueError(f"interpolation {interpolation!r}: one of {sorted(SURFACE_INTERPOLATION)}")
        if not (len(u) == len(x) == len(r)):
            raise ValueError("u, x, r: one array per cut each")
        self.u = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in u]
        self.x = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in x]
        self.r = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in r]
        for a, b, c in zip(self.u, self.x, self.r):
            if not (a.size == b.size == c.size):
                raise ValueError("the u, x and r columns of a cut differ in length")
        self.rref = None if rref is None else np.ascontiguousarray(rref, dtype=np.float64).reshape(-1)
        if self.rref is not None and self.rref.size != len(self.u):
            raise ValueError(f"{self.rref.size} reference radii for {len(self.u)} cuts")
        self.interpolation = interpolation
        K = len(self.u)
        self._nknots = np.array([a.size for a in self.u], dtype=np.uint64)
        cols = lambda arrs: (C.POINTER(C.c_double) * max(1, K))(*[_capi.f64ptr(a) for a in arrs])   # noqa: E731
        self._cols = [cols(self.u), cols(self.x), cols(self.r)]
        self._struct = _capi.tm_stack_surfaces(K, self._nknots.ctypes.data_as(C.POINTER(C.c_uint64)), *self._cols,
                                               None if self.rref is None else _capi.f64ptr(self.rref), SURFACE_INTERPOLATION[interpolation], 0)

    @property
    def ncuts(self):
        return len(self.u)

    def ref(self):
        return C.byref(self._struct)

    @classmethod
    def read(cls, files, rref=None, interpolation="cubic"):
        """One text file per cut, rows `u x r`, `#` comments and blank lines skipped, blanks, commas or semicolons between the numbers."""
        cols = []
        for f in files:
            rows = []
            with open(f) as fh:
                for ln, line in enumerate(fh, 1):
                    line = line.split("#", 1)[0].strip()
                    if not line:
                        continue
                    parts = line.replace(",", " ").replace(";", " ").split()
                    try:
                        row = [float(p) for p in parts]
                    except ValueError:
                        row = []
                    if len(row) != 3:
                        raise ValueError(f"{f}:{ln}: a row of a meridional table is `u x r`")
                    rows.append(row)
            if len(rows) < 2:
                raise ValueError(f"{f}: a meridional table needs at least two rows")
            cols.append(np.array(rows, dtype=np.float64))
        return cls([a[:, 0] for a in cols], [a[:, 1] for a in cols], [a[:, 2] for a in cols], rref, interpolation)


def quality_of_planes(X, Y, Z, block=0, field=False):
    """quality.Quality3d of any 3-D block given as (nk, nj, ni) arrays (PLOT3D order: what Stack.block returned, or a file read with
    output.read_plot3d_3d), evaluated on the CPU (tm_quality3d_planes_host: no GPU needed).  field=True: (record, per-cell min of the
    oriented scaled Jacobian as a (nk-1, nj-1, ni-1) array)."""
    from . import quality as _quality

    X, Y, Z = (np.ascontiguousarray(a, dtype=np.float64) for a in (X, Y, Z))
    if X.ndim != 3 or Y.shape != X.shape or Z.shape != X.shape:
        raise ValueError("X, Y, Z: three (nk, nj, ni) arrays of one shape")
    nk, nj, ni = X.shape
    q = _capi.tm_quality3d()
    f = np.empty((max(0, nk - 1), max(0, nj - 1), max(0, ni - 1)), dtype=np.float64) if field else None
    _capi.check(_capi.lib().tm_quality3d_planes_host(_capi.f64ptr(X), _capi.f64ptr(Y), _capi.f64ptr(Z), ni, nj, nk, block, C.byref(q),
                                                     _capi.f64ptr(f) if field else None))
    rec = _quality.Quality3d.from_struct(q)
    return (rec, f) if field else rec


SMOOTH_ALGORITHM = {"laplace": _capi.TM_S3_LAPLACE, "thomas-middlecoff": _capi.TM_S3_THOMAS_MIDDLECOFF, "prescribed": _capi.TM_S3_PRESCRIBED}


@dataclass
class Smooth3dInfo:
    """tm_smooth3d_info as a record ("elliptic smoothing of stacked blocks" in the header): counts over the interior nodes, the sign of
    the Jacobian J of the central differences in the input of the first and of the last sweep, the updates of those two sweeps."""

    nodes: int
    interior: int
    sweeps_done: int
    frozen: int
    first_neg: int
    first_pos: int
    first_zero_or_nan: int
    last_neg: int
    last_pos: int
    last_zero_or_nan: int
    last_max_node: int           # flat index (k*nj + j)*ni + i; -1: none
    first_sum_sq: float
    last_sum_sq: float
    last_max_update: float
    control_max: Tuple[float, float, float]

    @classmethod
    def from_struct(cls, s: "_capi.tm_smooth3d_info") -> "Smooth3dInfo":
        node = int(s.last_max_node)
        return cls(int(s.nodes), int(s.interior), int(s.sweeps_done), int(s.frozen), int(s.first_neg), int(s.first_pos), int(s.first_zero_or_nan),
                   int(s.last_neg), int(s.last_pos), int(s.last_zero_or_nan), -1 if node == 2 ** 64 - 1 else node, float(s.first_sum_sq),
                   float(s.last_sum_sq), float(s.last_max_update), tuple(float(v) for v in s.control_max))

    @property
    def last_rms_update(self) -> float:
        return float(np.sqrt(self.last_sum_sq / self.interior)) if self.interior else 0.0

    def line(self, name: str) -> str:
        return (f"{name}: sweeps {self.sweeps_done} interior {self.interior} frozen {self.frozen} "
                f"J<0 {self.first_neg} -> {self.last_neg} J=0/nan {self.first_zero_or_nan} -> {self.last_zero_or_nan} "
                f"rms update {self.last_rms_update:.3e} max update {self.last_max_update:.3e} at node {self.last_max_node} "
                f"max |f| {self.control_max[0]:.3e} {self.control_max[1]:.3e} {self.control_max[2]:.3e}")


def log_smooth3d(logger, names, per_block, stage="stack-smooth"):
    """One line per block on `logger` at INFO; every line starts with `stage`."""
    for name, r in zip(names, per_block):
        logger.info("%s", r.line(f"{stage} {name}"))


def _planes_in(X, Y, Z):
    X, Y, Z = (np.array(a, dtype=np.float64, order="C") for a in (X, Y, Z))   # copies: the call works in place
    if X.ndim != 3 or Y.shape != X.shape or Z.shape != X.shape:
        raise ValueError("X, Y, Z: three (nk, nj, ni) arrays of one shape")
    return X, Y, Z


def _smooth_opt(shape, sweeps, algorithm, omega, tol, control):
    """(tm_smooth3d_opt, the arrays it points to)"""
    if algorithm not in SMOOTH_ALGORITHM:
        raise ValueError(f"algorithm {algorithm!r}: one of {sorted(SMOOTH_ALGORITHM)}")
    if sweeps < 0:
        raise ValueError("sweeps >= 0")
    keep = []
    if algorithm == "prescribed" and control is not None:
        keep = [np.ascontiguousarray(a, dtype=np.float64) for a in control]
        if len(keep) != 3 or any(a.shape != tuple(shape) for a in keep):
            raise ValueError("control: three arrays of the shape of the planes")
    ptrs = [_capi.f64ptr(a) for a in keep] if keep else [None] * 3
    return _capi.tm_smooth3d_opt(SMOOTH_ALGORITHM[algorithm], 0, int(sweeps), float(omega), float(tol), *ptrs), keep


def smooth_planes(X, Y, Z, sweeps, algorithm="thomas-middlecoff", omega=1.0, tol=0.0, host=False, control=None):
    """`sweeps` Jacobi sweeps of the 3-D Winslow equations on a block given as (nk, nj, ni) arrays, its six faces held ("elliptic smoothing
    of stacked blocks" in the header, kernel K22) -> (X, Y, Z, Smooth3dInfo); the arguments are not modified.  algorithm: "laplace",
    "thomas-middlecoff" (the control field that keeps wall clustering, formed from the input block) or "prescribed" (control=(f1, f2, f3),
    arrays of the planes' shape).  tol > 0 ends the call once the rms update is <= tol (tested behind every 8th sweep).  On the MI355X
    (tm_smooth3d_planes); host=True: the same definition on the CPU (tm_smooth3d_planes_host, no GPU)."""
    X, Y, Z = _planes_in(X, Y, Z)
    nk, nj, ni = X.shape
    opt, keep = _smooth_opt(X.shape, sweeps, algorithm, omega, tol, control)
    info = _capi.tm_smooth3d_info()
    L = _capi.lib()
    _capi.check((L.tm_smooth3d_planes_host if host else L.tm_smooth3d_planes)(ni, nj, nk, _capi.f64ptr(X), _capi.f64ptr(Y), _capi.f64ptr(Z), C.byref(opt),
                                                                              C.byref(info)))
    del keep
    return X, Y, Z, Smooth3dInfo.from_struct(info)


def control_of_planes(X, Y, Z, host=False):
    """The Thomas-Middlecoff control field (f1, f2, f3) of a block given as (nk, nj, ni) arrays, 0 on every node that is not interior
    (tm_smooth3d_control; host=True: tm_smooth3d_control_host, no GPU)."""
    X, Y, Z = _planes_in(X, Y, Z)
    nk, nj, ni = X.shape
    f = [np.empty_like(X) for _ in range(3)]
    L = _capi.lib()
    _capi.check((L.tm_smooth3d_control_host if host else L.tm_smooth3d_control)(ni, nj, nk, _capi.f64ptr(X), _capi.f64ptr(Y), _capi.f64ptr(Z),
                                                                                *[_capi.f64ptr(a) for a in f]))
    return tuple(f)


@dataclass
class Mesh3d:
    """Blocks of a stacked mesh: per block the X, Y, Z coordinates as (nk, nj, ni) arrays (PLOT3D order, i fastest)."""

    names: List[str] = field(default_factory=list)
    blocks: List[Tuple[np.ndarray, np.ndarray, np.ndarray]] = field(default_factory=list)

    def sizes(self):
        return [(x.shape[2], x.shape[1], x.shape[0]) for x, _, _ in self.blocks]

    def smooth(self, sweeps, algorithm="thomas-middlecoff", omega=1.0, tol=0.0, host=False):
        """smooth_planes on every block, in place; -> the per-block Smooth3dInfo.  The faces of a block are held, so blocks stay conforming."""
        records = []
        for b, (X, Y, Z) in enumerate(self.blocks):
            X, Y, Z, info = smooth_planes(X, Y, Z, sweeps, algorithm, omega, tol, host)
            self.blocks[b] = (X, Y, Z)
            records.append(info)
        return records

    def write(self, filename):
        """Multi-block 3-D PLOT3D (output.write_plot3d_3d)."""
        from . import output

        output._format_of(filename)
        output.write_plot3d_3d(filename, self.sizes(), self.blocks)


class Stack:
    """tm_stack_opt + the calls that take it."""

    def __init__(self, span, layers, interpolation="cubic", mapping="planar", surfaces=None):
        if interpolation not in INTERPOLATION:
            raise ValueError(f"interpolation {interpolation!r}: one of {sorted(INTERPOLATION)}")
        if mapping not in MAPPING:
            raise ValueError(f"mapping {mapping!r}: one of {sorted(MAPPING)}")
        if (mapping == "revolution") != (surfaces is not None):
            raise ValueError("mapping='revolution' takes surfaces=Surfaces(...), and only it does")
        self.surfaces = surfaces
        self.span = np.ascontiguousarray(span, dtype=np.float64).reshape(-1)
        self.layers = np.ascontiguousarray(layers, dtype=np.float64).reshape(-1)
        self.interpolation, self.mapping = interpolation, mapping
        self._opt = _capi.tm_stack_opt(self.span.size, _capi.f64ptr(self.span), self.layers.size, _capi.f64ptr(self.layers),
                                       INTERPOLATION[interpolation], MAPPING[mapping])

    @property
    def ncuts(self):
        return int(self.span.size)

    @property
    def nlayers(self):
        return int(self.layers.size)

    def weights(self):
        """The (nlayers, ncuts) weight matrix (tm_stack_weights: host only)."""
        w = np.empty((max(1, self.nlayers), max(1, self.ncuts)), dtype=np.float64)
        opt = self._opt
        if self.surfaces is not None:   # A depends on span, layers and interpolation alone; tm_stack_weights has no tables and refuses mapping 2
            opt = _capi.tm_stack_opt(opt.ncuts, opt.span, opt.nlayers, opt.layers, opt.interpolation, _capi.TM_STACK_PLANAR)
        _capi.check(_capi.lib().tm_stack_weights(C.byref(opt), _capi.f64ptr(w)))
        return w[:self.nlayers, :self.ncuts]

    def surface_tables(self):
        """Per cut the (nknots - 1, 8) coefficients ax bx cx dx ar br cr dr of its intervals (tm_stack_surface_tables: host only)."""
        if self.surfaces is None:
            raise ValueError("surface_tables: only with mapping='revolution'")
        n = [max(0, int(a.size) - 1) for a in self.surfaces.u]
        out = np.empty(max(1, 8 * sum(n)), dtype=np.float64)
        _capi.check(_capi.lib().tm_stack_surface_tables(C.byref(self._opt), self.surfaces.ref(), _capi.f64ptr(out)))
        off = np.concatenate([[0], np.cumsum(n)])
        return [out[8 * off[c]:8 * off[c + 1]].reshape(-1, 8).copy() for c in range(len(n))]

    def _check_count(self, cuts):
        if len(cuts) != self.ncuts:
            raise ValueError(f"{len(cuts)} cuts for {self.ncuts} span positions")

    def block(self, cuts, b, k_begin=0, k_count=None, host=False, return_outside=False):
        """Layers [k_begin, k_begin + k_count) of block b as three (k_count, nj, ni) arrays.  cuts: one discrete.Mesh per cut (host
        coordinates, uploaded per call: tm_stack_block; host=True: tm_stack_block_host, no GPU) or one smooth.Smoother per cut (the
        coordinates resident in the handles: tm_stack_smoothers).  mapping="revolution" routes to the *_surf calls; return_outside=True
        then adds a fourth entry, per cut the number of the block's nodes whose u lies outside the cut's table (extrapolated)."""
        self._check_count(cuts)
        sf = self.surfaces
        if return_outside and sf is None:
            raise ValueError("return_outside: only with mapping='revolution'")
        outside = np.zeros(max(1, self.ncuts), dtype=np.uint64)
        extra = () if sf is None else (outside.ctypes.data_as(C.POINTER(C.c_uint64)) if return_outside else None,)
        head = lambda a: (a, C.byref(self._opt)) + (() if sf is None else (sf.ref(),))   # noqa: E731
        if k_count is None:
            k_count = self.nlayers - k_begin
        resident = all(hasattr(c, "_h") for c in cuts)
        meshes = [c._mesh for c in cuts] if resident else cuts
        ni, nj = meshes[0].blocks[b].points.size
        out = [np.empty((max(0, k_count), nj, ni), dtype=np.float64) for _ in range(3)]
        ptrs = [_capi.f64ptr(o) for o in out]
        L = _capi.lib()
        if resident:
            if host:
                raise ValueError("host=True evaluates host coordinates: pass the meshes, not the handles")
            handles = (C.c_void_p * len(cuts))(*[c._h for c in cuts])
            _capi.check((L.tm_stack_smoothers if sf is None else L.tm_stack_smoothers_surf)(*head(handles), b, k_begin, k_count, *ptrs, *extra))
        else:
            descs = [_capi.MeshDesc(m) for m in meshes]
            arr = (C.POINTER(_capi.tm_mesh_desc) * len(descs))(*[C.pointer(d.desc) for d in descs])
            if sf is None:
                fn = L.tm_stack_block_host if host else L.tm_stack_block
            else:
                fn = L.tm_stack_block_surf_host if host else L.tm_stack_block_surf
            _capi.check(fn(*head(arr), b, k_begin, k_count, *ptrs, *extra))
        return tuple(out) + ((outside[:self.ncuts].copy(),) if return_outside else ())

    def smooth(self, cuts, b, sweeps, algorithm="thomas-middlecoff", omega=1.0, tol=0.0, host=False, control=None):
        """(X, Y, Z, Smooth3dInfo): all layers of block b, stacked and then smoothed with its six faces held (smooth_planes).  cuts as in
        block(): one smooth.Smoother per cut -- stacked into a device buffer and smoothed there, only planes and record cross to the
        host, no handle is modified (tm_stack_smoothers_smooth) -- or one discrete.Mesh per cut (block(), then smooth_planes;
        host=True: both on the CPU)."""
        self._check_count(cuts)
        resident = all(hasattr(c, "_h") for c in cuts)
        if not resident:
            return smooth_planes(*self.block(cuts, b, host=host), sweeps, algorithm, omega, tol, host, control)
        if host:
            raise ValueError("host=True evaluates host coordinates: pass the meshes, not the handles")
        ni, nj = cuts[0]._mesh.blocks[b].points.size
        out = [np.empty((self.nlayers, nj, ni), dtype=np.float64) for _ in range(3)]
        opt, keep = _smooth_opt(out[0].shape, sweeps, algorithm, omega, tol, control)
        info = _capi.tm_smooth3d_info()
        handles = (C.c_void_p * len(cuts))(*[c._h for c in cuts])
        sf = self.surfaces
        L = _capi.lib()
        if sf is None:
            _capi.check(L.tm_stack_smoothers_smooth(handles, C.byref(self._opt), b, C.byref(opt), *[_capi.f64ptr(o) for o in out], C.byref(info)))
        else:
            _capi.check(L.tm_stack_smoothers_smooth_surf(handles, C.byref(self._opt), sf.ref(), b, C.byref(opt), *[_capi.f64ptr(o) for o in out], C.byref(info)))
        del keep
        return out[0], out[1], out[2], Smooth3dInfo.from_struct(info)

    def quality(self, cuts, host=False):
        """(per_block, total): the 3-D quality report of every stacked block (quality.Quality3d) and their total -- negative and degenerate
        hexahedra ACROSS layers, which the 2-D report of the cuts cannot see.  Evaluated on the device straight from the cuts (kernel K12:
        the 3-D block is never stored); cuts as in block(): Mesh (tm_stack_quality; host=True: tm_stack_quality_host, no GPU) or Smoother
        (tm_stack_smoothers_quality, the resident coordinates)."""
        from . import quality as _quality

        self._check_count(cuts)
        resident = all(hasattr(c, "_h") for c in cuts)
        meshes = [c._mesh for c in cuts] if resident else cuts
        L = _capi.lib()
        sf = self.surfaces
        head = lambda a: (a, C.byref(self._opt)) + (() if sf is None else (sf.ref(),))   # noqa: E731
        per_block = []
        if resident:
            if host:
                raise ValueError("host=True evaluates host coordinates: pass the meshes, not the handles")
            handles = (C.c_void_p * len(cuts))(*[c._h for c in cuts])
        else:
            descs = [_capi.MeshDesc(m) for m in meshes]
            arr = (C.POINTER(_capi.tm_mesh_desc) * len(descs))(*[C.pointer(d.desc) for d in descs])
        for b in range(len(meshes[0].blocks)):
            q = _capi.tm_quality3d()
            if resident:
                _capi.check((L.tm_stack_smoothers_quality if sf is None else L.tm_stack_smoothers_quality_surf)(*head(handles), b, C.byref(q)))
            elif sf is None:
                _capi.check((L.tm_stack_quality_host if host else L.tm_stack_quality)(*head(arr), b, C.byref(q)))
            else:
                _capi.check((L.tm_stack_quality_surf_host if host else L.tm_stack_quality_surf)(*head(arr), b, C.byref(q)))
            per_block.append(_quality.Quality3d.from_struct(q))
        return per_block, _quality.total_3d(per_block)

    def quality_field(self, cuts, b, k_begin=0, k_count=None):
        """Per-cell minimum of the oriented scaled Jacobian of block b, cell layers [k_begin, k_begin + k_count), as a (k_count, nj-1, ni-1)
        array (NaN for degenerate cells).  cuts: one smooth.Smoother per cut (tm_stack_smoothers_quality_field)."""
        self._check_count(cuts)
        if not all(hasattr(c, "_h") for c in cuts):
            raise ValueError("quality_field reads the coordinates resident in handles: pass one Smoother per cut")
        if k_count is None:
            k_count = self.nlayers - 1 - k_begin
        ni, nj = cuts[0]._mesh.blocks[b].points.size
        out = np.empty((max(0, k_count), max(0, nj - 1), max(0, ni - 1)), dtype=np.float64)
        handles = (C.c_void_p * len(cuts))(*[c._h for c in cuts])
        if self.surfaces is None:
            _capi.check(_capi.lib().tm_stack_smoothers_quality_field(handles, C.byref(self._opt), b, k_begin, k_count, _capi.f64ptr(out)))
        else:
            _capi.check(_capi.lib().tm_stack_smoothers_quality_field_surf(handles, C.byref(self._opt), self.surfaces.ref(), b, k_begin, k_count, _capi.f64ptr(out)))
        return out

    def check_elevation(self, cut, elevation):
        """TmError (InconsistentSize) naming the first offender of an elevation to curved hexahedra: a block of the cut (a discrete.Mesh:
        sizes and topology alone are read) or a connection range off the element grid, or the layer count (tm_ho3_check: host only)."""
        md = _capi.MeshDesc(cut, with_coordinates=False)
        _capi.check(_capi.lib().tm_ho3_check(md.ref(), C.byref(self._opt), C.byref(elevation._opt)))

    def elevate(self, cuts, elevation, b, g_begin=0, g_count=None, host=False, planes=True, return_outside=False):
        """(X, Y, Z, HoQuality3d, sj) of block b as curved hexahedra of the order of `elevation` (highorder.Elevation, order <= 4; "high-order
        hexahedra of stacked blocks" in the header), evaluated on the device straight from the cuts (kernel K16: the fine 3-D block is never
        stored).  X, Y, Z: the node layers [g_begin*p, (g_begin + g_count)*p] of the span elements [g_begin, g_begin + g_count) as
        (g_count*p + 1, nj, ni) arrays (None with planes=False: the report alone); the record and sj -- the scaled Jacobian per element as an
        (Eg, Ej, Ei) array, NaN for invalid elements -- always cover the whole block.  cuts as in block(): Mesh (tm_stack_elevate;
        host=True: tm_stack_elevate_host, no GPU) or Smoother (tm_stack_smoothers_elevate, the resident coordinates).
        return_outside=True (mapping="revolution") adds the per-cut count of extrapolated nodes."""
        from . import quality as _quality

        self._check_count(cuts)
        sf = self.surfaces
        if return_outside and sf is None:
            raise ValueError("return_outside: only with mapping='revolution'")
        resident = all(hasattr(c, "_h") for c in cuts)
        if resident and host:
            raise ValueError("host=True evaluates host coordinates: pass the meshes, not the handles")
        meshes = [c._mesh for c in cuts] if resident else cuts
        ni, nj = meshes[0].blocks[b].points.size
        p = max(1, elevation.order)
        Ei, Ej, Eg = max(0, (ni - 1) // p), max(0, (nj - 1) // p), max(0, (self.nlayers - 1) // p)
        if g_count is None:
            g_count = max(0, Eg - g_begin)
        out = [np.empty((g_count * p + 1, nj, ni), dtype=np.float64) if planes else None for _ in range(3)]
        sj = np.empty((Eg, Ej, Ei), dtype=np.float64)
        q = _capi.tm_ho3_quality()
        outside = np.zeros(max(1, self.ncuts), dtype=np.uint64)
        args = (C.byref(self._opt), None if sf is None else sf.ref(), C.byref(elevation._opt), b, g_begin, g_count if planes else 0,
                *[_capi.f64ptr(o) if planes else None for o in out], C.byref(q), _capi.f64ptr(sj),
                outside.ctypes.data_as(C.POINTER(C.c_uint64)) if return_outside else None)
        L = _capi.lib()
        if resident:
            handles = (C.c_void_p * len(cuts))(*[c._h for c in cuts])
            _capi.check(L.tm_stack_smoothers_elevate(handles, *args))
        else:
            descs = [_capi.MeshDesc(m) for m in meshes]
            arr = (C.POINTER(_capi.tm_mesh_desc) * len(descs))(*[C.pointer(d.desc) for d in descs])
            _capi.check((L.tm_stack_elevate_host if host else L.tm_stack_elevate)(arr, *args))
        res = (out[0], out[1], out[2], _quality.HoQuality3d.from_struct(q), sj)
        return res + ((outside[:self.ncuts].copy(),) if return_outside else ())

    def certify(self, cuts, elevation, b=None, host=False, max_depth=2):
        """The certificate of the curved hexahedra of block b ("high-order hexahedra: certificate" in the header, kernel K17) --
        (quality.HoCertificate3d, status, bounds): status an (Eg, Ej, Ei) uint8 array of TM_HO_PROVEN / TM_HO_INVALID / TM_HO_UNDECIDED,
        bounds an (Eg, Ej, Ei, 2) array of (lo, hi) with lo <= o*J <= hi on the whole element.  b=None: every block -- (total,
        [record per block], [status], [bounds]).  cuts as in block(): Mesh (tm_stack_certify; host=True: tm_stack_certify_host, no GPU)
        or Smoother (tm_stack_smoothers_certify, the resident coordinates)."""
        from . import quality as _quality

        self._check_count(cuts)
        resident = all(hasattr(c, "_h") for c in cuts)
        if resident and host:
            raise ValueError("host=True evaluates host coordinates: pass the meshes, not the handles")
        meshes = [c._mesh for c in cuts] if resident else cuts
        if b is None:
            self.check_elevation(meshes[0], elevation)
            out = [self.certify(cuts, elevation, k, host=host, max_depth=max_depth) for k in range(len(meshes[0].blocks))]
            per_block = [o[0] for o in out]
            return _quality.total_ho3_certificate(per_block), per_block, [o[1] for o in out], [o[2] for o in out]
        ni, nj = meshes[0].blocks[b].points.size
        p = max(1, elevation.order)
        E = (max(0, (self.nlayers - 1) // p), max(0, (nj - 1) // p), max(0, (ni - 1) // p))
        status = np.empty(E, dtype=np.uint8)
        bounds = np.empty(E + (2,), dtype=np.float64)
        c = _capi.tm_ho3_certificate()
        sf = self.surfaces
        args = (C.byref(self._opt), None if sf is None else sf.ref(), C.byref(elevation._opt), int(max_depth), b, C.byref(c),
                status.ctypes.data_as(C.POINTER(C.c_uint8)), _capi.f64ptr(bounds), None)
        L = _capi.lib()
        if resident:
            handles = (C.c_void_p * len(cuts))(*[h._h for h in cuts])
            _capi.check(L.tm_stack_smoothers_certify(handles, *args))
        else:
            descs = [_capi.MeshDesc(m) for m in meshes]
            arr = (C.POINTER(_capi.tm_mesh_desc) * len(descs))(*[C.pointer(d.desc) for d in descs])
            _capi.check((L.tm_stack_certify_host if host else L.tm_stack_certify)(arr, *args))
        return _quality.HoCertificate3d.from_struct(c), status, bounds

    def mesh3d_ho(self, cuts, elevation, host=False):
        """Every block of the cuts as curved hexahedra: a highorder.HighOrderMesh3d with the per-block and total quality.HoQuality3d (and,
        with mapping="revolution", per block the count of extrapolated nodes of every cut).  The size rule is checked first for all blocks
        (check_elevation)."""
        from . import highorder as _highorder
        from . import quality as _quality

        self._check_count(cuts)
        first = cuts[0]._mesh if hasattr(cuts[0], "_h") else cuts[0]
        self.check_elevation(first, elevation)
        m = _highorder.HighOrderMesh3d(elevation.order, elevation.distribution)
        for b, name in enumerate(first.names):
            X, Y, Z, q, sj, *outside = self.elevate(cuts, elevation, b, host=host, return_outside=self.surfaces is not None)
            m.outside += outside
            m.names.append(name)
            m.blocks.append((X, Y, Z))
            m.per_block.append(q)
            m.scaled_jacobian.append(sj)
        m.total = _quality.total_ho3(m.per_block)
        return m

    def mesh3d(self, cuts, host=False) -> Mesh3d:
        """Every block of the cuts, all layers."""
        self._check_count(cuts)
        first = cuts[0]._mesh if hasattr(cuts[0], "_h") else cuts[0]
        m = Mesh3d()
        for b, name in enumerate(first.names):
            m.names.append(name)
            m.blocks.append(self.block(cuts, b, host=host))
        return m
