"""High-order curved elements from smoothed blocks (include/tm_hip.h, "high-order elements"; the reference's roadmap item "high order
meshes -- equidistant / other distributions").

Every p x p group of cells of a block whose cell counts are multiples of p is one element of order p with (p+1)^2 nodes.  Its nodes are
the fine mesh itself (equidistant) or the element's degree-p tensor-product interpolant evaluated at another node distribution
(Gauss-Lobatto, or prescribed); the elements are judged by the Jacobian of that same polynomial at their nodes.

    el = Elevation(4)                          # Gauss-Lobatto nodes
    el.check(mesh)                             # TmError(InconsistentSize) naming the first block / connection off the element grid
    X, Y, q, sj = el.block(smoother, b)        # planes (nj, ni), quality.HoQuality, scaled Jacobian per element (Ej, Ei)
    Elevation(2, "equidistant").mesh(smoother).write("blade.vtk")

    cert, status, bounds = el.certify(smoother, b)   # quality.HoCertificate, (Ej, Ei) uint8 status, (Ej, Ei, 2) bounds of o*J

Stacked blocks (stack.Stack) become curved hexahedra of order p <= 4 the same way, in span as in i and j ("high-order hexahedra of stacked
blocks", kernel K16):

    X, Y, Z, q, sj = st.elevate(cuts, el, b)   # planes (nk, nj, ni), quality.HoQuality3d, scaled Jacobian per element (Eg, Ej, Ei)
    st.mesh3d_ho(cuts, Elevation(2, "equidistant")).write("blade.vtk")
    X, Y, Z, q, sj = planes3d(X0, Y0, Z0, el)  # any 3-D block, on the CPU

Evaluated on the MI355X (kernels K13, K14, K16); `host=True` evaluates the same definition on the CPU (a Mesh only), bit for bit."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Tuple

import numpy as np

from . import _capi
from . import quality as _quality

DISTRIBUTION = {"equidistant": _capi.TM_HO_EQUIDISTANT, "gauss_lobatto": _capi.TM_HO_GAUSS_LOBATTO, "prescribed": _capi.TM_HO_PRESCRIBED}
VTK_LAGRANGE_QUADRILATERAL = 70
VTK_LAGRANGE_HEXAHEDRON = 72


def lagrange_quad_order(p):
    """Local nodes (a, b) of an element of order p in the order of VTK's Lagrange quadrilateral (vtkLagrangeQuadrilateral::
    PointIndexFromIJK): the corners (0,0), (p,0), (p,p), (0,p); the edges b = 0 (a ascending), a = p (b ascending), b = p (a ascending),
    a = 0 (b ascending); the interior with a fastest."""
    order = [(0, 0), (p, 0), (p, p), (0, p)]
    order += [(a, 0) for a in range(1, p)]
    order += [(p, b) for b in range(1, p)]
    order += [(a, p) for a in range(1, p)]
    order += [(0, b) for b in range(1, p)]
    order += [(a, b) for b in range(1, p) for a in range(1, p)]
    return order


def lagrange_hex_order(p):
    """Local nodes (a, b, c) of an element of order p in the order of VTK 9's Lagrange hexahedron (vtkLagrangeHexahedron::
    PointIndexFromIJK): the corners of the face c = 0 counter-clockwise from (0,0,0), then those of c = p; the edges of c = 0 in the order
    of the quadrilateral (b = 0, a = p, b = p, a = 0, each ascending), those of c = p, then the four vertical edges at (0,0), (p,0), (p,p),
    (0,p) -- the numbering of VTK >= 9 --; the faces a = 0, a = p (b fastest), b = 0, b = p (a fastest), c = 0, c = p (a fastest); the
    interior with a fastest, then b."""
    r = range(1, p)
    ring = [(0, 0), (p, 0), (p, p), (0, p)]
    order = [(a, b, c) for c in (0, p) for a, b in ring]
    for c in (0, p):
        order += [(a, 0, c) for a in r] + [(p, b, c) for b in r] + [(a, p, c) for a in r] + [(0, b, c) for b in r]
    order += [(a, b, c) for a, b in ring for c in r]
    order += [(a, b, c) for a in (0, p) for c in r for b in r]
    order += [(a, b, c) for b in (0, p) for c in r for a in r]
    order += [(a, b, c) for c in (0, p) for b in r for a in r]
    order += [(a, b, c) for c in r for b in r for a in r]
    return order


def planes3d(X, Y, Z, elevation, block=0, planes=True):
    """(X, Y, Z, HoQuality3d, sj) of any 3-D block given as (nk, nj, ni) arrays (PLOT3D order: what Stack.block returned, or a file read
    with output.read_plot3d_3d), elevated on the CPU (tm_ho3_planes_host: no GPU needed).  The planes have the same shape (None with
    planes=False: the report alone); sj is the scaled Jacobian per element as an (Eg, Ej, Ei) array, NaN for invalid elements."""
    X, Y, Z = (np.ascontiguousarray(a, dtype=np.float64) for a in (X, Y, Z))
    if X.ndim != 3 or Y.shape != X.shape or Z.shape != X.shape:
        raise ValueError("X, Y, Z: three (nk, nj, ni) arrays of one shape")
    nk, nj, ni = X.shape
    p = max(1, elevation.order)
    out = [np.empty_like(X) if planes else None for _ in range(3)]
    sj = np.empty((max(0, (nk - 1) // p), max(0, (nj - 1) // p), max(0, (ni - 1) // p)), dtype=np.float64)
    q = _capi.tm_ho3_quality()
    _capi.check(_capi.lib().tm_ho3_planes_host(_capi.f64ptr(X), _capi.f64ptr(Y), _capi.f64ptr(Z), ni, nj, nk, C.byref(elevation._opt), block,
                                               *[_capi.f64ptr(o) if planes else None for o in out], C.byref(q), _capi.f64ptr(sj)))
    return out[0], out[1], out[2], _quality.HoQuality3d.from_struct(q), sj


def _planes_of(X, Y, Z):
    X, Y, Z = (np.ascontiguousarray(a, dtype=np.float64) for a in (X, Y, Z))
    if X.ndim != 3 or Y.shape != X.shape or Z.shape != X.shape:
        raise ValueError("X, Y, Z: three (nk, nj, ni) arrays of one shape")
    return X, Y, Z


def certify3d(X, Y, Z, elevation, max_depth=2, block=0):
    """(HoCertificate3d, status, bounds) of any 3-D block given as (nk, nj, ni) arrays (PLOT3D order), certified on the CPU
    (tm_ho3_certify_planes_host: no GPU needed): status an (Eg, Ej, Ei) uint8 array of TM_HO_PROVEN / TM_HO_INVALID / TM_HO_UNDECIDED,
    bounds an (Eg, Ej, Ei, 2) array of (lo, hi) with lo <= o*J <= hi on the whole element."""
    X, Y, Z = _planes_of(X, Y, Z)
    nk, nj, ni = X.shape
    p = max(1, elevation.order)
    E = (max(0, (nk - 1) // p), max(0, (nj - 1) // p), max(0, (ni - 1) // p))
    status = np.empty(E, dtype=np.uint8)
    bounds = np.empty(E + (2,), dtype=np.float64)
    c = _capi.tm_ho3_certificate()
    _capi.check(_capi.lib().tm_ho3_certify_planes_host(_capi.f64ptr(X), _capi.f64ptr(Y), _capi.f64ptr(Z), ni, nj, nk, C.byref(elevation._opt),
                                                       int(max_depth), block, C.byref(c), status.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                       _capi.f64ptr(bounds)))
    return _quality.HoCertificate3d.from_struct(c), status, bounds


def jacobian_bezier3d(X, Y, Z, elevation, e, f, g):
    """The (3p, 3p, 3p) Bernstein coefficients B[a, b, c] (a along i, b along j, c along span) of the Jacobian of element (e, f, g) of a
    3-D block given as (nk, nj, ni) arrays, not multiplied by the orientation (tm_ho3_jacobian_bezier_host: host only)."""
    X, Y, Z = _planes_of(X, Y, Z)
    nk, nj, ni = X.shape
    n = 3 * max(1, elevation.order)
    B = np.empty((n, n, n))
    _capi.check(_capi.lib().tm_ho3_jacobian_bezier_host(_capi.f64ptr(X), _capi.f64ptr(Y), _capi.f64ptr(Z), ni, nj, nk, C.byref(elevation._opt),
                                                        e, f, g, _capi.f64ptr(B)))
    return B


@dataclass
class HighOrderMesh3d:
    """The elevated blocks of a stacked mesh: per block the X, Y, Z coordinates as (nk, nj, ni) arrays (PLOT3D order, i fastest), the
    per-block and total quality.HoQuality3d and the scaled Jacobian per element as (Eg, Ej, Ei) arrays."""

    order: int
    distribution: str
    names: List[str] = field(default_factory=list)
    blocks: List[Tuple[np.ndarray, np.ndarray, np.ndarray]] = field(default_factory=list)
    per_block: List["_quality.HoQuality3d"] = field(default_factory=list)
    scaled_jacobian: List[np.ndarray] = field(default_factory=list)
    total: "_quality.HoQuality3d | None" = None
    outside: List[np.ndarray] = field(default_factory=list)   # mapping="revolution": per block the extrapolated nodes of every cut

    def sizes(self):
        return [(x.shape[2], x.shape[1], x.shape[0]) for x, _, _ in self.blocks]

    def write(self, filename):
        """`*.vtk`: a legacy ASCII VTK unstructured grid with one VTK_LAGRANGE_HEXAHEDRON (type 72) per element -- points per block in
        PLOT3D order, blocks concatenated (interface nodes are not merged: weld() does that), coordinates as %.17g; VTK's Lagrange cells assume equidistant
        nodes, so any other distribution raises ValueError.  Any other name: multi-block 3-D PLOT3D of the elevated nodes."""
        from . import output

        if str(filename).lower().endswith(".vtk"):
            if self.distribution != "equidistant":
                raise ValueError(f"VTK Lagrange cells assume equidistant nodes: a {self.distribution} elevation goes to PLOT3D")
            output.write_vtk_lagrange_hex(filename, self.order, self.blocks)
            return
        output._format_of(filename)
        output.write_plot3d_3d(filename, self.sizes(), self.blocks)

    def weld(self, mesh, host=False, boundary=False, orientation=None):
        """weld.UnstructuredMesh of these blocks: the interface nodes of `mesh` (the cut the blocks were stacked from: sizes and
        connections) merged, one Lagrange hexahedron of `order` per element (include/tm_hip.h, "welded unstructured mesh").
        boundary=True: with .boundary, the faces in patches (hub and shroud included); orientation: per block, None = that of the elements."""
        from . import weld

        if boundary and orientation is None:
            orientation = [q.orientation for q in self.per_block]
        return weld.Weld(mesh, host=host).mesh(self, self.order, self.distribution, boundary=boundary, orientation=orientation)


@dataclass
class HighOrderMesh:
    """The elevated blocks of a mesh: per block the X, Y planes as (nj, ni) arrays (i fastest, the order of the export planes), the
    per-block and total quality.HoQuality and the scaled Jacobian per element as (Ej, Ei) arrays."""

    order: int
    distribution: str
    names: List[str] = field(default_factory=list)
    blocks: List[Tuple[np.ndarray, np.ndarray]] = field(default_factory=list)
    per_block: List["_quality.HoQuality"] = field(default_factory=list)
    scaled_jacobian: List[np.ndarray] = field(default_factory=list)
    total: "_quality.HoQuality | None" = None

    def sizes(self):
        return [(x.shape[1], x.shape[0]) for x, _ in self.blocks]

    def elements(self):
        """Per block (Ei, Ej)."""
        return [((ni - 1) // self.order, (nj - 1) // self.order) for ni, nj in self.sizes()]

    def write(self, filename):
        """`*.vtk`: a legacy ASCII VTK unstructured grid with one VTK_LAGRANGE_QUADRILATERAL (type 70) per element -- points per block
        in plane order, blocks concatenated (interface nodes are not merged: weld() does that), coordinates as %.17g; VTK's Lagrange cells assume
        equidistant nodes, so any other distribution raises ValueError.  Any other name: multi-block 2-D PLOT3D of the elevated nodes
        (output.write_plot3d)."""
        from . import output

        if str(filename).lower().endswith(".vtk"):
            if self.distribution != "equidistant":
                raise ValueError(f"VTK Lagrange cells assume equidistant nodes: a {self.distribution} elevation goes to PLOT3D")
            output.write_vtk_lagrange(filename, self.order, self.blocks)
            return
        output._format_of(filename)
        output.write_plot3d(filename, self.sizes(), [(x.reshape(-1), y.reshape(-1)) for x, y in self.blocks])

    def weld(self, mesh, host=False, boundary=False, orientation=None):
        """weld.UnstructuredMesh of these blocks: the interface nodes of `mesh` (sizes and connections) merged, one Lagrange
        quadrilateral of `order` per element (include/tm_hip.h, "welded unstructured mesh").  boundary=True: with .boundary, the
        faces in patches; orientation: per block, None = that of the elements."""
        from . import weld

        if boundary and orientation is None:
            orientation = [q.orientation for q in self.per_block]
        return weld.Weld(mesh, host=host).mesh(self, self.order, self.distribution, boundary=boundary, orientation=orientation)


class Elevation:
    """tm_ho_opt + the calls that take it."""

    def __init__(self, order, distribution="gauss_lobatto", nodes=None):
        distribution = distribution.replace("-", "_")
        if distribution not in DISTRIBUTION:
            raise ValueError(f"distribution {distribution!r}: one of {sorted(DISTRIBUTION)}")
        if nodes is not None and distribution != "prescribed":
            raise ValueError("nodes go with distribution='prescribed'")
        if distribution == "prescribed" and nodes is None:
            raise ValueError("distribution='prescribed' needs nodes")
        self.order = int(order)
        self.distribution = distribution
        self.nodes = None if nodes is None else np.ascontiguousarray(nodes, dtype=np.float64).reshape(-1)
        if self.nodes is not None and self.nodes.size != self.order + 1:
            raise ValueError(f"{self.nodes.size} nodes for order {self.order}: order + 1 are needed")
        self._opt = _capi.tm_ho_opt(self.order, DISTRIBUTION[distribution], _capi.f64ptr(self.nodes) if self.nodes is not None else None)

    def tables(self):
        """(nodes[p+1], T[p+1, p+1], D[p+1, p+1]), row = target node (tm_ho_tables: host only)."""
        n1 = max(1, self.order + 1)
        t, T, D = np.empty(n1), np.empty((n1, n1)), np.empty((n1, n1))
        _capi.check(_capi.lib().tm_ho_tables(C.byref(self._opt), _capi.f64ptr(t), _capi.f64ptr(T), _capi.f64ptr(D)))
        return t, T, D

    def check(self, mesh):
        """TmError (InconsistentSize) naming the first block or connection range that does not lie on the element grid (tm_ho_check)."""
        md = _capi.MeshDesc(mesh, with_coordinates=False)
        _capi.check(_capi.lib().tm_ho_check(md.ref(), C.byref(self._opt)))

    def block(self, mesh_or_smoother, b, host=False, planes=True):
        """(X, Y, HoQuality, sj) of block b: the elevated nodes as (nj, ni) arrays (None, None with planes=False: the report alone), the
        block's record and the scaled Jacobian per element as an (Ej, Ei) array, NaN for invalid elements.  A discrete.Mesh is uploaded
        per call (tm_ho_elevate; host=True: tm_ho_elevate_host, no GPU); a smooth.Smoother gives the coordinates resident in its handle
        (tm_smoother_elevate)."""
        resident = hasattr(mesh_or_smoother, "_h")
        mesh = mesh_or_smoother._mesh if resident else mesh_or_smoother
        if resident and host:
            raise ValueError("host=True evaluates host coordinates: pass the mesh, not the handle")
        ni, nj = mesh.blocks[b].points.size
        p = max(1, self.order)
        X = np.empty((nj, ni), dtype=np.float64) if planes else None
        Y = np.empty((nj, ni), dtype=np.float64) if planes else None
        sj = np.empty((max(0, (nj - 1) // p), max(0, (ni - 1) // p)), dtype=np.float64)
        q = _capi.tm_ho_quality()
        args = (C.byref(self._opt), b, _capi.f64ptr(X) if planes else None, _capi.f64ptr(Y) if planes else None, C.byref(q), _capi.f64ptr(sj))
        L = _capi.lib()
        if resident:
            _capi.check(L.tm_smoother_elevate(mesh_or_smoother._h, *args))
        else:
            md = _capi.MeshDesc(mesh)
            _capi.check((L.tm_ho_elevate_host if host else L.tm_ho_elevate)(md.ref(), *args))
        return X, Y, _quality.HoQuality.from_struct(q), sj

    def certify_tables(self):
        """(M[p+1, p+1], wu[2p, p], wv[2p, p+1], G, norm): the Lagrange -> Bernstein matrix, the product weights, the guard factor G(p)
        and ||M||_inf (tm_ho_certify_tables: host only)."""
        p = max(1, self.order)
        M, wu, wv = np.empty((p + 1, p + 1)), np.empty((2 * p, p)), np.empty((2 * p, p + 1))
        G, norm = C.c_double(), C.c_double()
        _capi.check(_capi.lib().tm_ho_certify_tables(C.byref(self._opt), _capi.f64ptr(M), _capi.f64ptr(wu), _capi.f64ptr(wv), C.byref(G), C.byref(norm)))
        return M, wu, wv, G.value, norm.value

    def certify3d_tables(self):
        """(M[p+1, p+1], wA, wB, G3, norm) of the certificate of hexahedra: wA = (w^{p,p}[2p+1, p+1], w^{p-1,p}[2p, p], w^{p,p-1}[2p, p+1]),
        wB = (w^{p-1,2p}[3p, p], w^{p,2p-1}[3p, p+1]), the Bernstein product weights w^{a,b}[k, i] = C(a,i) C(b,k-i) / C(a+b,k); the
        guard factor G3(p) and ||M||_inf (tm_ho3_certify_tables: host only)."""
        p = max(1, self.order)
        M = np.empty((p + 1, p + 1))
        sa = [(2 * p + 1, p + 1), (2 * p, p), (2 * p, p + 1)]
        sb = [(3 * p, p), (3 * p, p + 1)]
        wA, wB = np.empty(sum(a * b for a, b in sa)), np.empty(sum(a * b for a, b in sb))
        G, norm = C.c_double(), C.c_double()
        _capi.check(_capi.lib().tm_ho3_certify_tables(C.byref(self._opt), _capi.f64ptr(M), _capi.f64ptr(wA), _capi.f64ptr(wB), C.byref(G), C.byref(norm)))

        def split(w, shapes):
            out, at = [], 0
            for a, b in shapes:
                out.append(w[at:at + a * b].reshape(a, b).copy())
                at += a * b
            return tuple(out)

        return M, split(wA, sa), split(wB, sb), G.value, norm.value

    def jacobian_bezier(self, mesh, b, e, f):
        """The (2p, 2p) Bernstein coefficients of the Jacobian of element (e, f) of block b (tm_ho_jacobian_bezier_host: host only)."""
        p = max(1, self.order)
        B = np.empty((2 * p, 2 * p))
        md = _capi.MeshDesc(mesh)
        _capi.check(_capi.lib().tm_ho_jacobian_bezier_host(md.ref(), C.byref(self._opt), b, e, f, _capi.f64ptr(B)))
        return B

    def certify(self, mesh_or_smoother, b=None, host=False, max_depth=3):
        """The certificate of block b -- (HoCertificate, status, bounds): status an (Ej, Ei) uint8 array of TM_HO_PROVEN / TM_HO_INVALID /
        TM_HO_UNDECIDED, bounds an (Ej, Ei, 2) array of (lo, hi) with lo <= o*J <= hi on the whole element.  b=None: every block --
        (total HoCertificate, [HoCertificate per block], [status], [bounds]).  A discrete.Mesh is uploaded per call (tm_ho_certify;
        host=True: tm_ho_certify_host, no GPU); a smooth.Smoother gives the coordinates resident in its handle (tm_smoother_certify)."""
        resident = hasattr(mesh_or_smoother, "_h")
        mesh = mesh_or_smoother._mesh if resident else mesh_or_smoother
        if resident and host:
            raise ValueError("host=True evaluates host coordinates: pass the mesh, not the handle")
        if b is None:
            self.check(mesh)
            out = [self.certify(mesh_or_smoother, k, host=host, max_depth=max_depth) for k in range(len(mesh.blocks))]
            per_block = [o[0] for o in out]
            return _quality.total_ho_certificate(per_block), per_block, [o[1] for o in out], [o[2] for o in out]
        ni, nj = mesh.blocks[b].points.size
        p = max(1, self.order)
        Ei, Ej = max(0, (ni - 1) // p), max(0, (nj - 1) // p)
        status = np.empty((Ej, Ei), dtype=np.uint8)
        bounds = np.empty((Ej, Ei, 2), dtype=np.float64)
        c = _capi.tm_ho_certificate()
        args = (C.byref(self._opt), int(max_depth), b, C.byref(c), status.ctypes.data_as(C.POINTER(C.c_uint8)), _capi.f64ptr(bounds))
        L = _capi.lib()
        if resident:
            _capi.check(L.tm_smoother_certify(mesh_or_smoother._h, *args))
        else:
            md = _capi.MeshDesc(mesh)
            _capi.check((L.tm_ho_certify_host if host else L.tm_ho_certify)(md.ref(), *args))
        return _quality.HoCertificate.from_struct(c), status, bounds

    def mesh(self, mesh_or_smoother, host=False) -> HighOrderMesh:
        """Every block, with the per-block and total quality."""
        first = mesh_or_smoother._mesh if hasattr(mesh_or_smoother, "_h") else mesh_or_smoother
        self.check(first)
        m = HighOrderMesh(self.order, self.distribution)
        for b, name in enumerate(first.names):
            X, Y, q, sj = self.block(mesh_or_smoother, b, host=host)
            m.names.append(name)
            m.blocks.append((X, Y))
            m.per_block.append(q)
            m.scaled_jacobian.append(sj)
        m.total = _quality.total_ho(m.per_block)
        return m
