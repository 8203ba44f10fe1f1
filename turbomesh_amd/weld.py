"""Blocks welded into one conforming unstructured mesh (include/tm_hip.h, "welded unstructured mesh"; kernel K18): one node numbering
across the connections of a mesh, and from it welded points and cells -- what an unstructured or high-order solver reads as ONE mesh.

The numbering is a function of sizes and connections alone, and the node grid of a block's high-order elements is the block's own
ni x nj index space, so one Weld serves every product of the library:

    w = Weld(mesh)                                 # .map (int32 per node, plane order), .nodes, .info
    w.points(smoother)                             # (nodes, 2): the coordinates resident in the handle, read in place on the device
    w.points(elevation.mesh(smoother))             # the elevated nodes of a highorder.HighOrderMesh
    w.points(stack.mesh3d(cuts))                   # (nk * nodes, 3), layer-major: stack.Mesh3d, highorder.HighOrderMesh3d or [(X, Y, Z)]
    w.cells(order=2)                               # (elements, 9) ids in the order of VTK's Lagrange quadrilateral
    w.cells(order=1, layers=nk)                    # hexahedra across nk layers
    smoother.weld().write("blade.vtk")             # UnstructuredMesh: legacy ASCII VTK, %.17g
    w.periodic_pairs()                             # [(pairs (n, 2), (tx, ty))] per periodic connection: periodic sides are not glued
    w.boundary(order=1, orientation=o)             # Boundary: faces over the same ids in patches (inlet, outlet, periodic sides, unassigned,
                                                   # hub and shroud with layers=nk); .measure(points) sums length / area, normal, moment per patch
    w.mesh(src, boundary=True).write_boundary("blade.vtk")   # blade.boundary.vtk + blade.boundary.json beside the volume file
    f = w.faces(layers=nk, orientation=o)          # Faces: what a finite-volume solver reads -- interior faces with owner < neighbour in
                                                   # upper-triangular order, then the boundary; f.metrics(points): volumes, closedness,
                                                   # non-orthogonality, skewness (FvReport); output.write_polymesh(dir, points, f)

A welded node has the coordinates of its owner (the class member with the smallest index), bit for bit; `info.max_gap` says by how much the
other members differ from it -- the rounding "the two sides agree to", or the size of the mesh when a connection is wrong.
Evaluated on the MI355X; `host=True` evaluates the same definition on the CPU, with the same results.
Not served: .vtu / CGNS / Gmsh / HOPR writers (they now need a writer only), gluing periodic sides, telling wall from hub inside the
`unassigned` patch, blocks spread over ranks, averaging the two sides of an interface."""
from __future__ import annotations

import ctypes as C
import json
from dataclasses import asdict, dataclass

import numpy as np

from . import _capi

VTK_QUAD, VTK_HEXAHEDRON = 9, 12
VTK_LAGRANGE_QUADRILATERAL, VTK_LAGRANGE_HEXAHEDRON = 70, 72
VTK_LINE, VTK_LAGRANGE_CURVE = 3, 68
PATCH_NAMES = {_capi.TM_BC_WALL: "wall", _capi.TM_BC_INLET: "inlet", _capi.TM_BC_OUTLET: "outlet", _capi.TM_PATCH_PERIODIC: "periodic",
               _capi.TM_PATCH_UNASSIGNED: "unassigned", _capi.TM_PATCH_HUB: "hub", _capi.TM_PATCH_SHROUD: "shroud"}
_I32P = C.POINTER(C.c_int32)


def _i32ptr(a):
    return a.ctypes.data_as(_I32P)


@dataclass
class WeldInfo:
    """tm_weld_info: node counts, classes by size, the largest class, periodic pairs and the gaps (0 until points() has run)."""

    nodes_in: int = 0
    nodes_out: int = 0
    classes_2: int = 0
    classes_3: int = 0
    classes_4: int = 0
    classes_5_up: int = 0
    max_class: int = 1
    periodic_pairs: int = 0
    gap_node: int = 0
    max_gap: float = 0.0
    periodic_gap: float = 0.0

    @classmethod
    def from_struct(cls, s):
        return cls(**s.as_dict())


def log_report(log, info, name="mesh"):
    """One line on `log` (the `weld` logger of the program): nodes in -> out, classes by size, periodic pairs, max_gap."""
    log.info("%s: %d -> %d nodes, classes of 2 / 3 / 4 / 5+: %d / %d / %d / %d (largest %d), %d periodic pairs (gap %.3e), max_gap %.3e at node %d", name,
             info.nodes_in, info.nodes_out, info.classes_2, info.classes_3, info.classes_4, info.classes_5_up, info.max_class, info.periodic_pairs,
             info.periodic_gap, info.max_gap, info.gap_node)


class UnstructuredMesh:
    """Welded points (n, 2) or (n, 3), cells (elements, nodes per element) and the VTK cell type: VTK_QUAD 9 / VTK_HEXAHEDRON 12 at order 1,
    VTK_LAGRANGE_QUADRILATERAL 70 / VTK_LAGRANGE_HEXAHEDRON 72 above."""

    def __init__(self, points, cells, cell_type, order, info=None, distribution="equidistant"):
        self.points = np.ascontiguousarray(points, dtype=np.float64)
        self.cells = np.ascontiguousarray(cells)
        self.cell_type = int(cell_type)
        self.order = int(order)
        self.info = info
        self.distribution = distribution
        if self.points.ndim != 2 or self.points.shape[1] not in (2, 3) or self.cells.ndim != 2:
            raise ValueError("points: (n, 2) or (n, 3); cells: (elements, nodes per element)")

    def write(self, filename):
        """`*.vtk`: legacy ASCII VTK unstructured grid, coordinates as %.17g (z = 0 for a plane mesh): output.read_vtk_lagrange reads it
        back bit for bit.  VTK's Lagrange cells assume equidistant nodes, so any other distribution raises ValueError."""
        if not str(filename).lower().endswith(".vtk"):
            raise ValueError(f"a welded mesh is written as legacy VTK (*.vtk), not {filename!r}")
        if self.order > 1 and self.distribution != "equidistant":
            raise ValueError(f"VTK Lagrange cells assume equidistant nodes, not a {self.distribution} elevation")
        kind = "quadrilaterals" if self.cell_type in (VTK_QUAD, VTK_LAGRANGE_QUADRILATERAL) else "hexahedra"
        with open(filename, "w") as fh:
            fh.write(f"# vtk DataFile Version 4.2\nwelded {kind} of order {self.order}\nASCII\nDATASET UNSTRUCTURED_GRID\n")
            fh.write(f"POINTS {len(self.points)} double\n")
            if self.points.shape[1] == 2:
                fh.write("".join("%.17g %.17g 0\n" % (x, y) for x, y in self.points.tolist()))
            else:
                fh.write("".join("%.17g %.17g %.17g\n" % (x, y, z) for x, y, z in self.points.tolist()))
            per = self.cells.shape[1]
            fh.write(f"CELLS {len(self.cells)} {len(self.cells) * (per + 1)}\n")
            head = str(per)
            fh.write("".join(head + " " + " ".join(map(str, row)) + "\n" for row in self.cells.tolist()))
            fh.write(f"CELL_TYPES {len(self.cells)}\n")
            fh.write(f"{self.cell_type}\n" * len(self.cells))
            wd = getattr(self, "wall_distance", None)
            if wd is not None:   # only when present: a file without the field is byte for byte what it was
                d = wd.distance if hasattr(wd, "distance") else np.asarray(wd, dtype=np.float64)
                if len(d) != len(self.points):
                    raise ValueError(f"{len(d)} wall distances for {len(self.points)} points")
                fh.write(f"POINT_DATA {len(d)}\nSCALARS wall_distance double 1\nLOOKUP_TABLE default\n")
                fh.write("".join("%.17g\n" % v for v in d.tolist()))

    def _write_points(self, fh):
        fh.write(f"POINTS {len(self.points)} double\n")
        if self.points.shape[1] == 2:
            fh.write("".join("%.17g %.17g 0\n" % (x, y) for x, y in self.points.tolist()))
        else:
            fh.write("".join("%.17g %.17g %.17g\n" % (x, y, z) for x, y, z in self.points.tolist()))

    def write_boundary(self, name):
        """The boundary of a mesh made with boundary=True, beside the volume file NAME.vtk: NAME.boundary.vtk -- the SAME points as the
        volume file, so ids are shared, the faces as cells (VTK_LINE 3 / VTK_LAGRANGE_CURVE 68 / VTK_QUAD 9 / VTK_LAGRANGE_QUADRILATERAL 70)
        and the CELL_DATA `patch` and `kind` -- and NAME.boundary.json, the patch table.  output.read_vtk_boundary reads the first back bit
        for bit.  Returns the two file names."""
        b = getattr(self, "boundary", None)
        if b is None:
            raise ValueError("the mesh carries no boundary: Weld.mesh(..., boundary=True)")
        if self.order > 1 and self.distribution != "equidistant":
            raise ValueError(f"VTK Lagrange cells assume equidistant nodes, not a {self.distribution} elevation")
        stem = str(name)[:-4] if str(name).lower().endswith(".vtk") else str(name)
        vtk, js = stem + ".boundary.vtk", stem + ".boundary.json"
        with open(vtk, "w") as fh:
            fh.write(f"# vtk DataFile Version 4.2\nboundary faces of order {self.order} in {len(b.patches)} patches\nASCII\nDATASET UNSTRUCTURED_GRID\n")
            self._write_points(fh)
            per = b.faces.shape[1]
            fh.write(f"CELLS {len(b.faces)} {len(b.faces) * (per + 1)}\n")
            head = str(per)
            fh.write("".join(head + " " + " ".join(map(str, row)) + "\n" for row in b.faces.tolist()))
            fh.write(f"CELL_TYPES {len(b.faces)}\n")
            fh.write(f"{b.cell_type}\n" * len(b.faces))
            fh.write(f"CELL_DATA {len(b.faces)}\nSCALARS patch int 1\nLOOKUP_TABLE default\n")
            fh.write("".join(f"{q}\n" for q in b.face_patch.tolist()))
            kinds = [b.patches[q].kind for q in b.face_patch.tolist()]
            fh.write("SCALARS kind int 1\nLOOKUP_TABLE default\n")
            fh.write("".join(f"{k}\n" for k in kinds))
        with open(js, "w") as fh:
            json.dump(b.table(), fh, indent=1)
        return vtk, js


@dataclass
class Patch:
    """tm_weld_patch: kind (TM_BC_* / TM_PATCH_*), name, source (index of the condition / the periodic connection, else -1), partner (the
    other patch of a periodic connection, else -1), translation (own face + translation = partner's face), begin / faces (the CSR over
    Boundary.faces), and the sums of Boundary.measure: measure (length / area), normal, moment."""

    kind: int
    name: str
    source: int
    partner: int
    translation: tuple
    begin: int
    faces: int
    measure: float = 0.0
    normal: tuple = (0.0, 0.0, 0.0)
    moment: float = 0.0


@dataclass
class BoundaryInfo:
    patches: int = 0
    faces: int = 0
    nodes_per_face: int = 0
    lateral_faces: int = 0
    cap_faces: int = 0
    loops: int = 0
    irregular_nodes: int = 0


def face_type_of(order, layered):
    if layered:
        return VTK_QUAD if order == 1 else VTK_LAGRANGE_QUADRILATERAL
    return VTK_LINE if order == 1 else VTK_LAGRANGE_CURVE


class Boundary:
    """The boundary faces of a Weld (include/tm_hip.h, "boundary of the welded mesh"; kernel K19): .faces (faces, nodes per face) int32
    welded ids, patch-major; .face_patch; .origin (faces, 4): block, side (4 / 5: hub / shroud), e, g; .patches (Patch records); .info
    (BoundaryInfo: counts, loops, irregular_nodes); .cell_type (VTK).  orientation: +-1 per block, from the quality report of the
    coordinates (quality.Quality.orientation, with layers quality.Quality3d.orientation) -- with it every normal points outward; None: +1."""

    def __init__(self, weld, order=1, layers=None, orientation=None):
        p = int(order)
        nk = int(layers) if layers else 0
        self.order, self.layers, self.host = p, nk, weld.host
        self._weld = weld
        L = _capi.lib()
        rec = _capi.tm_weld_boundary_info()
        _capi.check(L.tm_weld_boundary_plan(weld._md.ref(), p, nk, C.byref(rec), None))
        self.info = BoundaryInfo(**rec.as_dict())
        self._patches = (_capi.tm_weld_patch * max(1, self.info.patches))()
        _capi.check(L.tm_weld_boundary_plan(weld._md.ref(), p, nk, C.byref(rec), self._patches))
        o = None
        if orientation is not None:
            o = np.ascontiguousarray([int(v) for v in orientation], dtype=np.int32)
            if len(o) != len(weld.sizes):
                raise ValueError(f"{len(o)} orientations for {len(weld.sizes)} blocks")
        self.orientation = o
        self.faces = np.empty((self.info.faces, self.info.nodes_per_face), dtype=np.int32)
        self.face_patch = np.empty(self.info.faces, dtype=np.int32)
        self.origin = np.empty((self.info.faces, 4), dtype=np.int32)
        fn = L.tm_weld_boundary_faces_host if self.host else L.tm_weld_boundary_faces
        _capi.check(fn(weld._md.ref(), _i32ptr(weld.map), weld.nodes, p, nk, None if o is None else _i32ptr(o), _i32ptr(self.faces), _i32ptr(self.face_patch),
                       _i32ptr(self.origin)))
        self.cell_type = face_type_of(p, nk >= 2)
        self.patches = self._records()

    def _records(self):
        out, seen = [], {}
        for q in range(self.info.patches):
            r = self._patches[q]
            name = PATCH_NAMES.get(r.kind, f"kind{r.kind}")
            if r.kind == _capi.TM_PATCH_PERIODIC:
                name = f"periodic{r.source}" + ("a" if r.partner > q else "b")
            seen[name] = seen.get(name, 0) + 1
            if seen[name] > 1:
                name += str(seen[name])
            out.append(Patch(int(r.kind), name, int(r.source), int(r.partner), (float(r.translation[0]), float(r.translation[1])), int(r.face_begin),
                             int(r.faces), float(r.measure), tuple(float(v) for v in r.normal), float(r.moment)))
        return out

    def measure(self, points):
        """Per patch the sums over the fine sub-faces of its faces on the welded `points` ((nodes, 2), or (nk * nodes, 3) with layers; or a
        list of the component planes):
        measure (length / area), normal (outward with the right orientation), moment (sum / 2 = enclosed area; sum / 3 = volume for planar
        faces).  tm_weld_faces_measure (host=True: tm_weld_faces_measure_host).  Updates and returns .patches."""
        dim = 3 if self.layers >= 2 else 2
        if isinstance(points, (list, tuple)):   # the planes themselves, one array per component: nothing is copied
            planes = [np.ascontiguousarray(a, dtype=np.float64) for a in points[:dim]]
            if len(planes) < dim or any(a.ndim != 1 or len(a) != len(planes[0]) for a in planes):
                raise ValueError(f"points: {dim} planes of one length")
            pts = planes[0]
        else:
            pts = np.ascontiguousarray(points, dtype=np.float64)
            if pts.ndim != 2 or pts.shape[1] < dim:
                raise ValueError(f"points: (n, {dim}) welded coordinates")
            planes = [np.ascontiguousarray(pts[:, c]) for c in range(dim)]
        dp = C.POINTER(C.c_double)
        arr = (dp * dim)(*[_capi.f64ptr(a) for a in planes])
        L = _capi.lib()
        fn = L.tm_weld_faces_measure_host if self.host else L.tm_weld_faces_measure
        _capi.check(fn(dim, self.order, len(self.faces), _i32ptr(self.faces), _i32ptr(self.face_patch), self.info.patches, len(pts), dim, arr, self._patches))
        self.patches = self._records()
        return self.patches

    def periodic_faces(self):
        """Per periodic connection (faces of the side of ranges[0], faces of the side of ranges[1], translation): face t of one is the partner
        of face t of the other, node (a, c) of one the image of node (p - a, c) of the other."""
        out = []
        for q, r in enumerate(self.patches):
            if r.kind == _capi.TM_PATCH_PERIODIC and r.partner > q:
                o = self.patches[r.partner]
                out.append((self.faces[r.begin:r.begin + r.faces], self.faces[o.begin:o.begin + o.faces], r.translation))
        return out

    def wall_faces(self, kinds=None):
        """(faces, face_index, images) of the patches whose kind is named in `kinds` -- names of PATCH_NAMES; default ("wall", "unassigned"),
        with layers ("wall", "unassigned", "hub", "shroud") -- for Weld.wall_distance: the selected rows of .faces, patch-major, their
        indices into .faces, and the images of the periodic translations ((n, 5) rows t0, t1, t2, c, s: the identity, then +T and -T per
        distinct translation).  tm_wall_select; needs order 1."""
        if self.order != 1:
            raise ValueError("wall distance is defined on the fine mesh: a Boundary of order 1")
        if kinds is None:
            kinds = ("wall", "unassigned", "hub", "shroud") if self.layers >= 2 else ("wall", "unassigned")
        mask = kinds_mask(kinds)
        L = _capi.lib()
        nf, ni = C.c_uint64(0), C.c_uint64(0)
        md = self._weld._md.ref()
        _capi.check(L.tm_wall_select(md, self.layers, mask, C.byref(nf), None, C.byref(ni), None))
        index = np.empty(nf.value, dtype=np.int32)
        im = (_capi.tm_wall_image * max(1, ni.value))()
        _capi.check(L.tm_wall_select(md, self.layers, mask, C.byref(nf), _i32ptr(index), C.byref(ni), im))
        images = np.array([[m.t[0], m.t[1], m.t[2], m.c, m.s] for m in im[:ni.value]], dtype=np.float64).reshape(-1, 5)
        return np.ascontiguousarray(self.faces[index]), index, images

    def table(self):
        """The patch table as plain data (what NAME.boundary.json holds)."""
        return {"order": self.order, "layers": self.layers, "cell_type": self.cell_type, "info": asdict(self.info),
                "patches": [dict(asdict(r), translation=list(r.translation), normal=list(r.normal)) for r in self.patches]}


def resident_boundary(smoother, order=1, orientation=None):
    """smooth.Smoother.weld_boundary: (faces, face_patch, patches) from the coordinates resident in the handle."""
    L = _capi.lib()
    md = _capi.MeshDesc(smoother._mesh, with_coordinates=False)
    rec = _capi.tm_weld_boundary_info()
    _capi.check(L.tm_weld_boundary_plan(md.ref(), int(order), 0, C.byref(rec), None))
    faces = np.empty((rec.faces, rec.nodes_per_face), dtype=np.int32)
    face_patch = np.empty(rec.faces, dtype=np.int32)
    patches = (_capi.tm_weld_patch * max(1, rec.patches))()
    o = None if orientation is None else np.ascontiguousarray([int(v) for v in orientation], dtype=np.int32)
    if o is not None and len(o) != len(smoother._mesh.blocks):
        raise ValueError(f"{len(o)} orientations for {len(smoother._mesh.blocks)} blocks")
    _capi.check(L.tm_smoother_weld_boundary(smoother._h, int(order), None if o is None else _i32ptr(o), _i32ptr(faces), _i32ptr(face_patch), patches))
    b = Boundary.__new__(Boundary)
    b.info, b._patches = BoundaryInfo(**rec.as_dict()), patches
    return faces, face_patch, b._records()


def log_boundary(log, boundary, name="mesh"):
    """One line per patch on `log` (the `weld` logger of the program)."""
    i = boundary.info
    log.info("%s: boundary of %d faces in %d patches, %d loop(s), %d irregular nodes", name, i.faces, i.patches, i.loops, i.irregular_nodes)
    for q, r in enumerate(boundary.patches):
        log.info("%s: patch %d %-12s %7d faces, measure %.6e, normal (%+.3e, %+.3e, %+.3e), moment %+.6e%s", name, q, r.name, r.faces, r.measure, *r.normal,
                 r.moment, f", partner {r.partner}, translation ({r.translation[0]:g}, {r.translation[1]:g})" if r.partner >= 0 else "")


KIND_BITS = {name: kind for kind, name in PATCH_NAMES.items()}


def kinds_mask(kinds):
    """Bit k for kind k (tm_wall_select) from names of PATCH_NAMES, a comma-separated string or an integer mask."""
    if isinstance(kinds, int):
        return kinds
    if isinstance(kinds, str):
        kinds = [k.strip() for k in kinds.split(",") if k.strip()]
    mask = 0
    for k in kinds:
        if k not in KIND_BITS:
            raise ValueError(f"patch kind {k!r}: one of {sorted(KIND_BITS)}")
        mask |= 1 << KIND_BITS[k]
    return mask


def rotation_images(angle):
    """Images for cylindrical and revolution stacks, where the blades repeat by a rotation about the x axis and K19's planar translation
    does not apply: the identity, +angle, -angle as (3, 5) rows t0, t1, t2, c, s."""
    import math

    c, s = math.cos(angle), math.sin(angle)
    return np.array([[0.0, 0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, c, s], [0.0, 0.0, 0.0, c, -s]], dtype=np.float64)


@dataclass
class WallInfo:
    """tm_wall_info: sizes of the call, on_wall (distance exactly 0), nan_points, nearest_via_image, the maximum with its smallest node,
    pairs_evaluated (device: evaluations made; host: points x primitives x images)."""

    points: int = 0
    faces: int = 0
    primitives: int = 0
    images: int = 0
    groups: int = 0
    on_wall: int = 0
    nan_points: int = 0
    nearest_via_image: int = 0
    max_point: int = 0
    pairs_evaluated: int = 0
    max_distance: float = 0.0


@dataclass
class WallDistance:
    """distance (n,) float64, face (n,) int32 index into Boundary.faces of the nearest wall face, image (n,) int32 index of the image under
    which it is nearest (0: the wall itself), info (WallInfo).  A point with a NaN coordinate: NaN, -1, -1."""

    distance: np.ndarray
    face: np.ndarray
    image: np.ndarray
    info: WallInfo


def _images_struct(images):
    rows = np.ascontiguousarray(images, dtype=np.float64).reshape(-1, 5)
    arr = (_capi.tm_wall_image * max(1, len(rows)))()
    for m, r in zip(arr, rows.tolist()):
        m.t[0], m.t[1], m.t[2], m.c, m.s = r
    return arr, len(rows)


def wall_distance_of(faces, points, images=None, host=False, cull=True):
    """tm_wall_distance (host=True: tm_wall_distance_host) on any order-1 face list: faces (n, 2) edges over points (m, 2), or (n, 4)
    quadrilaterals over points (m, 3); images (k, 5) rows t0, t1, t2, c, s with row 0 the identity (None: the identity alone).
    cull=False: TM_WALL_NO_CULL, every pair is evaluated -- the results are the same.  -> WallDistance with face indexing `faces`."""
    faces = np.ascontiguousarray(faces, dtype=np.int32)
    pts = np.ascontiguousarray(points, dtype=np.float64)
    if faces.ndim != 2 or faces.shape[1] not in (2, 4):
        raise ValueError("faces: (n, 2) edges or (n, 4) quadrilaterals of order 1")
    dim = 2 if faces.shape[1] == 2 else 3
    if pts.ndim != 2 or pts.shape[1] < dim:
        raise ValueError(f"points: (n, {dim}) welded coordinates")
    planes = [np.ascontiguousarray(pts[:, c]) for c in range(dim)]
    arr = (C.POINTER(C.c_double) * dim)(*[_capi.f64ptr(a) for a in planes])
    im, nim = _images_struct(rotation_images(0.0)[:1] if images is None else images)
    n = len(pts)
    dist, face, image = np.empty(n), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
    rec = _capi.tm_wall_info()
    L = _capi.lib()
    fn = L.tm_wall_distance_host if host else L.tm_wall_distance
    _capi.check(fn(dim, len(faces), _i32ptr(faces), n, arr, nim, im, 0 if cull else _capi.TM_WALL_NO_CULL, _capi.f64ptr(dist), _i32ptr(face), _i32ptr(image),
                   C.byref(rec)))
    return WallDistance(dist, face, image, WallInfo(**rec.as_dict()))


def resident_wall_distance(smoother, kinds=None, cull=True, orientation=None):
    """smooth.Smoother.wall_distance: WallDistance of the coordinates resident in the handle (tm_smoother_wall_distance); face indexes the
    faces of Smoother.weld_boundary(1)."""
    L = _capi.lib()
    n = sum(int(b.points.size[0]) * int(b.points.size[1]) for b in smoother._mesh.blocks)   # nodes before welding: always enough
    o = None if orientation is None else np.ascontiguousarray([int(v) for v in orientation], dtype=np.int32)
    if o is not None and len(o) != len(smoother._mesh.blocks):
        raise ValueError(f"{len(o)} orientations for {len(smoother._mesh.blocks)} blocks")
    dist, face, image = np.empty(n), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
    info = _capi.tm_wall_info()
    _capi.check(L.tm_smoother_wall_distance(smoother._h, kinds_mask(("wall", "unassigned") if kinds is None else kinds), 0 if cull else _capi.TM_WALL_NO_CULL,
                                            None if o is None else _i32ptr(o), _capi.f64ptr(dist), _i32ptr(face), _i32ptr(image), C.byref(info)))
    n = int(info.points)
    return WallDistance(dist[:n].copy(), face[:n].copy(), image[:n].copy(), WallInfo(**info.as_dict()))


def log_wall_distance(log, wd, name="mesh"):
    """One line on `log` (the `weld` logger of the program): on-wall nodes, nodes nearest to an image, the maximum with its node."""
    i = wd.info
    log.info("%s: wall distance of %d nodes to %d faces under %d image(s): %d nodes on the wall, %d nodes nearest to an image, maximum %.6e at node %d", name,
             i.points, i.faces, i.images, i.on_wall, i.nearest_via_image, i.max_distance, i.max_point)


@dataclass
class FvReport:
    """tm_fv_info -- counts; min / max volume with their cells; negative_cells (V <= 0) and the first of them; total_volume; the largest
    closedness with its cell; the smallest cos with its face; nonorthogonal_faces (interior, cos < cos 70 degrees); inverted_faces
    (cos <= 0); the largest skewness with its face -- and with fields=True the arrays: volume, closedness (cells,), centre (cells, dim),
    area, face_centre (faces, dim), cos (faces,), skewness (internal faces,)."""

    cells: int = 0
    internal_faces: int = 0
    boundary_faces: int = 0
    min_volume_cell: int = 0
    max_volume_cell: int = 0
    negative_cells: int = 0
    first_negative_cell: int = 0
    max_closedness_cell: int = 0
    min_cos_face: int = 0
    nonorthogonal_faces: int = 0
    inverted_faces: int = 0
    max_skewness_face: int = 0
    min_volume: float = 0.0
    max_volume: float = 0.0
    total_volume: float = 0.0
    max_closedness: float = 0.0
    min_cos: float = 0.0
    max_skewness: float = 0.0
    volume: np.ndarray = None
    centre: np.ndarray = None
    closedness: np.ndarray = None
    area: np.ndarray = None
    face_centre: np.ndarray = None
    cos: np.ndarray = None
    skewness: np.ndarray = None


def fv_metrics_of(faces, owner, neighbour, cell_faces, points, fields=False, host=False):
    """tm_fv_metrics (host=True: tm_fv_metrics_host) on any face lists: faces (n, 2) edges over points (m, 2) with cell_faces (cells, 4),
    or (n, 4) quadrilaterals over points (m, 3) with cell_faces (cells, 6); owner (n,), neighbour (internal faces,) -> FvReport."""
    faces = np.ascontiguousarray(faces, dtype=np.int32)
    owner = np.ascontiguousarray(owner, dtype=np.int32)
    neighbour = np.ascontiguousarray(neighbour, dtype=np.int32)
    cell_faces = np.ascontiguousarray(cell_faces, dtype=np.int32)
    pts = np.ascontiguousarray(points, dtype=np.float64)
    if faces.ndim != 2 or faces.shape[1] not in (2, 4):
        raise ValueError("faces: (n, 2) edges or (n, 4) quadrilaterals of order 1")
    dim = 2 if faces.shape[1] == 2 else 3
    if pts.ndim != 2 or pts.shape[1] < dim:
        raise ValueError(f"points: (n, {dim}) welded coordinates")
    if cell_faces.ndim != 2 or cell_faces.shape[1] != 2 * dim or len(owner) != len(faces) or len(neighbour) > len(faces):
        raise ValueError(f"cell_faces: (cells, {2 * dim}); owner: one per face; neighbour: one per internal face")
    nc, nf, ni = len(cell_faces), len(faces), len(neighbour)
    planes = [np.ascontiguousarray(pts[:, c]) for c in range(dim)]
    arr = (C.POINTER(C.c_double) * dim)(*[_capi.f64ptr(a) for a in planes])
    out, fs = {}, None
    if fields:
        out = {"volume": np.empty(nc), "centre": np.empty((dim, nc)), "closedness": np.empty(nc), "area": np.empty((dim, nf)),
               "face_centre": np.empty((dim, nf)), "cos": np.empty(nf), "skewness": np.empty(ni)}
        fs = _capi.tm_fv_fields(**{k: _capi.f64ptr(v) for k, v in out.items()})
    rec = _capi.tm_fv_info()
    L = _capi.lib()
    fn = L.tm_fv_metrics_host if host else L.tm_fv_metrics
    _capi.check(fn(dim, nc, ni, nf - ni, _i32ptr(faces), _i32ptr(owner), _i32ptr(neighbour), _i32ptr(cell_faces), len(pts), arr,
                   None if fs is None else C.byref(fs), C.byref(rec)))
    for k in ("centre", "area", "face_centre"):
        if k in out:
            out[k] = np.ascontiguousarray(out[k].T)
    return FvReport(**rec.as_dict(), **out)


class Faces:
    """The face-based view of a Weld at order 1 (include/tm_hip.h, "faces of the welded mesh"; kernel K21): .faces (faces, 2 or 4) int32
    welded ids, interior faces first in upper-triangular order, then the faces of .boundary (a Boundary of order 1) in its order; .owner
    (faces,); .neighbour (ninternal,); .cell_faces (cells, 4 or 6): per cell of Weld.cells(1, layers) and local side the face index;
    .ninternal.  Every face is its owner's: its normal points owner -> neighbour, or out of the mesh.  orientation: see Boundary."""

    def __init__(self, weld, layers=None, orientation=None):
        nk = int(layers) if layers else 0
        self.layers, self.host = nk, weld.host
        self.boundary = Boundary(weld, 1, nk, orientation)
        L = _capi.lib()
        plan = _capi.tm_fv_plan()
        _capi.check(L.tm_weld_faces_plan(weld._md.ref(), nk, C.byref(plan)))
        self.ninternal, self.ncells = int(plan.internal_faces), int(plan.cells)
        n = self.ninternal + int(plan.boundary_faces)
        self.faces = np.empty((n, plan.nodes_per_face), dtype=np.int32)
        self.owner = np.empty(n, dtype=np.int32)
        self.neighbour = np.empty(self.ninternal, dtype=np.int32)
        self.cell_faces = np.empty((self.ncells, plan.faces_per_cell), dtype=np.int32)
        o = self.boundary.orientation
        fn = L.tm_weld_faces_host if self.host else L.tm_weld_faces
        _capi.check(fn(weld._md.ref(), _i32ptr(weld.map), weld.nodes, nk, None if o is None else _i32ptr(o), _i32ptr(self.faces), _i32ptr(self.owner),
                       _i32ptr(self.neighbour), _i32ptr(self.cell_faces)))

    def metrics(self, points, fields=False):
        """FvReport of the welded `points` ((nodes, 2), or (nk * nodes, 3) with layers)."""
        return fv_metrics_of(self.faces, self.owner, self.neighbour, self.cell_faces, points, fields=fields, host=self.host)


def resident_fv_report(smoother, orientation=None):
    """smooth.Smoother.fv_report: FvReport (the record alone) of the coordinates resident in the handle (tm_smoother_fv_report)."""
    o = None if orientation is None else np.ascontiguousarray([int(v) for v in orientation], dtype=np.int32)
    if o is not None and len(o) != len(smoother._mesh.blocks):
        raise ValueError(f"{len(o)} orientations for {len(smoother._mesh.blocks)} blocks")
    rec = _capi.tm_fv_info()
    _capi.check(_capi.lib().tm_smoother_fv_report(smoother._h, None if o is None else _i32ptr(o), C.byref(rec)))
    return FvReport(**rec.as_dict())


def log_fv_report(log, r, name="mesh"):
    """Three lines on `log` (the `weld` logger of the program): counts, volumes, face metrics."""
    log.info("%s: %d cells, %d internal and %d boundary faces", name, r.cells, r.internal_faces, r.boundary_faces)
    log.info("%s: volume %.6e .. %.6e (cells %d, %d), total %.9e, %d cells with V <= 0 (first %d), max closedness %.3e at cell %d", name, r.min_volume,
             r.max_volume, r.min_volume_cell, r.max_volume_cell, r.total_volume, r.negative_cells, r.first_negative_cell, r.max_closedness,
             r.max_closedness_cell)
    log.info("%s: min cos %.6f at face %d, %d internal faces beyond 70 degrees, %d faces with cos <= 0, max skewness %.6f at face %d", name, r.min_cos,
             r.min_cos_face, r.nonorthogonal_faces, r.inverted_faces, r.max_skewness, r.max_skewness_face)


def cell_type_of(order, hex):
    if order == 1:
        return VTK_HEXAHEDRON if hex else VTK_QUAD
    return VTK_LAGRANGE_HEXAHEDRON if hex else VTK_LAGRANGE_QUADRILATERAL


class Weld:
    """The welded numbering of a discrete.Mesh (tm_weld_map; host=True: tm_weld_map_host, no GPU)."""

    def __init__(self, mesh, host=False):
        self._mesh = mesh
        self.host = bool(host)
        self._md = _capi.MeshDesc(mesh, with_coordinates=False)
        self.sizes = [tuple(int(v) for v in b.points.size) for b in mesh.blocks]
        self.map = np.empty(sum(ni * nj for ni, nj in self.sizes), dtype=np.int32)
        rec = _capi.tm_weld_info()
        L = _capi.lib()
        _capi.check((L.tm_weld_map_host if self.host else L.tm_weld_map)(self._md.ref(), _i32ptr(self.map), C.byref(rec)))
        self._rec = rec
        self.info = WeldInfo.from_struct(rec)
        self.nodes = self.info.nodes_out

    def periodic_pairs(self):
        """Per periodic connection (pairs, translation): pairs an (n, 2) int32 array of welded ids (side of ranges[0], side of ranges[1]),
        translation the connection's (tx, ty), which maps the first onto the second (tm_weld_periodic_pairs: host only)."""
        flat = np.empty((max(1, self.info.periodic_pairs), 2), dtype=np.int32)
        _capi.check(_capi.lib().tm_weld_periodic_pairs(self._md.ref(), _i32ptr(self.map), _i32ptr(flat)))
        out, at = [], 0
        for c in self._mesh.connections:
            if c.periodicity is None:
                continue
            n = abs(int(c.ranges[0].end) - int(c.ranges[0].start)) + 1
            out.append((flat[at:at + n].copy(), (float(c.periodicity[0]), float(c.periodicity[1]))))
            at += n
        return out

    def _planes_of(self, src):
        """-> (ncomp, nk, [per component a list of per-block arrays of nk * nj * ni doubles, i fastest])"""
        blocks = getattr(src, "blocks", src)
        if len(blocks) != len(self.sizes):
            raise ValueError(f"{len(blocks)} blocks for a weld of {len(self.sizes)}")
        if hasattr(blocks[0], "points"):   # discrete.Mesh: (ni, nj, 2) interleaved
            comps = [[np.ascontiguousarray(b.points.data[:, :, c].T) for b in blocks] for c in range(2)]
            nk = 1
        else:
            ncomp = len(blocks[0])
            comps = [[np.ascontiguousarray(b[c], dtype=np.float64) for b in blocks] for c in range(ncomp)]
            nk = comps[0][0].shape[0] if comps[0][0].ndim == 3 else 1
        for plane in comps:
            for a, (ni, nj) in zip(plane, self.sizes):
                if a.shape != ((nk, nj, ni) if a.ndim == 3 else (nj, ni)):
                    raise ValueError(f"a block of shape {a.shape} where {(nj, ni)} nodes{' per layer' if a.ndim == 3 else ''} are welded")
        return len(comps), nk, comps

    def points(self, src):
        """Welded points of `src`: a discrete.Mesh, a smooth.Smoother (the coordinates resident in the handle, tm_smoother_weld), a
        highorder.HighOrderMesh -> (nodes, 2); a stack.Mesh3d, a highorder.HighOrderMesh3d or a list of (X, Y, Z) blocks as (nk, nj, ni)
        arrays -> (nk * nodes, 3), layer-major.  Updates info.max_gap, info.gap_node and info.periodic_gap."""
        L = _capi.lib()
        if hasattr(src, "_h"):
            if self.host:
                raise ValueError("host=True evaluates host coordinates: pass the mesh, not the handle")
            if [tuple(int(v) for v in b.points.size) for b in src._mesh.blocks] != self.sizes:
                raise ValueError("the handle holds another mesh")
            X, Y = np.empty(self.nodes), np.empty(self.nodes)
            rec = _capi.tm_weld_info()
            _capi.check(L.tm_smoother_weld(src._h, None, _capi.f64ptr(X), _capi.f64ptr(Y), C.byref(rec)))
            if rec.nodes_out != self.nodes:
                raise ValueError("the handle holds another mesh")
            self.info = WeldInfo.from_struct(rec)
            return np.stack([X, Y], axis=1)
        ncomp, nk, comps = self._planes_of(src)
        nb = len(self.sizes)
        dp = C.POINTER(C.c_double)
        planes = (dp * (ncomp * nb))(*[_capi.f64ptr(a) for plane in comps for a in plane])
        outs = [np.empty(nk * self.nodes) for _ in range(ncomp)]
        out = (dp * ncomp)(*[_capi.f64ptr(o) for o in outs])
        rec = self._rec
        _capi.check((L.tm_weld_points_host if self.host else L.tm_weld_points)(self._md.ref(), _i32ptr(self.map), ncomp, nk, planes, out, C.byref(rec)))
        self.info = WeldInfo.from_struct(rec)
        return np.stack(outs, axis=1)

    def cells(self, order=1, layers=None):
        """(elements, (order+1)^2) int32 ids of the quadrilaterals of `order` (1 .. 8) in the order of highorder.lagrange_quad_order,
        elements with e fastest and blocks in order; layers=nk >= 2: (elements, (order+1)^3) hexahedra (order 1 .. 4) across nk layers in
        the order of highorder.lagrange_hex_order, ids k * nodes + map (tm_weld_cells; host=True: tm_weld_cells_host)."""
        p = int(order)
        nk = int(layers) if layers else 0
        hex = nk >= 2
        if not 1 <= p <= (_capi.TM_HO3_MAX_ORDER if hex else _capi.TM_HO_MAX_ORDER):
            raise ValueError(f"order {p}: 1 .. {_capi.TM_HO3_MAX_ORDER if hex else _capi.TM_HO_MAX_ORDER}")
        n = sum(((ni - 1) // p) * ((nj - 1) // p) for ni, nj in self.sizes) * (max(0, nk - 1) // p if hex else 1)
        cells = np.empty((n, (p + 1) ** (3 if hex else 2)), dtype=np.int32)
        L = _capi.lib()
        _capi.check((L.tm_weld_cells_host if self.host else L.tm_weld_cells)(self._md.ref(), _i32ptr(self.map), self.nodes, p, nk, _i32ptr(cells)))
        return cells

    def boundary(self, order=1, layers=None, orientation=None):
        """The Boundary of this weld at `order` (with layers=nk >= 2 of the stacked mesh): faces in patches over the welded ids
        (tm_weld_boundary_faces; host=True: tm_weld_boundary_faces_host)."""
        return Boundary(self, order, layers, orientation)

    def faces(self, layers=None, orientation=None):
        """The Faces of this weld (with layers=nk >= 2 of the stacked mesh): interior faces with owner and neighbour in upper-triangular
        order, then the boundary of order 1; .metrics(points) gives the finite-volume report (tm_weld_faces; host=True:
        tm_weld_faces_host)."""
        return Faces(self, layers, orientation)

    def wall_distance(self, points, boundary=None, kinds=None, images=None, periodic=True, host=None, cull=True):
        """WallDistance of the welded `points` ((nodes, 2), or (nk * nodes, 3) with layers) to the faces of `boundary` (None: the Boundary
        of order 1 with the layers of the points) whose kind is in `kinds` (see Boundary.wall_faces).  images: (k, 5) rows, e.g.
        rotation_images(2 pi / blades); None: the periodic translations of the plan, or with periodic=False the wall itself alone.
        host (None: as this Weld): the host twin, plain loops over all pairs.  face refers to boundary.faces."""
        pts = np.ascontiguousarray(points, dtype=np.float64)
        host = self.host if host is None else bool(host)
        if boundary is None:
            nk = len(pts) // max(1, self.nodes) if pts.ndim == 2 and pts.shape[1] == 3 else 0
            boundary = self.boundary(1, nk)
        faces, index, plan_images = boundary.wall_faces(kinds)
        if len(faces) == 0:
            raise ValueError("no face of the boundary has one of the kinds asked for")
        if images is None:
            images = plan_images if periodic else plan_images[:1]
        wd = wall_distance_of(faces, pts, images, host=host, cull=cull)
        wd.face = np.where(wd.face >= 0, index[np.maximum(wd.face, 0)], -1).astype(np.int32)
        return wd

    def mesh(self, src, order=1, distribution="equidistant", boundary=False, orientation=None, wall_distance=False, kinds=None, images=None):
        """UnstructuredMesh of `src` (see points) with cells of `order`; the layers follow from the source.  boundary=True: the mesh
        carries .boundary, the Boundary at that order measured on the welded points (orientation: see Boundary).  wall_distance=True: it
        carries .wall_distance (WallDistance, see Weld.wall_distance for kinds and images) and write() emits the field; defined on the
        fine mesh, so at order 1."""
        pts = self.points(src)
        nk = len(pts) // max(1, self.nodes) if pts.shape[1] == 3 else 0
        um = UnstructuredMesh(pts, self.cells(order, nk), cell_type_of(order, nk >= 2), order, info=self.info, distribution=distribution)
        if boundary:
            um.boundary = self.boundary(order, nk, orientation)
            um.boundary.measure(pts)
        if wall_distance:
            if order != 1:
                raise ValueError("wall distance is defined on the fine mesh: compute it at order 1 and attach it to the element nodes")
            um.wall_distance = self.wall_distance(pts, self.boundary(1, nk, orientation), kinds=kinds, images=images)
        return um
