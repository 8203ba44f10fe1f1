"""Structured output of a mesh -- the step right after the hot path.

Mirrors the reference's writer boundary: `Mesh.write(filename)` (discrete.zig:197-216) and the smoother's
`system.write` with the control function (smooth.zig:396-414) hand the writer ONE PLANE PER COORDINATE with i fastest
(cgns.zig:75-104: plane[j*ni + i] = block(i,j)), optionally planes "P" and "Q" (cgns.zig:106-154).  That
de-interleaving transpose runs on the device (`tm_export_soa` / `tm_smoother_export_soa`, kernel K8).

File formats.  The reference writes CGNS through the system cgns library, which this image does not have: like a
reference build without -Duse-cgns, `.cgns` raises OutputFormatNotEnabled (discrete.zig:215).  What is written instead is
multi-block 2-D PLOT3D, whose grid file is exactly those planes: little-endian, no record markers,
    int32 nblocks | nblocks x (int32 ni, int32 nj) | per block: x[ni*nj] then y[ni*nj] (float64, i fastest)
and, for P,Q, a PLOT3D function file: int32 nblocks | nblocks x (int32 ni, nj, nvar=2) | per block: P plane, Q plane."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _capi


class OutputFormatNotEnabled(RuntimeError):
    """discrete.zig:215 error.OutputFormatNotEnabled"""


def block_planes(points) -> tuple[np.ndarray, np.ndarray]:
    """(x, y) planes of one block's (ni, nj, 2) array, element j*ni + i, transposed on the device (cgns.zig:75-104)."""
    xy = np.ascontiguousarray(points, dtype=np.float64)
    ni, nj = xy.shape[0], xy.shape[1]
    x = np.empty(ni * nj, dtype=np.float64)
    y = np.empty(ni * nj, dtype=np.float64)
    dp = C.POINTER(C.c_double)
    _capi.check(_capi.lib().tm_export_soa(xy.ctypes.data_as(dp), ni, nj, x.ctypes.data_as(dp), y.ctypes.data_as(dp)))
    return x, y


def write_plot3d(filename, sizes, planes):
    """sizes: [(ni, nj)], planes: [(x, y)] with i fastest.  Pure file writing (no device)."""
    with open(filename, "wb") as f:
        np.array([len(sizes)], dtype="<i4").tofile(f)
        np.array(sizes, dtype="<i4").reshape(-1, 2).tofile(f)
        for (ni, nj), (x, y) in zip(sizes, planes):
            assert x.size == ni * nj and y.size == ni * nj
            np.asarray(x, dtype="<f8").tofile(f)
            np.asarray(y, dtype="<f8").tofile(f)


def write_plot3d_function(filename, sizes, fields):
    """fields: per block a list of planes (here [P, Q])."""
    with open(filename, "wb") as f:
        np.array([len(sizes)], dtype="<i4").tofile(f)
        for (ni, nj), fl in zip(sizes, fields):
            np.array([ni, nj, len(fl)], dtype="<i4").tofile(f)
        for (ni, nj), fl in zip(sizes, fields):
            for p in fl:
                assert p.size == ni * nj
                np.asarray(p, dtype="<f8").tofile(f)


def read_plot3d(filename):
    """-> [(ni, nj, x(ni,nj), y(ni,nj))] with x[i, j] indexing restored."""
    with open(filename, "rb") as f:
        nb = int(np.fromfile(f, dtype="<i4", count=1)[0])
        sizes = np.fromfile(f, dtype="<i4", count=2 * nb).reshape(nb, 2)
        out = []
        for ni, nj in sizes:
            x = np.fromfile(f, dtype="<f8", count=ni * nj).reshape(nj, ni).T
            y = np.fromfile(f, dtype="<f8", count=ni * nj).reshape(nj, ni).T
            out.append((int(ni), int(nj), x, y))
    return out


def write_plot3d_3d(filename, sizes, planes):
    """Multi-block 3-D PLOT3D grid file, little-endian, no record markers:
        int32 nblocks | nblocks x (int32 ni, nj, nk) | per block: X[ni*nj*nk], Y, Z (float64, i fastest, then j, then k).
    sizes: [(ni, nj, nk)]; planes: per block (X, Y, Z), each any array of ni*nj*nk elements in that order -- what
    `stack.Stack.block` returns as (nk, nj, ni) arrays.  Pure file writing (no device)."""
    with open(filename, "wb") as f:
        np.array([len(sizes)], dtype="<i4").tofile(f)
        np.array(sizes, dtype="<i4").reshape(-1, 3).tofile(f)
        for (ni, nj, nk), xyz in zip(sizes, planes):
            assert len(xyz) == 3
            for p in xyz:
                p = np.asarray(p)
                assert p.size == ni * nj * nk
                np.ascontiguousarray(p, dtype="<f8").tofile(f)


def read_plot3d_3d(filename):
    """-> [(ni, nj, nk, X, Y, Z)], the coordinates as (nk, nj, ni) arrays (the order of the file)."""
    with open(filename, "rb") as f:
        nb = int(np.fromfile(f, dtype="<i4", count=1)[0])
        sizes = np.fromfile(f, dtype="<i4", count=3 * nb).reshape(nb, 3)
        out = []
        for ni, nj, nk in sizes:
            n = int(ni) * int(nj) * int(nk)
            xyz = [np.fromfile(f, dtype="<f8", count=n).reshape(nk, nj, ni) for _ in range(3)]
            out.append((int(ni), int(nj), int(nk), *xyz))
    return out


def write_vtk_lagrange(filename, order, blocks):
    """Legacy ASCII VTK unstructured grid of curved quadrilaterals: one VTK_LAGRANGE_QUADRILATERAL (type 70) of `order` per element.
    blocks: per block the (X, Y) planes as (nj, ni) arrays whose ni-1 and nj-1 are multiples of `order` (highorder.HighOrderMesh.blocks).
    Points: per block in plane order (i fastest), blocks concatenated, %.17g (reads back bit for bit), z = 0.  Local node (a, b) of
    element (e, f) is point (f*order + b)*ni + e*order + a of its block, listed in the order of highorder.lagrange_quad_order.
    Pure file writing (no device)."""
    from .highorder import VTK_LAGRANGE_QUADRILATERAL, lagrange_quad_order

    p = int(order)
    local = lagrange_quad_order(p)
    la = np.array([a for a, _ in local], dtype=np.int64)
    lb = np.array([b for _, b in local], dtype=np.int64)
    cells, offset, npoints = [], 0, 0
    for X, _ in blocks:
        nj, ni = X.shape
        if (ni - 1) % p or (nj - 1) % p:
            raise ValueError(f"a block of {ni} x {nj} nodes has no elements of order {p}")
        Ei, Ej = (ni - 1) // p, (nj - 1) // p
        f, e = np.meshgrid(np.arange(Ej, dtype=np.int64), np.arange(Ei, dtype=np.int64), indexing="ij")   # elements with e fastest
        ids = offset + (f.reshape(-1, 1) * p + lb) * ni + e.reshape(-1, 1) * p + la
        cells.append(ids)
        offset += ni * nj
    npoints = offset
    cells = np.concatenate(cells) if cells else np.empty((0, len(local)), dtype=np.int64)
    with open(filename, "w") as fh:
        fh.write(f"# vtk DataFile Version 4.2\ncurved quadrilaterals of order {p}\nASCII\nDATASET UNSTRUCTURED_GRID\n")
        fh.write(f"POINTS {npoints} double\n")
        for X, Y in blocks:
            fh.write("".join("%.17g %.17g 0\n" % (x, y) for x, y in zip(X.reshape(-1).tolist(), Y.reshape(-1).tolist())))
        fh.write(f"CELLS {len(cells)} {len(cells) * (len(local) + 1)}\n")
        head = str(len(local))
        fh.write("".join(head + " " + " ".join(map(str, row)) + "\n" for row in cells.tolist()))
        fh.write(f"CELL_TYPES {len(cells)}\n")
        fh.write(f"{VTK_LAGRANGE_QUADRILATERAL}\n" * len(cells))


def write_vtk_lagrange_hex(filename, order, blocks):
    """Legacy ASCII VTK unstructured grid of curved hexahedra: one VTK_LAGRANGE_HEXAHEDRON (type 72) of `order` per element.
    blocks: per block the (X, Y, Z) coordinates as (nk, nj, ni) arrays whose ni-1, nj-1 and nk-1 are multiples of `order`
    (highorder.HighOrderMesh3d.blocks).  Points: per block in PLOT3D order (i fastest), blocks concatenated, %.17g (reads back bit for
    bit).  Local node (a, b, c) of element (e, f, g) is point ((g*order + c)*nj + f*order + b)*ni + e*order + a of its block, listed in
    the order of highorder.lagrange_hex_order.  Pure file writing (no device)."""
    from .highorder import VTK_LAGRANGE_HEXAHEDRON, lagrange_hex_order

    p = int(order)
    local = np.array(lagrange_hex_order(p), dtype=np.int64)
    la, lb, lc = local[:, 0], local[:, 1], local[:, 2]
    cells, offset = [], 0
    for X, _, _ in blocks:
        nk, nj, ni = X.shape
        if (ni - 1) % p or (nj - 1) % p or (nk - 1) % p or nk < 2:
            raise ValueError(f"a block of {ni} x {nj} x {nk} nodes has no elements of order {p}")
        Ei, Ej, Eg = (ni - 1) // p, (nj - 1) // p, (nk - 1) // p
        g, f, e = np.meshgrid(np.arange(Eg, dtype=np.int64), np.arange(Ej, dtype=np.int64), np.arange(Ei, dtype=np.int64), indexing="ij")   # e fastest
        g, f, e = g.reshape(-1, 1), f.reshape(-1, 1), e.reshape(-1, 1)
        cells.append(offset + ((g * p + lc) * nj + f * p + lb) * ni + e * p + la)
        offset += ni * nj * nk
    cells = np.concatenate(cells) if cells else np.empty((0, len(local)), dtype=np.int64)
    with open(filename, "w") as fh:
        fh.write(f"# vtk DataFile Version 4.2\ncurved hexahedra of order {p}\nASCII\nDATASET UNSTRUCTURED_GRID\n")
        fh.write(f"POINTS {offset} double\n")
        for X, Y, Z in blocks:
            fh.write("".join("%.17g %.17g %.17g\n" % xyz for xyz in zip(X.reshape(-1).tolist(), Y.reshape(-1).tolist(), Z.reshape(-1).tolist())))
        fh.write(f"CELLS {len(cells)} {len(cells) * (len(local) + 1)}\n")
        head = str(len(local))
        fh.write("".join(head + " " + " ".join(map(str, row)) + "\n" for row in cells.tolist()))
        fh.write(f"CELL_TYPES {len(cells)}\n")
        fh.write(f"{VTK_LAGRANGE_HEXAHEDRON}\n" * len(cells))


def read_vtk_lagrange(filename):
    """-> (points (n, 3) float64, cells (ncells, nodes per cell) int64, cell_types (ncells,) int64) of a file written by
    write_vtk_lagrange or write_vtk_lagrange_hex (legacy ASCII, every cell with the same number of nodes: (p+1)^2 of type 70, or
    (p+1)^3 of type 72 with all three coordinates of the points in use)."""
    with open(filename) as fh:
        tok = fh.read().split("\n", 4)
    if len(tok) < 5 or not tok[0].startswith("# vtk DataFile") or tok[2].strip() != "ASCII" or tok[3].split() != ["DATASET", "UNSTRUCTURED_GRID"]:
        raise ValueError(f"{filename}: not a legacy ASCII VTK unstructured grid")
    w = tok[4].split()
    k = 0
    if w[k] != "POINTS" or w[k + 2] != "double":
        raise ValueError(f"{filename}: POINTS <n> double expected")
    n = int(w[k + 1])
    k += 3
    points = np.array([float(v) for v in w[k:k + 3 * n]], dtype=np.float64).reshape(n, 3)
    k += 3 * n
    if w[k] != "CELLS":
        raise ValueError(f"{filename}: CELLS expected")
    nc, size = int(w[k + 1]), int(w[k + 2])
    k += 3
    flat = np.array([int(v) for v in w[k:k + size]], dtype=np.int64)
    k += size
    per = size // nc - 1 if nc else 0
    rows = flat.reshape(nc, per + 1) if nc else flat.reshape(0, 1)
    if nc and not np.all(rows[:, 0] == per):
        raise ValueError(f"{filename}: cells of different sizes")
    if w[k] != "CELL_TYPES" or int(w[k + 1]) != nc:
        raise ValueError(f"{filename}: CELL_TYPES expected")
    types = np.array([int(v) for v in w[k + 2:k + 2 + nc]], dtype=np.int64)
    return points, rows[:, 1:].copy(), types


def read_vtk_point_data(filename):
    """-> {name: (n,) float64} of the POINT_DATA scalars of a legacy ASCII VTK file written by weld.UnstructuredMesh.write (the
    `wall_distance` of a mesh made with wall_distance=True, %.17g: read back bit for bit); {} when the file has no POINT_DATA."""
    with open(filename) as fh:
        text = fh.read()
    if not text.startswith("# vtk DataFile"):
        raise ValueError(f"{filename}: not a legacy VTK file")
    at = text.find("\nPOINT_DATA ")
    if at < 0:
        return {}
    w = text[at:].split()
    n, k, data = int(w[1]), 2, {}
    while k < len(w) and w[k] == "SCALARS":
        if w[k + 2] != "double" or w[k + 3] != "1" or w[k + 4:k + 6] != ["LOOKUP_TABLE", "default"]:
            raise ValueError(f"{filename}: SCALARS <name> double 1 expected")
        data[w[k + 1]] = np.array([float(v) for v in w[k + 6:k + 6 + n]], dtype=np.float64)
        k += 6 + n
    return data


def read_vtk_boundary(filename):
    """-> (points (n, 3) float64, faces (nfaces, nodes per face) int64, cell_types (nfaces,) int64, patch (nfaces,) int64, kind (nfaces,)
    int64) of a NAME.boundary.vtk written by weld.UnstructuredMesh.write_boundary (legacy ASCII: lines 3, Lagrange curves 68, quadrilaterals
    9 or Lagrange quadrilaterals 70 over the points of the volume file, CELL_DATA `patch` and `kind`)."""
    with open(filename) as fh:
        tok = fh.read().split("\n", 4)
    if len(tok) < 5 or not tok[0].startswith("# vtk DataFile") or tok[2].strip() != "ASCII" or tok[3].split() != ["DATASET", "UNSTRUCTURED_GRID"]:
        raise ValueError(f"{filename}: not a legacy ASCII VTK unstructured grid")
    w = tok[4].split()
    if w[0] != "POINTS" or w[2] != "double":
        raise ValueError(f"{filename}: POINTS <n> double expected")
    n = int(w[1])
    k = 3
    points = np.array([float(v) for v in w[k:k + 3 * n]], dtype=np.float64).reshape(n, 3)
    k += 3 * n
    if w[k] != "CELLS":
        raise ValueError(f"{filename}: CELLS expected")
    nc, size = int(w[k + 1]), int(w[k + 2])
    k += 3
    flat = np.array([int(v) for v in w[k:k + size]], dtype=np.int64)
    k += size
    per = size // nc - 1 if nc else 0
    rows = flat.reshape(nc, per + 1) if nc else flat.reshape(0, 1)
    if nc and not np.all(rows[:, 0] == per):
        raise ValueError(f"{filename}: faces of different sizes")
    if w[k] != "CELL_TYPES" or int(w[k + 1]) != nc:
        raise ValueError(f"{filename}: CELL_TYPES expected")
    types = np.array([int(v) for v in w[k + 2:k + 2 + nc]], dtype=np.int64)
    k += 2 + nc
    if w[k] != "CELL_DATA" or int(w[k + 1]) != nc:
        raise ValueError(f"{filename}: CELL_DATA expected")
    k += 2
    data = {}
    for _ in range(2):
        if w[k] != "SCALARS" or w[k + 4:k + 6] != ["LOOKUP_TABLE", "default"]:
            raise ValueError(f"{filename}: SCALARS <name> int 1 expected")
        data[w[k + 1]] = np.array([int(v) for v in w[k + 6:k + 6 + nc]], dtype=np.int64)
        k += 6 + nc
    if set(data) != {"patch", "kind"}:
        raise ValueError(f"{filename}: CELL_DATA patch and kind expected")
    return points, rows[:, 1:].copy(), types, data["patch"], data["kind"]


_FOAM_CLASSES = {"points": "vectorField", "faces": "faceList", "owner": "labelList", "neighbour": "labelList", "boundary": "polyBoundaryMesh"}


def _foam_header(name, note=None):
    lines = ["FoamFile", "{", "    version     2.0;", "    format      ascii;", f"    class       {_FOAM_CLASSES[name]};"]
    if note:
        lines.append(f'    note        "{note}";')
    return "\n".join(lines + ['    location    "constant/polyMesh";', f"    object      {name};", "}", "", ""])


def polymesh_patch_type(kind, empty_caps=False):
    """OpenFOAM patch type of a patch kind: wall and unassigned -> wall, inlet / outlet -> patch, periodic -> cyclic, hub / shroud -> wall
    (empty when the layer is the one-cell extrusion of a plane mesh)."""
    if kind == _capi.TM_PATCH_PERIODIC:
        return "cyclic"
    if kind in (_capi.TM_BC_INLET, _capi.TM_BC_OUTLET):
        return "patch"
    if kind in (_capi.TM_PATCH_HUB, _capi.TM_PATCH_SHROUD) and empty_caps:
        return "empty"
    return "wall"


def write_polymesh(directory, points, faces, boundary=None, empty_caps=False):
    """An OpenFOAM polyMesh directory -- ASCII `points`, `faces`, `owner`, `neighbour`, `boundary`, doubles with 17 significant digits --
    from the welded `points` ((nk * nodes, 3)) and a weld.Faces of a stacked mesh (quadrilateral faces: interior faces first in
    upper-triangular order, every normal owner -> neighbour or outward, then the patches of `boundary`, default faces.boundary, as
    contiguous startFace / nFaces ranges).  Patch names are the Boundary's; types by polymesh_patch_type; each periodic pair becomes two
    `cyclic` patches that name each other, `transform translational` with the patch's translation as separationVector (own face +
    vector = partner's face).  Nobody has run OpenFOAM's checkMesh on such a directory.  Returns the five file names."""
    boundary = faces.boundary if boundary is None else boundary
    pts = np.ascontiguousarray(points, dtype=np.float64)
    F = np.ascontiguousarray(faces.faces)
    if pts.ndim != 2 or pts.shape[1] != 3 or F.ndim != 2 or F.shape[1] != 4:
        raise ValueError("a polyMesh needs a stacked mesh: points (n, 3) and quadrilateral faces (with a plane mesh: one extruded layer)")
    if len(boundary.faces) != len(F) - faces.ninternal:
        raise ValueError("the boundary is not the one of these faces")
    os.makedirs(directory, exist_ok=True)
    names = {k: os.path.join(directory, k) for k in _FOAM_CLASSES}
    note = f"nPoints: {len(pts)} nCells: {faces.ncells} nFaces: {len(F)} nInternalFaces: {faces.ninternal}"
    with open(names["points"], "w") as fh:
        fh.write(_foam_header("points") + f"{len(pts)}\n(\n" + "".join("(%.17g %.17g %.17g)\n" % tuple(p) for p in pts.tolist()) + ")\n")
    with open(names["faces"], "w") as fh:
        fh.write(_foam_header("faces") + f"{len(F)}\n(\n" + "".join("4(%d %d %d %d)\n" % tuple(r) for r in F.tolist()) + ")\n")
    with open(names["owner"], "w") as fh:
        fh.write(_foam_header("owner", note) + f"{len(F)}\n(\n" + "".join(f"{v}\n" for v in faces.owner.tolist()) + ")\n")
    with open(names["neighbour"], "w") as fh:
        fh.write(_foam_header("neighbour", note) + f"{faces.ninternal}\n(\n" + "".join(f"{v}\n" for v in faces.neighbour.tolist()) + ")\n")
    with open(names["boundary"], "w") as fh:
        fh.write(_foam_header("boundary") + f"{len(boundary.patches)}\n(\n")
        for r in boundary.patches:
            kind = polymesh_patch_type(r.kind, empty_caps)
            fh.write(f"    {r.name}\n    {{\n        type            {kind};\n")
            if kind == "cyclic":
                fh.write(f"        neighbourPatch  {boundary.patches[r.partner].name};\n        transform       translational;\n")
                fh.write("        separationVector (%.17g %.17g 0);\n" % (r.translation[0], r.translation[1]))
            fh.write(f"        nFaces          {r.faces};\n        startFace       {faces.ninternal + r.begin};\n    }}\n")
        fh.write(")\n")
    return [names[k] for k in ("points", "faces", "owner", "neighbour", "boundary")]


def _foam_body(filename, name):
    with open(filename) as fh:
        text = fh.read()
    head, sep, body = text.partition("}\n")
    if not head.startswith("FoamFile") or not sep or f"object      {name};" not in head or f"class       {_FOAM_CLASSES[name]};" not in head:
        raise ValueError(f"{filename}: not an ASCII OpenFOAM {name} file")
    count, _, rest = body.lstrip().partition("\n(\n")
    return int(count), rest[:rest.rindex(")")]


def read_polymesh(directory):
    """-> dict of a directory written by write_polymesh: points (n, 3) float64 bit for bit, faces (n, 4), owner, neighbour (int64) and
    boundary, a list of dicts name, type, nFaces, startFace and for cyclic patches neighbourPatch, separationVector."""
    n, body = _foam_body(os.path.join(directory, "points"), "points")
    points = np.array([float(v) for v in body.replace("(", " ").replace(")", " ").split()], dtype=np.float64).reshape(n, 3)
    n, body = _foam_body(os.path.join(directory, "faces"), "faces")
    flat = np.array([int(v) for v in body.replace("4(", " ").replace(")", " ").split()], dtype=np.int64)
    out = {"points": points, "faces": flat.reshape(n, 4)}
    for name in ("owner", "neighbour"):
        n, body = _foam_body(os.path.join(directory, name), name)
        out[name] = np.array([int(v) for v in body.split()], dtype=np.int64)
        if len(out[name]) != n:
            raise ValueError(f"{directory}/{name}: {len(out[name])} labels where {n} are announced")
    n, body = _foam_body(os.path.join(directory, "boundary"), "boundary")
    patches = []
    for chunk in body.split("}")[:-1]:
        name, _, entries = chunk.partition("{")
        rec = {"name": name.strip()}
        for entry in entries.split(";"):
            w = entry.split()
            if not w:
                continue
            if w[0] == "separationVector":
                rec[w[0]] = tuple(float(v.strip("()")) for v in w[1:])
            elif w[0] in ("nFaces", "startFace"):
                rec[w[0]] = int(w[1])
            else:
                rec[w[0]] = w[1]
        patches.append(rec)
    if len(patches) != n:
        raise ValueError(f"{directory}/boundary: {len(patches)} patches where {n} are announced")
    out["boundary"] = patches
    return out


def _format_of(filename):
    ext = os.path.splitext(filename)[1].lower()
    if ext == ".cgns":
        raise OutputFormatNotEnabled("CGNS output needs the cgns library (reference: -Duse-cgns); use .xyz / .p3d (PLOT3D)")
    if ext not in (".xyz", ".p3d", ".x"):
        raise OutputFormatNotEnabled(f"unknown output format {ext!r}; supported: .xyz / .p3d / .x (PLOT3D)")
    return "plot3d"


def write_mesh(mesh, filename):
    """discrete.zig:197-216 Mesh.write"""
    _format_of(filename)
    sizes = [(b.points.data.shape[0], b.points.data.shape[1]) for b in mesh.blocks]
    write_plot3d(filename, sizes, [block_planes(b.points.data) for b in mesh.blocks])


def write_smoother(smoother, filename, with_control_function=True):
    """smooth.zig:396-414 RowCompressedMatrixSystem2d.write: coordinates resident in the handle + control function."""
    _format_of(filename)
    mesh = smoother._mesh
    L = _capi.lib()
    dp = C.POINTER(C.c_double)
    sizes, planes, fields = [], [], []
    for b, blk in enumerate(mesh.blocks):
        ni, nj = blk.points.data.shape[0], blk.points.data.shape[1]
        x, y, p, q = (np.empty(ni * nj, dtype=np.float64) for _ in range(4))
        _capi.check(L.tm_smoother_export_soa(smoother._h, b, x.ctypes.data_as(dp), y.ctypes.data_as(dp),
                                             p.ctypes.data_as(dp) if with_control_function else None,
                                             q.ctypes.data_as(dp) if with_control_function else None))
        sizes.append((ni, nj))
        planes.append((x, y))
        fields.append([p, q])
    write_plot3d(filename, sizes, planes)
    if with_control_function:
        write_plot3d_function(os.path.splitext(filename)[0] + ".f", sizes, fields)
