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
