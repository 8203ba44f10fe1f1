"""GPU: the welded numbering on the device (kernel K18: tm_weld_map / tm_weld_points / tm_weld_cells / tm_smoother_weld) against the host
definition -- map, every field of info, welded planes and cells equal exactly -- on the topologies of tests/test_weld_cpu.py and on the
shapes where the kernels can go wrong: less than one scan tile, many tiles, tile sums that span more than one tile themselves, links
across tile boundaries, high-order and 3-D cells, the elevated planes of K13, the coordinates resident in a handle."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

from tests import test_weld_cpu as cpu
from turbomesh_amd import _capi, configs, highorder, output, weld
from turbomesh_amd.boundary import Connection, Range, Side
from turbomesh_amd.discrete import Block2d, Mesh
from turbomesh_amd.smoothing import smooth, solver
from turbomesh_amd.types import Mat2d

pytestmark = pytest.mark.gpu


def same_info(a, b):
    assert dataclasses.asdict(a) == dataclasses.asdict(b)


def check_against_host(mesh, wh, points_of=None, orders=(1,), layers=None):
    wd = weld.Weld(mesh)
    assert np.array_equal(wd.map, wh.map)
    same_info(wd.info, wh.info)
    if points_of is not None:
        pd, ph = wd.points(points_of), wh.points(points_of)
        assert pd.shape == ph.shape and np.array_equal(pd, ph)
        same_info(wd.info, wh.info)   # max_gap, gap_node and periodic_gap included
    for p in orders:
        assert np.array_equal(wd.cells(p, layers), wh.cells(p, layers))
    return wd


@pytest.mark.parametrize("name", sorted(cpu.TABLE))
def test_every_topology_of_the_table(name):
    # two_by_two: 288 nodes, less than one scan tile; T106: 13 tiles, perimeter links scattered over eight blocks
    mesh, wh, _, _, _ = cpu.case(name)
    wd = check_against_host(mesh, wh, points_of=mesh)
    assert wd.nodes == cpu.TABLE[name][2]


def test_tile_sums_that_span_more_than_one_tile():
    # 1500 x 1501 = 2 251 500 nodes = 1100 scan tiles of 2048: the tile sums themselves fill more than one tile of 1024, so the second
    # level of the scan runs.  The block is closed on itself by j_min <-> j_max: every row ends in a node that is not an owner, so the
    # offsets of all tiles matter.  Sizes only: the numbering reads no coordinates.
    ni, nj = 1500, 1501
    assert -(-(ni * nj) // 2048) > 1024
    mesh = Mesh()
    mesh.addBlock("big", Block2d(Mat2d.placeholder((ni, nj))))
    mesh.connections.append(Connection((Range(0, Side.j_min, 0, nj - 1), Range(0, Side.j_max, 0, nj - 1)), None))
    wh = weld.Weld(mesh, host=True)
    wd = check_against_host(mesh, wh, orders=())
    assert wd.nodes == ni * nj - nj and wd.info.classes_2 == nj
    assert np.array_equal(wd.map.reshape(nj, ni)[:, -1], wd.map.reshape(nj, ni)[:, 0])


def test_links_across_tile_boundaries():
    mesh = configs.strip(2, 1030, 1030)   # 1 060 900 nodes per block: neither the block nor its rows end on a tile of 2048
    wh = weld.Weld(mesh, host=True)
    wd = check_against_host(mesh, wh, points_of=mesh)
    assert wd.nodes == 2 * 1030 * 1030 - 1030 and wd.info.max_gap == 0.0


def test_order_5_cells_of_t106():
    mesh, wh, _, _, _ = cpu.case("T106")
    cells = weld.Weld(mesh).cells(5)
    assert cells.shape == (960, 36) and np.array_equal(cells, wh.cells(5))


def test_hexahedra_of_order_2_on_three_layers():
    mesh = configs.two_by_two(7, 7, tfi=cpu.oracle_tfi)
    blocks = [tuple(np.stack([p * (1.0 + k / 3.0) if c < 2 else p + k / 7.0 for k in range(3)]) for c, p in enumerate((X, Y, np.zeros_like(X))))
              for X, Y in cpu.R.mesh_planes(mesh)]
    wd = check_against_host(mesh, weld.Weld(mesh, host=True), points_of=blocks, orders=(1, 2), layers=3)
    assert wd.cells(2, 3).shape == (36, 27)


def test_welded_k13_planes_of_t106():
    # Gauss-Lobatto nodes of order 2: the two sides of an interface sum in their own index order, so max_gap is the rounding they
    # differ by; device and host must report the same value at the same node
    mesh, wh, _, _, _ = cpu.case("T106")
    hom = highorder.Elevation(2, "gauss_lobatto").mesh(mesh)
    wd = weld.Weld(mesh)
    pd, ph = wd.points(hom), weld.Weld(mesh, host=True).points(hom)
    assert np.array_equal(pd, ph)
    hi = weld.Weld(mesh, host=True)
    hi.points(hom)
    same_info(wd.info, hi.info)
    print(f"T106, order 2, Gauss-Lobatto: max_gap {wd.info.max_gap:.3e} at node {wd.info.gap_node}")


@pytest.mark.parametrize("name", ["two_by_two", "cut"])
def test_coordinates_resident_in_a_handle(name):
    # the cut of the table trades the two ranges of four interfaces, which a handle refuses as the reference does (ranges[0].block <
    # ranges[1].block, smooth.zig:562): the handle gets the same cut, flips included, with its ranges in the order it accepts
    mesh = cpu.TABLE[name][0]() if name != "cut" else cpu.meshes.cut(cpu.warped_grid(23, 31), **cpu.CUT)
    d = mesh.blocks[0].points.data
    d[1:-1, 1:-1] += 0.002 * np.sin(37.0 * np.arange(d[1:-1, 1:-1].size)).reshape(d[1:-1, 1:-1].shape)   # something to smooth
    wd = weld.Weld(mesh)
    with smooth.Smoother(mesh, solver.Option.hip()) as sm:
        sm.iterate(2)
        pts = wd.points(sm)
        N = wd.info.nodes_in
        m, X, Y, rec = np.empty(N, np.int32), np.empty(N), np.empty(N), _capi.tm_weld_info()   # the C entry point, map included
        _capi.check(_capi.lib().tm_smoother_weld(sm._h, m.ctypes.data_as(C.POINTER(C.c_int32)), _capi.f64ptr(X), _capi.f64ptr(Y), C.byref(rec)))
        um = sm.weld()
        sm.download()
    wh = weld.Weld(mesh, host=True)
    ph = wh.points(mesh)   # the downloaded coordinates through the host definition
    assert np.array_equal(pts, ph) and np.array_equal(m, wh.map)
    assert np.array_equal(np.stack([X[:wh.nodes], Y[:wh.nodes]], axis=1), ph)
    same_info(wd.info, wh.info)
    same_info(weld.WeldInfo.from_struct(rec), wh.info)
    assert np.array_equal(um.points, ph) and np.array_equal(um.cells, wh.cells(1)) and um.cell_type == 9


def test_cli_welds_t106_at_order_2(tmp_path, monkeypatch):
    from turbomesh_amd.__main__ import main

    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    monkeypatch.chdir(gold)   # profile files are named relative to the working directory
    out = str(tmp_path / "t.vtk")
    main([os.path.join("examples", "T106", "T106.json"), "--hip", "--order", "2", "--weld", "--output", out])
    pts, cells, types = output.read_vtk_lagrange(out)
    assert len(pts) == 24430 and cells.shape == (6000, 9) and np.all(types == 70)


def test_cli_welds_stacked_cuts(tmp_path, monkeypatch):
    from turbomesh_amd.__main__ import main

    monkeypatch.chdir(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    cfg = os.path.join("examples", "T106", "T106.json")
    out = str(tmp_path / "s.vtk")
    main([cfg, "--hip", "--iterations", "2", "--stack", cfg, "--span", "0,0.1", "--layers", "3", "--weld", "--output", out])
    pts, cells, types = output.read_vtk_lagrange(out)
    assert len(pts) == 3 * 24430 and cells.shape == (2 * 24000, 8) and np.all(types == 12)
    assert np.array_equal(pts[:24430, :2], pts[24430:2 * 24430, :2])   # planar mapping: the layers repeat the cut


def test_cpp_mirror_welds_a_strip():
    import subprocess

    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "turbomesh_amd", "tm_harness")
    r = subprocess.run([exe, "weld", "33", "41", "3"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "weld: 4059 -> 3977 nodes" in r.stdout and "device equals host: yes" in r.stdout
