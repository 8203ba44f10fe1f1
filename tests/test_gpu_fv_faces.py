"""GPU: the face-based view of the welded mesh and its finite-volume metrics on the device (kernel K21: tm_weld_faces, tm_fv_metrics,
tm_smoother_fv_report) against the host definition -- every integer list equal exactly, every per-cell and per-face double and every
extreme of the record with its index equal bit for bit (one shared header), total_volume within 2 (n - 1) 2^-53 sum |V| (identical terms,
two orders of summation), two calls bit-identical -- on the topologies of tests/test_weld_cpu.py and on the shapes where the kernels can go
wrong: fewer cells than a wave, rows that are no multiple of 64 with a flipped block and a scan over several partial tiles, layers, a
ring two cells around."""
import dataclasses
import os

import numpy as np
import pytest

from tests import test_fv_faces_cpu as fcpu
from tests import test_weld_boundary_cpu as bcpu
from tests import test_weld_cpu as cpu
from turbomesh_amd import _capi, configs, output, stack, weld
from turbomesh_amd.smoothing import smooth, solver

pytestmark = pytest.mark.gpu
FIELDS = ("volume", "centre", "closedness", "area", "face_centre", "cos", "skewness")
SUMMED = ("total_volume",)


def same_report(rd, rh):
    """device against host: every field bit for bit except total_volume, which is summed in another order"""
    for fld in dataclasses.fields(rh):
        a, b = getattr(rd, fld.name), getattr(rh, fld.name)
        if fld.name in FIELDS:
            assert (a is None) == (b is None)
            if a is not None:
                nan = np.isnan(b)   # 0 / 0 of a degenerate cell is a NaN on both sides; its sign bit is the processor's
                assert a.shape == b.shape and np.array_equal(np.isnan(a), nan) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64)), fld.name
        elif fld.name not in SUMMED:
            assert a == b and (not isinstance(b, float) or np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)), fld.name
    n = rh.cells
    bar = 2.0 * (n - 1) * 2.0 ** -53 * (float(np.abs(rh.volume).sum()) if rh.volume is not None else abs(rh.total_volume) * n)
    assert abs(rd.total_volume - rh.total_volume) <= bar, (rd.total_volume, rh.total_volume, bar)


def check_against_host(mesh, pts, layers=None, orientation=None, wh=None):
    wh = wh or weld.Weld(mesh, host=True)
    wd = weld.Weld(mesh)
    fh, fd = wh.faces(layers, orientation), wd.faces(layers, orientation)
    for k in fcpu.LISTS:
        a, b = getattr(fd, k), getattr(fh, k)
        assert a.dtype == np.int32 and a.shape == b.shape and np.array_equal(a, b), k
    assert fd.ninternal == fh.ninternal and fd.ncells == fh.ncells
    rh, rd = fh.metrics(pts, fields=True), fd.metrics(pts, fields=True)
    same_report(rd, rh)
    again = wd.faces(layers, orientation)
    assert all(np.array_equal(getattr(again, k), getattr(fd, k)) for k in fcpu.LISTS)
    ra = again.metrics(pts, fields=True)
    assert ra.total_volume == rd.total_volume and ra.volume.tobytes() == rd.volume.tobytes() and ra.cos.tobytes() == rd.cos.tobytes()   # the same bits from run to run
    assert dataclasses.astuple(fd.metrics(pts))[:18] == dataclasses.astuple(rd)[:18]   # the record does not depend on the optional outputs
    return fd, rd


@pytest.mark.parametrize("name", sorted(cpu.TABLE))
def test_every_topology_of_the_table(name):
    mesh, w, pts, o, _, _ = fcpu.plane_case(name)
    fd, _ = check_against_host(mesh, pts, orientation=o, wh=w)
    assert fd.ninternal == fcpu.INTERIOR[name]


def test_four_cells_less_than_a_wave():
    mesh = configs.single_block(3, 3)
    wh = weld.Weld(mesh, host=True)
    fd, rd = check_against_host(mesh, wh.points(mesh), wh=wh)
    assert (fd.ncells, fd.ninternal, len(fd.faces)) == (4, 4, 12) and rd.negative_cells == 0


@pytest.mark.parametrize("layers", [None, 3])
def test_rows_of_300_cells_a_flipped_block_and_a_scan_over_partial_tiles(layers):
    mesh = configs.strip(2, 301, 203, reverse_odd=True, tfi=cpu.oracle_tfi)
    wh = weld.Weld(mesh, host=True)
    if layers:
        blocks = bcpu.planar_blocks(mesh, layers)
        o = tuple(stack.quality_of_planes(*blk).orientation for blk in blocks)
        pts = wh.points(blocks)
    else:
        o = tuple(q.orientation for q in mesh.quality(host=True)[0])
        pts = wh.points(mesh)
    assert sorted(o) == [-1, 1]
    fd, rd = check_against_host(mesh, pts, layers=layers, orientation=o, wh=wh)
    cells = 2 * 300 * 202 * (layers - 1 if layers else 1)
    assert fd.ncells == cells and fd.ninternal == ((6 if layers else 4) * cells - len(fd.boundary.faces)) // 2   # 119 (237) tiles of the scan, the last one partial
    assert rd.negative_cells == 0 and rd.inverted_faces == 0


def test_more_than_2_to_20_cells_take_the_second_level_of_the_scan():
    mesh = configs.single_block(1025, 1027)   # 1024 x 1026 cells: 1026 tiles of 1024 counts, whose sums span two tiles themselves
    wh, wd = weld.Weld(mesh, host=True), weld.Weld(mesh)
    fh, fd = wh.faces(), wd.faces()
    assert fh.ncells == 1024 * 1026 > 2 ** 20 and fh.ninternal == 2 * 1024 * 1026 - 1024 - 1026
    for k in fcpu.LISTS:
        assert np.array_equal(getattr(fd, k), getattr(fh, k)), k


def test_a_ring_two_cells_around():
    mesh = cpu.polar_ring(7, 3)
    wh = weld.Weld(mesh, host=True)
    for o in ((1,), (-1,)):
        fd, _ = check_against_host(mesh, wh.points(mesh), orientation=o, wh=wh)
        pairs = list(zip(fd.owner[:fd.ninternal].tolist(), fd.neighbour.tolist()))
        assert len({p for p in pairs if pairs.count(p) == 2}) == 6
    with pytest.raises(_capi.TmError) as e:
        weld.Weld(cpu.polar_ring(7, 2)).faces(orientation=(1,))
    assert e.value.code == _capi.TM_E_MISMATCH


def test_report_of_the_coordinates_resident_in_a_handle():
    mesh = configs.two_by_two(33, 33, tfi=cpu.oracle_tfi)
    d = mesh.blocks[0].points.data
    d[1:-1, 1:-1] += 0.001 * np.sin(37.0 * np.arange(d[1:-1, 1:-1].size)).reshape(d[1:-1, 1:-1].shape)   # something to smooth
    wd = weld.Weld(mesh)
    with smooth.Smoother(mesh, solver.Option.hip(inner=solver.Inner.relax)) as sm:
        sm.iterate(3)
        got = sm.fv_report()
        o = [q.orientation for q in sm.quality()[0]]
        pts = wd.points(sm)
        sm.download()
    want = wd.faces(orientation=o).metrics(pts)
    assert got == want and got.cells == 4 * 32 * 32 and got.min_volume > 0   # the same kernels on the same planes: the same bits
    wh = weld.Weld(mesh, host=True)
    assert np.array_equal(wh.points(mesh), pts)   # the composition on the downloaded coordinates
    same_report(want, wh.faces(orientation=o).metrics(pts))


def test_cli_writes_the_polymesh_of_t106(tmp_path, monkeypatch, caplog):
    import logging

    from turbomesh_amd.__main__ import main

    monkeypatch.chdir(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))   # profile files are named relative to the working directory
    d = str(tmp_path / "polyMesh")
    with caplog.at_level(logging.INFO, logger="weld"):
        main([os.path.join("examples", "T106", "T106.json"), "--hip", "--weld", "--polymesh", d, "--fv-report", "--output", str(tmp_path / "t106.vtk")])
    assert sorted(os.listdir(d)) == ["boundary", "faces", "neighbour", "owner", "points"]
    got = output.read_polymesh(d)
    assert got["faces"].shape == (47570 + 860 + 2 * 24000, 4) and len(got["neighbour"]) == 47570 and len(got["points"]) == 2 * 24430
    assert [p["type"] for p in got["boundary"]].count("empty") == 2 and [p["type"] for p in got["boundary"]].count("cyclic") == 6
    assert any("internal" in r.getMessage() and "24000 cells" in r.getMessage() for r in caplog.records if r.name == "weld")


def test_cpp_mirror_lists_the_faces_of_a_strip():
    import subprocess

    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "turbomesh_amd", "tm_harness")
    for args, cells in ((["33", "41", "3"], 3 * 32 * 40), (["33", "41", "3", "5"], 3 * 32 * 40 * 4)):
        r = subprocess.run([exe, "fv"] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert f"fv: {cells} cells" in r.stdout and "device equals host: yes" in r.stdout
