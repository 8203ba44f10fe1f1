"""GPU: the wall distance of the welded mesh on the device (kernel K20: tm_wall_distance, tm_smoother_wall_distance) against the host twin.
In every case distance, face and image equal the host twin's exactly, the culled launch equals TM_WALL_NO_CULL exactly, the record equals
the host's in every field but pairs_evaluated, a second call is bit-identical, and on cases of 4 groups or more the culled launch
evaluates fewer pairs than there are -- a condition with no ratio attached.

The shapes are those where the kernel can go wrong: less than a wave and a group; a group boundary +- 1 with a point count that is no
multiple of 64 or 256; more groups than one LDS chunk holds (WD_CHUNK = 64 groups of WD_GROUP = 64 primitives: single_block(n, 5) with
both long sides as walls has 2 (n - 1) faces, so n = 32 * WD_CHUNK + 2 = 2050 gives 4098 faces in 65 groups); patches that meet inside
a group; ties; a NaN point inside a full wave; many workgroups of triangles with a flipped block; the examples as their files say.

strip(2, 301, 203) on 3 layers has 366 009 nodes and 491 216 triangles: its host twin would take over an hour, so that shape is held to
the device-only conditions (culled == not culled, repeat, record against counts) and a strip(2, 41, 29) of the same construction is held
to the host twin as well."""
import logging
import os
import threading

import numpy as np
import pytest

from tests import test_wall_distance_cpu as wcpu
from tests import test_weld_boundary_cpu as bcpu
from tests import test_weld_cpu as cpu
from turbomesh_amd import _capi, configs, output, stack, weld
from turbomesh_amd.boundary import Condition, ConditionTag, Range, Side
from turbomesh_amd.smoothing import smooth, solver

pytestmark = pytest.mark.gpu

RECORD = ["points", "faces", "primitives", "images", "groups", "on_wall", "nan_points", "nearest_via_image", "max_point", "max_distance"]


def same(a, b):
    nan = np.isnan(a.distance)
    assert np.array_equal(nan, np.isnan(b.distance)) and np.array_equal(a.distance[~nan], b.distance[~nan])
    assert np.array_equal(a.face, b.face) and np.array_equal(a.image, b.image)
    for k in RECORD:
        assert getattr(a.info, k) == getattr(b.info, k), k


def device_runs(faces, pts, images=None):
    """culled, not culled and culled again on the device: equal exactly -> the culled result"""
    dev = weld.wall_distance_of(faces, pts, images)
    every = weld.wall_distance_of(faces, pts, images, cull=False)
    same(every, dev)
    again = weld.wall_distance_of(faces, pts, images)
    same(again, dev)
    assert again.info.pairs_evaluated == dev.info.pairs_evaluated
    i = dev.info
    total = i.points * i.primitives * i.images
    assert every.info.pairs_evaluated == (i.points - i.nan_points) * i.primitives * i.images
    if i.groups >= 4:
        assert dev.info.pairs_evaluated < total
    print(f"{i.points} points, {i.primitives} primitives in {i.groups} groups, {i.images} image(s): {dev.info.pairs_evaluated} of {total} pairs evaluated")
    return dev


def check(faces, pts, images=None):
    dev = device_runs(faces, pts, images)
    same(dev, weld.wall_distance_of(faces, pts, images, host=True))
    return dev


def test_one_face_three_points():
    wd = check(np.array([[0, 1]], dtype=np.int32), np.array([[0.0, 0.0], [1.0, 0.0], [0.5, 0.25]]))
    assert np.array_equal(wd.distance, [0.0, 0.0, 0.25]) and wd.info.groups == 1


@pytest.mark.parametrize("nfaces", [65, 129])
def test_a_group_boundary_plus_one_with_261_points(nfaces):
    pts = bcpu.plane_case("plate")[2]
    assert len(pts) == 261
    k = np.arange(nfaces)
    faces = np.stack([(5 * k) % 261, (5 * k + 1 + k % 3) % 261], axis=1).astype(np.int32)   # segments between nodes of the mesh, none degenerate
    wd = check(faces, pts)
    assert wd.info.groups == (nfaces + 63) // 64


def test_more_groups_than_one_lds_chunk():
    n = 32 * _capi.WD_CHUNK + 2
    mesh = configs.single_block(n, 5)
    w = weld.Weld(mesh, host=True)
    b = w.boundary(1)
    walls = np.nonzero((b.origin[:, 1] == int(Side.i_min)) | (b.origin[:, 1] == int(Side.i_max)))[0]
    wd = check(b.faces[walls], w.points(mesh))
    assert wd.info.faces == 2 * (n - 1) and wd.info.groups == _capi.WD_CHUNK + 1


def test_patches_that_meet_inside_a_group():
    mesh = configs.single_block(21, 17)
    for side, n, kind in ((Side.i_min, 21, ConditionTag.wall), (Side.i_max, 21, ConditionTag.wall), (Side.j_min, 17, ConditionTag.inlet), (Side.j_max, 17, ConditionTag.outlet)):
        mesh.boundary_conditions.append(Condition(Range(0, side, 0, n - 1), kind))
    w = weld.Weld(mesh, host=True)
    b = w.boundary(1)
    faces, index, images = b.wall_faces(("wall", "inlet", "outlet"))
    assert len(faces) == 72 and len(images) == 1
    wd = check(faces, w.points(mesh))
    assert wd.info.on_wall == 72


def test_a_wall_node_shared_by_two_faces_goes_to_the_smaller_face():
    mesh = wcpu.unit_square(9)
    w = weld.Weld(mesh, host=True)
    b = w.boundary(1)
    wall = np.nonzero(b.origin[:, 1] == int(Side.i_min))[0]
    wd = check(b.faces[wall], w.points(mesh))
    assert np.array_equal(wd.distance, (np.arange(81) // 9) / 8.0) and np.array_equal(wd.face, np.maximum(np.arange(81) % 9 - 1, 0))


def test_the_exact_image_tie():
    faces, pts, images = wcpu.tie_case()
    wd = check(faces, pts, images)
    assert np.array_equal(wd.distance[9:], np.full(9, 0.5)) and not wd.image.any() and np.array_equal(wd.face[9:], np.maximum(np.arange(9) - 1, 0))


def test_a_nan_point_inside_a_full_wave():
    _, w, pts = bcpu.plane_case("plate")[:3]
    pts = pts.copy()
    b = w.boundary(1)
    used = np.unique(b.faces)
    victim = int(np.setdiff1d(np.arange(64, 128), used)[0])   # in the second wave, not a node of the wall
    pts[victim, 0] = np.nan
    wd = check(b.faces, pts)
    assert np.isnan(wd.distance[victim]) and wd.face[victim] == -1 and wd.image[victim] == -1 and wd.info.nan_points == 1


def layered(mesh, nk):
    w = weld.Weld(mesh, host=True)
    blocks = bcpu.planar_blocks(mesh, nk)
    o = tuple(stack.quality_of_planes(*blk).orientation for blk in blocks)
    b = w.boundary(1, layers=nk, orientation=o)
    return w.points(blocks), b, o


def test_a_small_strip_of_triangles_with_a_flipped_block():
    pts, b, o = layered(configs.strip(2, 41, 29, reverse_odd=True, tfi=cpu.oracle_tfi), 3)
    assert sorted(o) == [-1, 1]
    faces, index, images = b.wall_faces(("hub", "shroud", "unassigned"))
    wd = check(faces, pts)
    assert wd.info.primitives == 2 * len(faces) and wd.info.on_wall == len(np.unique(faces))


def test_many_workgroups_of_triangles_and_a_flipped_block():
    pts, b, o = layered(configs.strip(2, 301, 203, reverse_odd=True, tfi=cpu.oracle_tfi), 3)
    assert sorted(o) == [-1, 1]
    faces, index, images = b.wall_faces(("hub", "shroud", "unassigned"))
    assert len(faces) == 2 * 2 * 300 * 202 + 2 * (2 * 202 + 2 * 2 * 300)
    wd = device_runs(faces, pts)   # the host twin of this shape: see the module's docstring
    nodes = len(pts) // 3
    assert wd.info.on_wall == len(np.unique(faces)) and wd.info.nan_points == 0
    assert np.array_equal(wd.distance[:nodes], np.zeros(nodes)) and np.array_equal(wd.distance[2 * nodes:], np.zeros(nodes))
    assert (wd.distance[nodes:2 * nodes] <= 0.125).all() and (wd.distance[nodes:2 * nodes] > 0).sum() > 0


@pytest.mark.parametrize("name", ["T106", "LS89"])
def test_the_examples_as_their_files_say(name):
    pts, b, faces, index, images, host = wcpu.plane_run(name, ("unassigned",))
    assert len(images) == 3
    wd = check(faces, pts, images)
    assert wd.info.nearest_via_image > 0
    wdev = weld.Weld(cpu.case(name)[0])   # Weld on the device end to end: face refers to Boundary.faces
    via = wdev.wall_distance(pts, wdev.boundary(1, orientation=bcpu.orientation_of(name)), kinds=("unassigned",))
    same(via, host)


def test_rotational_images():
    w, pts, b, faces, index, images = wcpu.rotational_case()
    wd = check(faces, pts, images)
    assert wd.info.images == 3


def test_wall_distance_of_the_coordinates_resident_in_a_handle():
    mesh = configs.two_by_two(33, 33, tfi=cpu.oracle_tfi)
    d = mesh.blocks[0].points.data
    d[1:-1, 1:-1] += 0.001 * np.sin(37.0 * np.arange(d[1:-1, 1:-1].size)).reshape(d[1:-1, 1:-1].shape)   # something to smooth
    w = weld.Weld(mesh)
    with smooth.Smoother(mesh, solver.Option.hip(inner=solver.Inner.relax)) as sm:
        sm.iterate(3)
        got = sm.wall_distance()
        o = [q.orientation for q in sm.quality()[0]]
        want = w.wall_distance(w.points(sm), w.boundary(1, orientation=o))
    same(got, want)
    assert got.info.faces == 256 and got.info.on_wall == 256 and got.info.max_distance > 0.0


def test_rank_hooks_are_refused():
    from tests.test_gpu_virtual_ranks import ThreadHooks, _Shared

    world, owner = 2, [0, 1, 0, 1]
    opt = solver.Option.hip(inner=solver.Inner.relax)
    shared = _Shared(world)
    ms = [configs.strip(4, 17, 24, reverse_odd=True) for _ in range(world)]
    hooks, codes, errors = [None] * world, [None] * world, []
    lock = threading.Lock()

    def work(r):
        try:
            with lock:
                hooks[r] = ThreadHooks(shared, ms[r], owner, r, world, opt)
            shared.barrier.wait()
            with lock:
                try:
                    hooks[r].smoother.wall_distance()
                except _capi.TmError as e:
                    codes[r] = e.code
        except BaseException as e:  # pragma: no cover
            errors.append((r, e))
            shared.barrier.abort()

    threads = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    for h in hooks:
        if h is not None:
            h.smoother.close()
    assert not errors, errors
    assert codes == [_capi.TM_E_UNSUPPORTED] * world


def test_cli_writes_the_wall_distance_of_t106(tmp_path, monkeypatch, caplog):
    from turbomesh_amd.__main__ import main

    monkeypatch.chdir(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))   # profile files are named relative to the working directory
    out = str(tmp_path / "t106.vtk")
    with caplog.at_level(logging.INFO, logger="weld"):
        main([os.path.join("examples", "T106", "T106.json"), "--hip", "--weld", "--wall-distance", "--output", out])
    assert sorted(os.listdir(tmp_path)) == ["t106.vtk"]
    field = output.read_vtk_point_data(out)["wall_distance"]
    pts = output.read_vtk_lagrange(out)[0][:, :2]   # %.17g: the welded points of the run, bit for bit
    w = weld.Weld(cpu.case("T106")[0])
    want = w.wall_distance(pts, w.boundary(1, orientation=bcpu.orientation_of("T106")))   # the orientation the handle takes from its quality report
    assert np.array_equal(field, want.distance) and want.info.faces == 340 and want.info.images == 3
    lines = [r.getMessage() for r in caplog.records if r.name == "weld" and "nodes nearest to an image" in r.getMessage()]
    assert len(lines) == 1 and f"{want.info.nearest_via_image} nodes nearest to an image" in lines[0] and want.info.nearest_via_image > 0
    with pytest.raises(SystemExit) as e:
        main([os.path.join("examples", "T106", "T106.json"), "--hip", "--wall-distance", "--output", out])
    assert e.value.code == 2


def test_cpp_mirror_prints_the_record_of_a_strip():
    import subprocess

    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "turbomesh_amd", "tm_harness")
    for args, faces in ((["33", "41", "3"], 2 * 40 + 6 * 32), (["17", "21", "2", "3"], (2 * 20 + 4 * 16) * 2 + 2 * 2 * 16 * 20)):
        r = subprocess.run([exe, "wall-distance"] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert f"points, {faces} faces" in r.stdout and "device equals host: yes" in r.stdout and "culled equals not culled: yes" in r.stdout
