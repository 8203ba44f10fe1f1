"""CPU: the mesh quality report through tm_mesh_quality_host (no GPU touched) -- struct layout and exports, analytic meshes whose
answers are known by construction, an independent numpy restatement of the definitions of include/tm_hip.h on the parity topologies
and the two example meshes (seed, smoothed as written, Laplace-smoothed), and the facts those meshes pin: the TFI seeds are folded,
the example run unfolds all but one cell of T106, Laplace smoothing folds the O-grid blocks through the blade."""
import ctypes
import functools
import math

import numpy as np
import pytest

from oracle import oracle
from tests import meshes
from tests.conftest import OracleMesh, oracle_tfi
from tests.test_o4h import load
from turbomesh_amd import _capi, configs, quality
from turbomesh_amd.discrete import Mesh

REAL_FIELDS = ["min_scaled_jacobian", "min_angle_deg", "max_angle_deg", "max_aspect", "max_growth_i", "max_growth_j", "min_area", "max_area", "total_area"]


def mesh_of(*arrays):
    m = Mesh()
    for k, a in enumerate(arrays):
        m.addBlock(f"b{k}", configs.block_from_array(np.ascontiguousarray(a, dtype=np.float64).copy()))
    return m


def host(*arrays):
    return quality.mesh(mesh_of(*arrays), host=True)


# ------------------------------------------------------------------ the definitions restated in numpy (not shared with the product)
def np_quality(xy):
    """Section "mesh quality" of include/tm_hip.h for one (ni, nj, 2) block: dict of the record's fields + the per-cell minimum m,
    the degenerate mask and the number of valid cells within 1e-9 of a histogram edge."""
    x, y = xy[..., 0], xy[..., 1]
    A, B, C, D = (slice(None, -1), slice(None, -1)), (slice(1, None), slice(None, -1)), (slice(1, None), slice(1, None)), (slice(None, -1), slice(1, None))
    Js, Ps, Ss, Cs = [], [], [], []
    with np.errstate(all="ignore"):
        for c, nx, pv in ((A, B, D), (B, C, A), (C, D, B), (D, A, C)):
            ux, uy, vx, vy = x[nx] - x[c], y[nx] - y[c], x[pv] - x[c], y[pv] - y[c]
            J = ux * vy - uy * vx
            P = (ux * ux + uy * uy) * (vx * vx + vy * vy)
            Js.append(J)
            Ps.append(P)
            Ss.append(J / np.sqrt(P))
            Cs.append(np.clip((ux * vx + uy * vy) / np.sqrt(P), -1.0, 1.0))
        J, P, S, Cc = np.array(Js), np.array(Ps), np.array(Ss), np.array(Cs)
        a = 0.5 * ((x[C] - x[A]) * (y[D] - y[B]) - (x[D] - x[B]) * (y[C] - y[A]))
        cells = a.size
        sa, sabs = a.sum(), np.abs(a).sum()
        o = 0 if abs(sa) <= cells * 2.0 ** -53 * sabs else (1 if sa > 0 else -1)
        oo = 1 if o == 0 else o
        deg = ((P == 0) | ~np.isfinite(P) | ~np.isfinite(J)).any(axis=0)
        inverted = ~deg & ((oo * J).min(axis=0) <= 0)
        valid = ~deg & ~inverted
        m = (oo * S).min(axis=0)
        r = {"cells": cells, "orientation": o, "inverted": int(inverted.sum()), "degenerate": int(deg.sum())}
        nd = ~deg
        edges = np.arange(1, 10) / 10.0
        r["hist"] = tuple(int(v) for v in np.bincount(np.searchsorted(edges, m[valid], side="right"), minlength=10))
        near = int((np.abs(m[valid][:, None] - edges[None, :]).min(axis=1) < 1e-9).sum()) if valid.any() else 0
        if nd.any():
            r["min_scaled_jacobian"] = float(m[nd].min())
            r["min_angle_deg"] = float(np.degrees(np.arccos(Cc[:, nd].max())))
            r["max_angle_deg"] = float(np.degrees(np.arccos(Cc[:, nd].min())))
            r["min_area"], r["max_area"] = float((oo * a)[nd].min()), float((oo * a)[nd].max())
        r["total_area"] = float(oo * sa)
        Li = np.sqrt((x[1:] - x[:-1]) ** 2 + (y[1:] - y[:-1]) ** 2)            # (ni-1, nj): edges along i
        Lj = np.sqrt((x[:, 1:] - x[:, :-1]) ** 2 + (y[:, 1:] - y[:, :-1]) ** 2)   # (ni, nj-1): edges along j
        li, lj = Li[:, :-1] + Li[:, 1:], Lj[:-1] + Lj[1:]
        if nd.any():
            r["max_aspect"] = float((np.maximum(li, lj) / np.minimum(li, lj))[nd].max())

        def growth(l0, l1):
            ok = (l0 != 0) & (l1 != 0)
            return float((np.maximum(l0, l1)[ok] / np.minimum(l0, l1)[ok]).max()) if ok.any() else 1.0

        r["max_growth_i"], r["max_growth_j"] = growth(Li[:-1], Li[1:]), growth(Lj[:, :-1], Lj[:, 1:])
    return r, m, deg, near, float(sabs)


def close(a, b, rel=1e-12):
    return a == b or abs(a - b) <= rel * max(abs(a), abs(b))


def check_against_numpy(q, xy, label):
    r, m, deg, near, _ = np_quality(xy)
    for k in ("cells", "orientation", "inverted", "degenerate"):
        assert getattr(q, k) == r[k], (label, k, getattr(q, k), r[k])
    for k in REAL_FIELDS:
        if k in r:
            assert close(getattr(q, k), r[k]), (label, k, getattr(q, k), r[k])
    if "min_scaled_jacobian" in r:   # the reported worst cell holds numpy's minimum (positions may tie)
        assert not deg[q.worst_i, q.worst_j]
        assert abs(m[q.worst_i, q.worst_j] - r["min_scaled_jacobian"]) <= 1e-12, (label, q.worst_i, q.worst_j)
    assert sum(q.hist) == q.cells - q.inverted - q.degenerate
    assert max(abs(h0 - h1) for h0, h1 in zip(q.hist, r["hist"])) <= near, (label, q.hist, r["hist"], near)   # only a cell on a bin edge may land differently
    return r, near


# ------------------------------------------------------------------ struct and exports
def test_struct_size_and_exports():
    assert ctypes.sizeof(_capi.tm_quality) == 208
    lib = _capi.lib()
    for name in ("tm_mesh_quality", "tm_mesh_quality_host", "tm_smoother_quality", "tm_smoother_quality_field"):
        assert hasattr(lib, name) and name in _capi.EXPORTS
    off = {f[0]: getattr(_capi.tm_quality, f[0]).offset for f in _capi.tm_quality._fields_}
    assert off["orientation"] == 24 and off["min_scaled_jacobian"] == 32 and off["worst_block"] == 40 and off["min_angle_deg"] == 64
    assert off["max_aspect"] == 80 and off["min_area"] == 104 and off["hist"] == 128


# ------------------------------------------------------------------ analytic meshes
H, K, NI, NJ = 0.5, 0.125, 7, 9


def cartesian():
    i, j = np.meshgrid(np.arange(NI), np.arange(NJ), indexing="ij")
    return np.stack([H * i, K * j], axis=-1).astype(np.float64)


def sheared():
    g = cartesian()
    g[..., 0] = g[..., 0] + g[..., 1] * math.tan(math.radians(30.0))
    return g


def test_uniform_cartesian_grid():
    per, total = host(cartesian())
    q = per[0]
    cells = (NI - 1) * (NJ - 1)
    assert q.cells == cells and q.inverted == 0 and q.degenerate == 0 and q.orientation == 1
    assert q.hist == (0,) * 9 + (cells,)
    assert q.min_scaled_jacobian == 1.0 and (q.worst_block, q.worst_i, q.worst_j) == (0, 0, 0)
    assert q.max_aspect == 4.0 and q.max_growth_i == 1.0 and q.max_growth_j == 1.0
    assert abs(q.min_angle_deg - 90.0) <= 1e-13 and abs(q.max_angle_deg - 90.0) <= 1e-13
    assert q.total_area == cells * H * K and q.min_area == H * K and q.max_area == H * K
    assert total == q   # one block: the total is the block


def test_sheared_grid():
    q = host(sheared())[0][0]
    assert q.inverted == 0 and q.degenerate == 0 and q.orientation == 1
    assert abs(q.min_scaled_jacobian - math.cos(math.radians(30.0))) <= 1e-13
    assert abs(q.min_angle_deg - 60.0) <= 1e-11 and abs(q.max_angle_deg - 120.0) <= 1e-11
    assert q.hist[8] == q.cells and abs(q.total_area - q.cells * H * K) <= 1e-13
    check_against_numpy(q, sheared(), "sheared")


def test_i_reversed_block_is_left_handed():
    a, b = host(cartesian())[0][0], host(cartesian()[::-1])[0][0]
    assert b.orientation == -1 and a.orientation == 1
    b.orientation = 1
    assert a == b   # every other field, bit for bit
    s, r = host(sheared())[0][0], host(sheared()[::-1])[0][0]
    assert r.orientation == -1 and r.inverted == 0 and r.hist == s.hist   # the worst cell is decided by the last bit here: not compared
    for k in REAL_FIELDS:
        assert close(getattr(s, k), getattr(r, k), 1e-13), k
    # a mesh of a right- and a left-handed block: each block by its own orientation, the total says they differ
    per, total = host(cartesian(), cartesian()[::-1])
    assert [p.orientation for p in per] == [1, -1] and total.orientation == 0
    assert total.inverted == 0 and total.cells == 2 * a.cells and total.total_area == 2 * a.total_area and total.hist[9] == total.cells


def test_one_node_moved_across_its_neighbour():
    g = cartesian()
    g[3, 4, 0] += 1.5 * H   # node (3,4) now lies beyond node (4,4): cells (3,3) and (3,4) fold, (2,3) and (2,4) stretch
    q = host(g)[0][0]
    assert q.cells == 48 and q.inverted == 2 and q.degenerate == 0 and q.orientation == 1
    # both folded cells have a corner with s = -1 exactly (edges anti-parallel to the frame): the tie goes to the lower cell
    assert q.min_scaled_jacobian == -1.0 and (q.worst_block, q.worst_i, q.worst_j) == (0, 3, 3)
    # the stretched cells: min s = 0.0625 / (0.5 * sqrt(0.578125)) = 0.164 -> bin 1; the other 44 are squares
    assert q.hist == (0, 2, 0, 0, 0, 0, 0, 0, 0, 44)
    check_against_numpy(q, g, "folded")
    # the same in a left-handed block: still two inverted cells, found through max J >= 0
    ql = host(g[::-1])[0][0]
    assert ql.orientation == -1 and ql.inverted == 2 and ql.min_scaled_jacobian == -1.0 and ql.hist == q.hist
    assert (ql.worst_i, ql.worst_j) == (2, 3)   # cells (3,3), (3,4) are cells (2,3), (2,4) of the reversed block


def test_two_coincident_nodes():
    g = cartesian()
    g[3, 4] = g[4, 4]   # the edge (3,4)-(4,4) has length 0: the two cells on it are degenerate
    q = host(g)[0][0]
    assert q.degenerate == 2 and q.inverted == 0 and sum(q.hist) == 46
    r, m, deg, _, _ = np_quality(g)
    assert sorted(zip(*np.nonzero(deg))) == [(3, 3), (3, 4)]
    for k in REAL_FIELDS:   # extremes over the other 46 cells only: all finite, equal to the restatement's
        assert math.isfinite(getattr(q, k)) and close(getattr(q, k), r[k]), k
    assert q.min_scaled_jacobian > 0 and q.max_angle_deg < 180.0 and q.max_aspect < 10.0
    # every cell degenerate: no extreme exists
    z = host(np.zeros((3, 4, 2)))[0][0]
    assert z.degenerate == z.cells == 6 and z.inverted == 0 and sum(z.hist) == 0 and z.orientation == 0
    assert math.isnan(z.min_scaled_jacobian) and (z.worst_block, z.worst_i, z.worst_j) == (0, 0, 0)
    assert z.max_growth_i == 1.0 and z.max_growth_j == 1.0


def test_single_cell_block():
    q = host(np.array([[[0.0, 0.0], [0.0, 1.0]], [[2.0, 0.0], [2.0, 1.0]]]))[0][0]
    assert q.cells == 1 and q.hist[9] == 1 and q.max_growth_i == 1.0 and q.max_growth_j == 1.0
    assert q.max_aspect == 2.0 and q.total_area == 2.0 and q.min_scaled_jacobian == 1.0


def test_growth_is_measured_along_grid_lines():
    i, j = np.meshgrid(np.arange(5), np.arange(4), indexing="ij")
    g = np.stack([1.5 ** i, 0.25 * 2.0 ** j], axis=-1)   # geometric spacing: ratio 1.5 along i, 2 along j
    q = host(g)[0][0]
    assert q.max_growth_i == 1.5 and q.max_growth_j == 2.0 and q.inverted == 0


def test_block_with_one_node_row_is_a_size_error():
    with pytest.raises(_capi.TmError) as e:
        host(np.zeros((1, 5, 2)))
    assert e.value.code == _capi.TM_E_SIZE
    with pytest.raises(_capi.TmError) as e:
        host(cartesian(), np.zeros((4, 1, 2)))
    assert e.value.code == _capi.TM_E_SIZE


# ------------------------------------------------------------------ numpy restatement on the parity topologies and the examples
@pytest.mark.parametrize("name", sorted(meshes.TOPOLOGIES))
def test_topologies_against_numpy(name):
    mesh = meshes.TOPOLOGIES[name](oracle_tfi)
    per, total = mesh.quality(host=True)
    for b, q in enumerate(per):
        check_against_numpy(q, mesh.blocks[b].points.data, f"{name}[{b}]")
    assert total.cells == sum(q.cells for q in per) and total.inverted == sum(q.inverted for q in per)


@functools.lru_cache(maxsize=None)
def example(name, stage):
    """Block coordinates of an example mesh: 'seed' (TFI), 'written' (the JSON as written on the oracle: 10 iterations, GMRES + ILU(0),
    White), 'laplace' (2 exact Picard iterations, Laplace control function)."""
    inp, mesh = load(name, oracle_tfi)
    if stage == "seed":
        return [b.points.data.copy() for b in mesh.blocks]
    om = OracleMesh(mesh)
    if stage == "written":
        w = inp.wall_control_function.white
        st = oracle.smooth_mesh(om, inp.iterations, solver=oracle.SOLVER_GMRES, preconditioner=oracle.PRECOND_ILU0, control=("white", w.ds_target, w.theta_target))
        assert st.outer_iterations == 10 and st.not_converged == 0
    else:
        oracle.picard_exact(om, 2)
    return [np.ascontiguousarray(b) for b in om.blocks]


@pytest.mark.parametrize("name", ["T106", "LS89"])
@pytest.mark.parametrize("stage", ["seed", "written", "laplace"])
def test_examples_against_numpy(name, stage):
    blocks = example(name, stage)
    per, total = host(*blocks)
    for b, q in enumerate(per):
        check_against_numpy(q, blocks[b], f"{name}/{stage}[{b}]")
    assert total.inverted == sum(q.inverted for q in per) and total.degenerate == 0
    worst = min(per, key=lambda q: q.min_scaled_jacobian)
    assert total.min_scaled_jacobian == worst.min_scaled_jacobian and total.worst_block == worst.worst_block


# ------------------------------------------------------------------ pinned facts
def test_tfi_seeds_are_folded():
    assert [q.inverted for q in host(*example("T106", "seed"))[0]] == [0, 0, 0, 3, 0, 50, 0, 0]
    assert [q.inverted for q in host(*example("LS89", "seed"))[0]] == [0, 0, 0, 0, 0, 588, 0, 42]


def test_t106_blocks_differ_in_handedness():
    assert [q.orientation for q in host(*example("T106", "seed"))[0]] == [-1 if b in (1, 4, 5) else 1 for b in range(8)]


def test_example_runs_as_written_unfold_all_but_one_cell():
    per, total = host(*example("T106", "written"))
    assert [q.inverted for q in per] == [1, 0, 0, 0, 0, 0, 0, 0]
    assert (total.worst_block, total.worst_i, total.worst_j) == (0, 213, 0)
    assert abs(total.min_scaled_jacobian - (-0.04822)) <= 1e-5
    per, total = host(*example("LS89", "written"))
    assert [q.inverted for q in per] == [0] * 8 and total.ok


@pytest.mark.parametrize("name", ["T106", "LS89"])
def test_laplace_smoothing_folds_the_o_grid_blocks(name):
    blocks = example(name, "laplace")
    per, _ = host(*blocks)
    assert per[0].inverted > 0 and per[1].inverted > 0
    assert [q.inverted for q in per] == [np_quality(b)[0]["inverted"] for b in blocks]
