"""CPU: the run tables of the perimeter-row launches and the strip plan of the fused level kernel (turbomesh_amd/csrc/tm_edge_tables.cpp,
read through tm_edge_tables_probe) against the plan they compress: tm_plan_build's global row table and tm_plan_local's rank-local
numbering.  Every run and every row is checked, nothing is sampled.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from tests.conftest import oracle_tfi
from tests.meshes import TOPOLOGIES
from turbomesh_amd import _capi, configs, distributed
from turbomesh_amd.smoothing import smooth

ALL, NF, NF_GHOST, LEVEL1, LEVEL2, LEVEL3 = range(6)
KIND_FIXED, KIND_SMOOTHED, KIND_INTERIOR = 0, 1, 5
EDGE_BLOCK = 128            # rows of a run per workgroup (tm_edge_types.h)
METRIC_SLOTS = (2, 1, 4, 3)   # im1_j, ip1_j, i_jm1, i_jp1 in the slot numbering of smooth.zig:175-185 (PlanRow::metric, tm_plan.hpp)


def probe(mesh, owner, rank, world, table, level_strip=0):
    md = _capi.MeshDesc(mesh, with_coordinates=False)
    info = _capi.tm_edge_tables_info()
    own = (C.c_int32 * len(owner))(*owner)
    _capi.check(_capi.lib().tm_edge_tables_probe(md.ref(), own, rank, world, table, level_strip, C.byref(info)))
    try:
        def arr(name, n, width=1):
            a = np.ctypeslib.as_array(getattr(info, name), (max(n * width, 1),))[:n * width].astype(np.int64)
            return a.reshape(n, width) if width > 1 else a

        nr, ns, nt = int(info.nruns), int(info.nstrips), int(info.ntasks)
        T = {k: arr(k, nr) for k in ("first", "count", "row0", "row_stride", "kind", "ncols", "self", "flags")}
        T.update({k: arr(k, nr, 9) for k in ("col0", "col_stride")})
        T.update({k: arr(k, nr, 4) for k in ("met0", "met_stride")})
        T.update(nrows=int(info.nrows), nruns=nr, wg_run=arr("wg_run", int(info.nwg)), wg_k0=arr("wg_k0", int(info.nwg)), gid=arr("gid", int(info.nrows)),
                 nstrips=ns, strip_off=arr("strip_off", ns, 4) if ns else np.zeros((0, 4), np.int64), task=arr("task", nt, 4) if nt else np.zeros((0, 4), np.int64))
        return T
    finally:
        _capi.lib().tm_edge_tables_free(C.byref(info))


class Plan:
    """What the tables compress, in numpy: the global row table (tm_plan_build) and one rank's numbering (tm_plan_local)."""

    def __init__(self, mesh, owner, rank, world):
        self.rows = smooth.plan_rows(mesh)
        self.at = {int(g): k for k, g in enumerate(self.rows["row"])}
        self.lp = lp = distributed.local_plan(mesh, owner, rank, world)
        self.shape = [tuple(int(v) for v in b.points.size) for b in mesh.blocks]
        self.start = np.concatenate([[0], np.cumsum([ni * nj for ni, nj in self.shape])])
        self.n_owned = lp["n_owned"]
        self.local = np.full(self.start[-1], -1, dtype=np.int64)   # gid -> local id
        for b, ls in zip(lp["owned_blocks"], lp["local_start"]):
            self.local[self.start[b]:self.start[b + 1]] = ls + np.arange(self.start[b + 1] - self.start[b])
        self.local[lp["ghost_gid"]] = self.n_owned + np.arange(len(lp["ghost_gid"]))
        self.owned_perimeter = [int(g) for g in self.rows["row"] if self.local[g] >= 0 and self.local[g] < self.n_owned]

    def block_ij(self, gid):
        b = int(np.searchsorted(self.start, gid, side="right")) - 1
        return (b,) + divmod(int(gid - self.start[b]), self.shape[b][1])

    def moving(self):
        return [g for g in self.owned_perimeter if self.rows["kind"][self.at[g]] != KIND_FIXED]

    def zone(self, lev):
        """Interior nodes within 4 - lev of a side whose perimeter rows move; a corner node counts for its row i = const only."""
        sides = {int(b): set() for b in self.lp["owned_blocks"]}
        for g in self.moving():
            b, i, j = self.block_ij(g)
            ni, nj = self.shape[b]
            corner_row = i in (0, ni - 1)
            sides[b] |= {s for s, on in ((0, i == 0), (1, i == ni - 1), (2, j == 0 and not corner_row), (3, j == nj - 1 and not corner_row)) if on}
        out, d = [], 4 - lev
        for b, on in sides.items():
            ni, nj = self.shape[b]
            i, j = np.meshgrid(np.arange(1, ni - 1), np.arange(1, nj - 1), indexing="ij")
            inside = ((0 in on) & (i <= d)) | ((1 in on) & (i >= ni - 1 - d)) | ((2 in on) & (j <= d)) | ((3 in on) & (j >= nj - 1 - d))
            out += [int(g) for g in (self.start[b] + i * nj + j)[inside]]
        return out

    def selection(self, table):
        """The gids a table has to hold; for level 1 the remote part is only known to lie in the ghost set (tm_plan_local does not list
        the depth-2 definitions), so it is returned as None and checked as a subset."""
        if table == ALL:
            return self.owned_perimeter, []
        own = self.moving() + (self.zone(table - LEVEL1) if table >= LEVEL1 else [])
        if table in (NF_GHOST, LEVEL2):
            return own, [int(g) for g in self.lp["ghost_row_gid"]]
        return own, (None if table == LEVEL1 else [])


def expand(T):
    """Per run: positions, local row ids, local column ids [count, 9], metric neighbours [count, 4]."""
    out = []
    for r in range(T["nruns"]):
        k = np.arange(T["count"][r])
        out.append((T["first"][r] + k, T["row0"][r] + k * T["row_stride"][r], T["col0"][r] + k[:, None] * T["col_stride"][r],
                    T["met0"][r] + k[:, None] * T["met_stride"][r]))
    return out


def check_table(P, T, table):
    n, rows = T["nrows"], P.rows
    # 1. tiling, permutation of the selection
    assert T["nruns"] == 0 or T["first"][0] == 0
    assert np.array_equal(T["first"][1:], (T["first"] + T["count"])[:-1]) and int(T["count"].sum()) == n and np.all(T["count"] >= 1)
    own, remote = P.selection(table)
    got = sorted(int(g) for g in T["gid"])
    assert len(set(got)) == n
    mine = [g for g in got if P.local[g] < P.n_owned]
    assert mine == sorted(own)
    theirs = [g for g in got if P.local[g] >= P.n_owned]
    if remote is None:   # the depth-2 set holds the depth-1 rows
        assert set(int(g) for g in P.lp["ghost_row_gid"]) <= set(theirs)
    else:
        assert theirs == sorted(remote)
    # 2. expansion and 3. static fields, row by row
    for r, (pos, row, col, met) in enumerate(expand(T)):
        gids = T["gid"][pos]
        assert np.array_equal(row, P.local[gids]), r
        kind, ncols = int(T["kind"][r]), int(T["ncols"][r])
        ghost = row >= P.n_owned
        assert np.all(ghost == ghost[0])
        if kind == KIND_INTERIOR:
            assert ncols == 9 and T["self"][r] == 4
            for k, g in enumerate(gids):
                b, i, j = P.block_ij(g)
                ni, nj = P.shape[b]
                assert 1 <= i <= ni - 2 and 1 <= j <= nj - 2 and int(g) not in P.at
                want = [g + di * nj + dj for di in (-1, 0, 1) for dj in (-1, 0, 1)]
                assert np.array_equal(col[k], P.local[want]), (r, k)
            assert (int(T["flags"][r]) & 0x1C) == (0 if ghost[0] else 16)
            continue
        at = np.array([P.at[int(g)] for g in gids])
        k0 = at[0]
        assert np.all(rows["kind"][at] == kind) and np.all(rows["ncols"][at] == ncols)
        assert np.all(rows["slot"][at] == rows["slot"][k0])
        assert all(np.array_equal(rows[c][a], rows[c][k0], equal_nan=True) for a in at for c in ("coef_x", "coef_y"))
        cols = rows["cols"][at, :ncols]
        assert np.array_equal(col[:, :ncols], P.local[cols]), r
        assert np.all(cols[:, T["self"][r]] == gids)
        if kind == KIND_SMOOTHED:
            for q, slot in enumerate(METRIC_SLOTS):
                where = np.argmax(rows["slot"][at] == slot, axis=1)
                assert np.all(rows["slot"][at, where] == slot)
                assert np.array_equal(met[:, q], P.local[rows["cols"][at, where]]), (r, q)
        # bits 2 / 3: the right-hand side of a ghost copy comes from the row's value where the plan takes it from the coordinates
        from_coords = np.isnan(rows["rhs"][at])
        assert np.all(from_coords == from_coords[0])
        want = (4 if from_coords[0, 0] else 0) | (8 if from_coords[0, 1] else 0) if ghost[0] else 0
        assert (int(T["flags"][r]) & 0x1C) == want, r
    # 4. one workgroup per EDGE_BLOCK rows of a run
    want = [(r, k0) for r in range(T["nruns"]) for k0 in range(0, int(T["count"][r]), EDGE_BLOCK)]
    assert list(zip(T["wg_run"].tolist(), T["wg_k0"].tolist())) == want
    assert len(want) == int(np.sum(-(-T["count"] // EDGE_BLOCK)))


def reads_of(T, n_local):
    """Per position in run order: the local ids its row reads at the previous level (columns, metric neighbours if smoothed, itself)."""
    out = [None] * T["nrows"]
    made = np.full(n_local, -1, dtype=np.int64)   # local id -> position
    for r, (pos, row, col, met) in enumerate(expand(T)):
        ids = np.concatenate([col[:, :T["ncols"][r]], met if T["kind"][r] == KIND_SMOOTHED else met[:, :0], row[:, None]], axis=1)
        for p, i in zip(pos, ids):
            out[p] = i
        made[row] = pos
    return out, made


def check_strips(P, tables):
    """5. every level-3 row in exactly one strip; per strip, what its rows read and the level below produces is inside its tasks there."""
    T3 = tables[2]
    n_local = P.n_owned + len(P.lp["ghost_gid"])
    reads, made = zip(*(reads_of(T, n_local) for T in tables))
    off, task = T3["strip_off"], T3["task"]
    assert T3["nstrips"] > 0 and off[0, 0] == 0 and off[-1, 3] == len(task)
    assert np.array_equal(off[1:, 0], off[:-1, 3]) and np.all(np.diff(off, axis=1) >= 0)
    owners = np.zeros(T3["nrows"], dtype=np.int64)
    for s in range(T3["nstrips"]):
        have = []
        for lev in range(3):
            T, cover = tables[lev], np.zeros(tables[lev]["nrows"], dtype=bool)
            for level, run, k0, count in task[off[s, lev]:off[s, lev + 1]]:
                assert level == lev + 1 and 1 <= count <= 64 and 0 <= k0 and k0 + count <= T["count"][run], (s, lev)
                cover[T["first"][run] + k0:T["first"][run] + k0 + count] = True
            have.append(cover)
        owners += have[2]
        for lev in (2, 1):
            for p in np.flatnonzero(have[lev]):
                below = made[lev - 1][reads[lev][p]]
                assert np.all(have[lev - 1][below[below >= 0]]), (s, lev, p)
    assert np.all(owners == 1)


def single(mesh):
    return [0] * len(mesh.blocks), 0, 1


@pytest.mark.parametrize("table", [ALL, NF])
@pytest.mark.parametrize("name", list(TOPOLOGIES))
def test_tables_of_the_topologies(name, table):
    mesh = TOPOLOGIES[name](oracle_tfi)
    P = Plan(mesh, *single(mesh))
    check_table(P, probe(mesh, *single(mesh), table), table)


@pytest.fixture
def triples_on_small_blocks(monkeypatch):
    monkeypatch.setenv("TM_TRIPLES_MIN_NODES", "1")   # the depth-3 halo for every block of at least 16 x 16 nodes (triple_halo_for)


@pytest.mark.parametrize("owner", [[0, 0, 1, 1], [0, 1, 0, 1]])
@pytest.mark.parametrize("rank", [0, 1])
def test_tables_of_two_ranks(owner, rank, triples_on_small_blocks):
    mesh = configs.strip(4, 17, 21, tfi=oracle_tfi)
    P = Plan(mesh, owner, rank, 2)
    assert len(P.lp["ghost_row_gid"]) > 0
    tables = [probe(mesh, owner, rank, 2, table, level_strip=8) for table in range(6)]
    for table, T in enumerate(tables):
        check_table(P, T, table)
    assert any(P.local[g] >= P.n_owned for g in tables[LEVEL1]["gid"])   # the depth-2 ghost rows are there
    check_strips(P, tables[LEVEL1:])


LEVEL_MESHES = {
    "strip2_reversed": lambda: configs.strip(2, 17, 21, tfi=oracle_tfi, reverse_odd=True),
    "two_by_two": lambda: configs.two_by_two(17, 19, tfi=oracle_tfi),
    "periodic_channel": lambda: configs.periodic_channel(21, 15, tfi=oracle_tfi),
}


@pytest.mark.parametrize("name", list(LEVEL_MESHES))
def test_level_tables_and_strip_closure(name):
    mesh = LEVEL_MESHES[name]()
    P = Plan(mesh, *single(mesh))
    tables = [probe(mesh, *single(mesh), table, level_strip=8) for table in (LEVEL1, LEVEL2, LEVEL3)]
    for table, T in zip((LEVEL1, LEVEL2, LEVEL3), tables):
        check_table(P, T, table)
    check_strips(P, tables)


def test_strip_closure_with_the_default_strip_length():
    mesh = configs.strip(2, 40, 130, tfi=oracle_tfi)
    P = Plan(mesh, *single(mesh))
    tables = [probe(mesh, *single(mesh), table) for table in (LEVEL1, LEVEL2, LEVEL3)]
    for table, T in zip((LEVEL1, LEVEL2, LEVEL3), tables):
        check_table(P, T, table)
    check_strips(P, tables)
    # 130 positions along the interface rows, 60 per strip: three strips per side of the interface at least
    assert tables[2]["nstrips"] >= 6
