"""K2 and the Krylov kernels at every chunk height, on small blocks.

The interior operator (apply_tile, csrc/tm_kernels.hip) runs with chunks of RI rows and row groups of U rows.  A small mesh fits 512 workgroups
at RI = 3, so the bit-exact small-shape tests (test_gpu_operator, test_gpu_smooth, test_gpu_edgecases) all run RI = 3, U = 3; every mesh above
about 0.4 M nodes runs U = 6 with chunks of 6 .. 36 rows.  Here that configuration is reached on blocks of a few thousand nodes, by
TM_APPLY_ROWS=h (read when a handle is created, tools/README.md) and by tall thin blocks which the library's own rules hand tall chunks:

1. the operator (MODE_RAW, MODE_SCALED, vector and field window, with and without (P,Q)) bit for bit against the oracle's mirror of the device
   arithmetic, the reference-order CSR on the perimeter, and the same handle at 3 rows;
2. single relaxation sweeps bit for bit against the oracle's sweeps, their displacement sums against the 3-row run;
3. the dot-product launches of k_apply (profiling on: no merged launch) under GMRES(30) and the classic BiCGStab recurrence;
4. the two kernels of the two-kernel BiCGStab iteration (k_apply_vk<VK_R>, <VK_S2>) at heights 6 .. 36 in both layouts, the spilling VK_R
   variant, and chunks taller than the blocks of a multi-block mesh;
5. the heights the library chooses by itself.

The bar of the capped Krylov runs (parts 3 to 5) is max-abs 1e-11 -- the bar of test_two_kernel_iteration_odd_shapes for the same protocol,
eager against lazy.  Per-node arithmetic is the same at every height (-ffp-contract=off); only the grouping of the partial sums changes with
the tiles.  A node stored twice or not at all at a chunk seam, or a partial sum that misses a row, moves nodes by the size of the update
itself, which these tests require to be at least 1e-6: five orders between "rounding" and "wrong".  (Measured distances: 2e-16 .. 5e-15.
A single wrong last bit in one row is below any such bar; only the bit-exact parts 1, 2 and 5 see that.)

With TM_CHUNK_PARITY_OUT=<file> every measured distance is appended to that file as "part case height layout distance"
(profiles/chunk_height_parity.txt)."""
import os

import numpy as np
import pytest

from oracle import oracle
from tests import test_gpu_gmres as gm
from tests import test_gpu_operator as op
from tests.conftest import OracleMesh, mesh_flat, oracle_tfi
from turbomesh_amd import configs
from turbomesh_amd.smoothing import smooth, solver, wall_control_function as wcf

pytestmark = pytest.mark.gpu
BAR = 1e-11          # max-abs distance of two capped runs whose partial sums are grouped differently
MIN_UPDATE = 1e-6    # ... on meshes which those runs move by at least this much

# (height, interior rows, nj).  Interior rows per height h: 6, h, h + 1, 2 h, 2 h + 5, and 4 (clamped below 6: the three-row group).
# nj: 3 / 9 a single partial wave; 64 / 65 one wave and one column more; 128 two waves; 129 the first width at which wave 1 owns 64 columns
# and takes the unpredicated loop; 130; 257 / 258 a second workgroup column that owns 0 / 1 columns.
OPERATOR_CASES = [
    (6, 6, 3), (6, 7, 129), (6, 12, 64), (6, 17, 257), (6, 4, 65),
    (7, 6, 9), (7, 7, 130), (7, 8, 258), (7, 14, 65), (7, 19, 128),
    (12, 6, 128), (12, 12, 257), (12, 13, 3), (12, 24, 130), (12, 29, 64),
    (18, 6, 258), (18, 18, 9), (18, 19, 64), (18, 36, 129), (18, 41, 65),
    (24, 24, 65), (24, 25, 128), (24, 48, 9), (24, 53, 258),
    (36, 36, 129), (36, 37, 257), (36, 72, 3), (36, 77, 130), (36, 4, 9),
]
# the same rule with the widths around the edges of the overlapping strips: 62 / 124 / 248 owned columns
VK_CASES = [
    (6, 6, 9), (6, 7, 126), (6, 12, 250), (6, 17, 65), (6, 4, 64),
    (7, 6, 127), (7, 7, 251), (7, 8, 64), (7, 14, 9), (7, 19, 250),
    (18, 6, 251), (18, 18, 65), (18, 19, 127), (18, 36, 126), (18, 41, 64),
    (36, 36, 250), (36, 37, 9), (36, 72, 127), (36, 77, 251), (36, 6, 65), (36, 4, 126),
]


def _ids(cases):
    return [f"h{h}-{rows + 2}x{nj}" for h, rows, nj in cases]


def _set(monkeypatch, **env):
    """TM_* variables for the next handle; None removes one."""
    for k, v in env.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))


def _report(part, case, height, layout, dist):
    line = f"{part:10s} {case:22s} rows {str(height):>7s}  {layout:14s} {dist:.3e}"
    print(line)
    if os.environ.get("TM_CHUNK_PARITY_OUT"):
        with open(os.environ["TM_CHUNK_PARITY_OUT"], "a") as fh:
            fh.write(line + "\n")


# ------------------------------------------------------------------ 1. the operator
def _operator_outputs(ni, nj, vec, field):
    """(A vec, D^-1 A vec, A x, row kinds) of a handle created under the current environment; field: a prescribed (P,Q) or None."""
    mesh = configs.single_block(ni, nj, perturb=0.2)
    algo = None if field is None else wcf.Algorithm.prescribed([field])
    with smooth.Smoother(mesh, solver.Option.hip(), algo) as sm:
        if field is not None:
            assert np.array_equal(sm.control_function(), field.reshape(-1, 2))
        return sm.apply(vec, scaled=False), sm.apply(vec, scaled=True), sm.apply(mesh_flat(mesh), scaled=False), sm.row_kinds()


def _check_operator(h, rows, nj, with_pq, monkeypatch):
    ni = rows + 2
    mesh = configs.single_block(ni, nj, perturb=0.2)
    om = OracleMesh(mesh)
    vec = np.random.default_rng(7).standard_normal((ni * nj, 2))
    field = np.random.default_rng(11).uniform(-0.5, 0.5, (ni, nj, 2)) if with_pq else None
    pq = None if field is None else field.reshape(-1, 2)
    _set(monkeypatch, TM_APPLY_ROWS=h)
    raw, scaled, fx, kinds = _operator_outputs(ni, nj, vec, field)
    _set(monkeypatch, TM_APPLY_ROWS=3)
    raw3, scaled3, fx3, _ = _operator_outputs(ni, nj, vec, field)
    perim = kinds >= 0
    # perimeter rows of a lone block are `fixed` (identity rows, no (P,Q) in them): the reference-order CSR of the Laplace system
    ref, _, diag, _ = op._oracle_apply(om, vec)
    dinv = np.where(diag == 0.0, 1.0, 1.0 / diag)
    x = om.flat()
    ref_x, _, _, _ = op._oracle_apply(OracleMesh(mesh), x)
    tag = f"h={h} {ni}x{nj} pq={with_pq}"
    assert np.array_equal(raw[perim], ref[perim]), tag
    assert np.array_equal(scaled[perim], (ref * dinv)[perim]), tag
    assert np.array_equal(fx[perim], ref_x[perim]), tag
    # interior rows: the oracle's mirror of the device operation order
    for got, mode, v, what in ((raw, oracle.MIRROR_RAW, vec, "raw"), (scaled, oracle.MIRROR_SCALED, vec, "scaled"), (fx, oracle.MIRROR_RAW, x, "field")):
        mir = op._mirror(om, v, mode, pq)
        bad = np.flatnonzero((got[~perim] != mir[~perim]).any(axis=1))
        assert bad.size == 0, f"{tag} {what}: {bad.size} interior rows differ from the mirror, first at interior index {bad[:5]}"
        assert np.isfinite(got).all() and np.abs(got[~perim]).max() > 0
    # ... and the 3-row chunks of the same mesh: tells a disagreement with the mirror from a disagreement between heights
    assert np.array_equal(raw, raw3) and np.array_equal(scaled, scaled3) and np.array_equal(fx, fx3), tag


@pytest.mark.parametrize("h,rows,nj", OPERATOR_CASES, ids=_ids(OPERATOR_CASES))
def test_operator_rows_at_every_chunk_height(h, rows, nj, monkeypatch):
    _check_operator(h, rows, nj, False, monkeypatch)


@pytest.mark.parametrize("h,rows,nj", [(6, 17, 257), (7, 19, 128), (12, 29, 64), (18, 41, 65), (24, 53, 258), (36, 77, 130)])
def test_operator_rows_with_a_control_function_at_every_chunk_height(h, rows, nj, monkeypatch):
    _check_operator(h, rows, nj, True, monkeypatch)


# ------------------------------------------------------------------ 2. single relaxation sweeps
RELAX_CASES = [c for c in OPERATOR_CASES if c[0] in (6, 7, 18)]


def _relax(ni, nj, omega):
    mesh = configs.single_block(ni, nj, perturb=0.2)
    with smooth.Smoother(mesh, solver.Option.hip(inner=solver.Inner.relax, single_sweep=True, omega=omega)) as sm:
        st = sm.iterate(3)
        sm.download()
    return mesh.blocks[0].points.data.copy(), st


@pytest.mark.parametrize("omega", [1.0, 0.9])
@pytest.mark.parametrize("h,rows,nj", RELAX_CASES, ids=_ids(RELAX_CASES))
def test_single_sweeps_at_every_chunk_height(h, rows, nj, omega, monkeypatch):
    ni = rows + 2
    ref = configs.single_block(ni, nj, perturb=0.2).blocks[0].points.data.copy()
    seed = ref.copy()
    oracle.time_relax_sweeps(ref, 3, omega)
    _set(monkeypatch, TM_APPLY_ROWS=h)
    got, st = _relax(ni, nj, omega)
    _set(monkeypatch, TM_APPLY_ROWS=3)
    got3, st3 = _relax(ni, nj, omega)
    assert np.array_equal(got, ref), (h, ni, nj, omega, float(np.abs(got - ref).max()))
    assert np.array_equal(got3, ref)
    assert not np.array_equal(got[1:-1, 1:-1], seed[1:-1, 1:-1])
    # the displacement sums of the last sweep: the same terms, grouped by other tiles (the bar of test_gpu_fused for a regrouped deterministic sum)
    assert st["operator_sweeps"] == 3 == st3["operator_sweeps"]
    assert st["last_dx2"] == pytest.approx(st3["last_dx2"], rel=1e-11, abs=1e-300)
    assert st["last_dy2"] == pytest.approx(st3["last_dy2"], rel=1e-11, abs=1e-300)


# ------------------------------------------------------------------ capped Krylov runs (parts 3 to 5)
def _capped(ni, nj, profile=False, **opt):
    """Two Picard iterations of five inner iterations each under the current environment -> (coordinates, stats)."""
    mesh = configs.single_block(ni, nj, perturb=0.2)
    with smooth.Smoother(mesh, solver.Option.hip(rtol=1e-30, max_inner=5, check_every=5, **opt)) as sm:
        if profile:
            sm.profile(1)
        st = sm.iterate(2)
        sm.download()
    return mesh.blocks[0].points.data.copy(), st


def _check_capped(part, ni, nj, height, layout, got, st, ref):
    seed = configs.single_block(ni, nj, perturb=0.2).blocks[0].points.data
    dist = float(np.abs(got - ref).max())
    _report(part, f"{ni}x{nj}", height, layout, dist)
    assert np.isfinite(got).all()
    assert st["inner_iterations"] == 10, st
    for a, b in ((got[0], seed[0]), (got[-1], seed[-1]), (got[:, 0], seed[:, 0]), (got[:, -1], seed[:, -1])):
        assert np.array_equal(a, b)   # the fixed boundary, to the bit
    update = float(np.abs(got[1:-1, 1:-1] - seed[1:-1, 1:-1]).max())
    assert update >= MIN_UPDATE, (ni, nj, update)   # a seam defect is of the size of the update: >= 1e5 bars
    assert dist <= BAR, (part, ni, nj, height, layout, dist)


# ------------------------------------------------------------------ 3. the dot-product launches of k_apply
def test_gmres_recurrence_through_unmerged_launches_at_18_rows(monkeypatch):
    # profiling on: no merged interior + perimeter launch, so the residual (MODE_RESID, DOT_OUT2) goes through launch_apply_block like the
    # Arnoldi applies -- the route of every mesh of more than 1024 workgroups; 41 = 2 x 18 + 5 interior rows.  The bar is the one of
    # test_gpu_gmres (1e-9 between two GMRES runs stopped at the same tolerance); 65 columns keep it meaningful for this taller block: the
    # CPU recurrence itself lands 2.0e-10 from the exact solution of this system (8e-11 .. 1e-10 for that test's 41 x 37 block), so two
    # such runs are at most 4e-10 apart, while at 130 columns it is 5.8e-10 from it and the bar could fail on conditioning alone.
    _set(monkeypatch, TM_APPLY_ROWS=18)
    gm.frozen_system_against_the_cpu_gmres(43, 65, prepare=lambda sm: sm.profile(1))


@pytest.mark.parametrize("nj", [65, 130])
def test_classic_bicgstab_through_unmerged_launches_at_18_rows(nj, monkeypatch):
    # TM_FUSE_2=0 + eager scalars: the classic recurrence, whose applies carry DOT_AUX / DOT_IN / DOT_OUT2.  18-row chunks and profiling on
    # (k_apply<.., U = 6>, one launch for the interior and one for the perimeter rows) against 3-row chunks in the merged launch.
    # 130 columns: wave 1 takes the unpredicated loop with the dot products in it.
    _set(monkeypatch, TM_FUSE_2=0, TM_VK_OVERLAP=None, TM_APPLY_ROWS=3)
    ref, _ = _capped(43, nj, eager_scalars=True)
    _set(monkeypatch, TM_APPLY_ROWS=18)
    got, st = _capped(43, nj, profile=True, eager_scalars=True)
    _check_capped("classic", 43, nj, 18, "unmerged", got, st, ref)


# ------------------------------------------------------------------ 4. the two kernels of the two-kernel iteration
_VK_REF = {}


def _vk_reference(ni, nj, monkeypatch):
    """3-row chunks, 64-column tiles with halo loads: the configuration test_two_kernel_iteration_odd_shapes pins.  Once per shape."""
    if (ni, nj) not in _VK_REF:
        _set(monkeypatch, TM_APPLY_ROWS=3, TM_VK_OVERLAP=0)
        ref, st = _capped(ni, nj)
        assert st["inner_iterations"] == 10
        ref.setflags(write=False)
        _VK_REF[(ni, nj)] = ref
    return _VK_REF[(ni, nj)]


@pytest.mark.parametrize("overlap", [0, 1], ids=["halo", "overlap"])
@pytest.mark.parametrize("h,rows,nj", VK_CASES, ids=_ids(VK_CASES))
def test_two_kernel_iteration_at_every_chunk_height(h, rows, nj, overlap, monkeypatch):
    # k_apply_vk<VK_R> stores r', p' and u for the owner of a node as its row ENTERS the window; the chunk's first halo row and the rows past
    # its end belong to the neighbours.  Tall chunks put seams, short last chunks and the clamped loads behind the block's last row where
    # 3-row chunks never have them.
    ni = rows + 2
    ref = _vk_reference(ni, nj, monkeypatch)
    _set(monkeypatch, TM_APPLY_ROWS=h, TM_VK_OVERLAP=overlap)
    got, st = _capped(ni, nj)
    _check_capped("two-kernel", ni, nj, h, "overlap" if overlap else "halo", got, st, ref)


@pytest.mark.parametrize("nj", [9, 66])
def test_two_kernel_iteration_with_the_spilling_vk_r_variant(nj, monkeypatch):
    # 798 interior rows in 3-row chunks: 266 interior workgroups and the perimeter rows' behind them -- more than 256, at most 2048, so
    # launch_apply_virtual takes k_apply_vk<.., VK_R, MINW = 2>, the variant that spills registers (no odd-shape test launches that many)
    _set(monkeypatch, TM_APPLY_ROWS=None, TM_VK_OVERLAP=None)
    ref, _ = _capped(800, nj, eager_scalars=True)
    got, st = _capped(800, nj)
    _check_capped("spilling", 800, nj, "default", "halo", got, st, ref)


def test_chunks_taller_than_the_blocks_of_a_multi_block_mesh(monkeypatch):
    # the multi-block rule (24 rows for every block when no common height fits 512 workgroups) on blocks of 12 interior rows; 11 blocks: the
    # interior rows go out in two launches and the perimeter rows in a third.  Run as test_more_blocks_than_one_batch_launch_holds runs it.
    _set(monkeypatch, TM_APPLY_ROWS=24, TM_VK_OVERLAP=None)
    build = lambda tfi=None: configs.strip(11, 14, 23, reverse_odd=True, tfi=tfi)
    om = OracleMesh(build(oracle_tfi))
    oracle.picard_exact(om, 3)
    for eager in (False, True):
        mesh = build()
        with smooth.Smoother(mesh, solver.Option.hip(rtol=1e-13, max_inner=5000, eager_scalars=eager)) as sm:
            st = sm.iterate(3)
            sm.download()
        assert st["not_converged"] == 0
        rms = float(np.sqrt(np.mean((mesh_flat(mesh) - om.flat()) ** 2)))
        _report("strip11", "11x(14x23)", 24, "eager" if eager else "lazy", rms)
        assert rms <= 1e-10, (eager, rms)


# ------------------------------------------------------------------ 5. the heights the library chooses
@pytest.mark.parametrize("ni,nj,inner,expected", [(1545, 9, solver.Inner.bicgstab, 6), (7700, 9, solver.Inner.gmres, 18)], ids=["1545x9-bicgstab-6", "7700x9-gmres-18"])
def test_the_librarys_own_chunk_height_on_tall_thin_blocks(ni, nj, inner, expected, monkeypatch):
    # Smoother::size_launches, one 256-column workgroup per chunk, 128 perimeter rows per workgroup:
    #   1545 x 9, BiCGStab: 1543 interior rows = 515 chunks of 3 (> 512 without the perimeter rows), 258 chunks of 6 + 3104 perimeter rows in
    #                       25 workgroups <= 512 -> shortest_rows gives 6;
    #   7700 x 9, GMRES:    the search ends at 15 rows (7698 / 15 -> 514 chunks > 512), no common height -> the per-block rule
    #                       (rows_per_chunk, tm_kernels.hip): the first multiple of 3 with at most 512 chunks, capped at 18 -> 18 (428 chunks).
    # With nothing set the run must equal the run forced to that height bit for bit: same launches, same deterministic sums.  Another
    # height groups the partial sums differently (the distance to it is printed, not asserted: it may be zero by chance).
    opt = dict(inner=inner)
    _set(monkeypatch, TM_APPLY_ROWS=None, TM_VK_OVERLAP=None)
    own, st = _capped(ni, nj, **opt)
    _set(monkeypatch, TM_APPLY_ROWS=expected)
    forced, _ = _capped(ni, nj, **opt)
    _set(monkeypatch, TM_APPLY_ROWS=expected + 6)
    other, _ = _capped(ni, nj, **opt)
    _report("own-height", f"{ni}x{nj}", expected, inner.name, float(np.abs(own - forced).max()))
    _report("own-height", f"{ni}x{nj}", expected + 6, inner.name, float(np.abs(own - other).max()))
    seed = configs.single_block(ni, nj, perturb=0.2).blocks[0].points.data
    assert np.isfinite(own).all() and st["inner_iterations"] == 10
    assert not np.array_equal(own[1:-1, 1:-1], seed[1:-1, 1:-1])
    assert np.array_equal(own, forced), (ni, nj, expected, float(np.abs(own - forced).max()))
