"""The multigrid preconditioner of Inner.mg_bicgstab pinned as an OPERATOR: its transfer kernels one by one, the level hierarchy, the V-cycle
of lone blocks and the whole Smoother::precondition of coupled meshes, each against the plain-numpy reference of tests/mg_reference.py in
longdouble.  (The solver tests only see that BiCGStab still converges, which it does with any non-singular preconditioner.)

Tolerance of the cycle and preconditioner comparisons, from the reference alone: d = rms(z_float64 - z_longdouble) of the host reference for the
case; the device must lie within 16 d of the longdouble result.  tests/test_mg_reference_cpu.py shows that a wrong transfer weight, a missing
(s_i s_j)^2, undoubled P,Q, a mishandled short last cell, missing ring corners or omega = 0.79 each move z by more than 1000 such tolerances.
With TM_MG_PARITY_OUT=<file> every comparison appends "case env d distance ratio" to that file (profiles/mg_vcycle_parity.txt)."""
import os

import numpy as np
import pytest

from tests import mg_reference as ref
from tests.conftest import OracleMesh, oracle_tfi
from tests.meshes import TOPOLOGIES
from turbomesh_amd import _capi, configs
from turbomesh_amd.smoothing import smooth, solver, wall_control_function as wcf

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
LD = np.longdouble
MG = dict(inner=solver.Inner.mg_bicgstab, rtol=1e-12, max_inner=500, check_every=1)
WHITE = ("white", 0.02, 0.5 * np.pi)
UNFUSED = {"TM_MG_PAIR": "0", "TM_MG_RESTRICT_FUSED": "0", "TM_MG_FUSE_PROLONG": "0"}


def _rand(shape, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, shape)


def _perimeter(a):
    return np.concatenate([a[0].ravel(), a[-1].ravel(), a[1:-1, 0].ravel(), a[1:-1, -1].ravel()])


# ------------------------------------------------------------------ the four transfer kernels, each alone
TRANSFER_SHAPES = [(5, 5, 1, 1), (6, 6, 1, 1), (9, 8, 1, 1), (7, 6, 1, 1), (5, 300, 1, 1), (300, 4, 1, 0), (4, 300, 0, 1), (33, 259, 0, 1), (33, 259, 1, 0),
                   (70001, 9, 1, 1), (131077, 5, 1, 1)]


def _probe(kind, nif, njf, ci, cj, inp, out, xc=None, sx=1.0, sy=1.0):
    inp = np.ascontiguousarray(inp, dtype=np.float64)
    out = np.ascontiguousarray(out, dtype=np.float64).copy()
    xc = None if xc is None else np.ascontiguousarray(xc, dtype=np.float64)
    _capi.check(_capi.lib().tm_mg_transfer_probe(kind, nif, njf, ci, cj, _capi.f64ptr(inp), None if xc is None else _capi.f64ptr(xc), sx, sy, _capi.f64ptr(out)))
    return out


def _coarse_shape(nif, njf, ci, cj):
    return (nif // 2 + 1 if ci else nif, njf // 2 + 1 if cj else njf)


@pytest.mark.parametrize("nif,njf,ci,cj", TRANSFER_SHAPES)
def test_injection_is_bit_exact(nif, njf, ci, cj):
    fine = _rand((nif, njf, 2), 1)
    nic, njc = _coarse_shape(nif, njf, ci, cj)
    for sx, sy in ((1.0, 1.0), (2.0 if ci else 1.0, 2.0 if cj else 1.0)):   # coordinates; P,Q doubled per coarsened direction
        got = _probe(0, nif, njf, ci, cj, fine, np.full((nic, njc, 2), np.nan), sx=sx, sy=sy)
        assert np.array_equal(got, ref.inject(fine, ci, cj, sx, sy))


@pytest.mark.parametrize("nif,njf,ci,cj", TRANSFER_SHAPES)
def test_restriction_against_longdouble(nif, njf, ci, cj):
    r = _rand((nif, njf, 2), 2)
    nic, njc = _coarse_shape(nif, njf, ci, cj)
    ii, jj = np.meshgrid(np.arange(nic, dtype=np.float64), np.arange(njc, dtype=np.float64), indexing="ij")
    xc = np.stack([0.01 * ii + 0.002 * jj, 0.013 * jj - 0.001 * ii], axis=-1) + 0.002 * _rand((nic, njc, 2), 3)   # a perturbed sheared lattice
    sentinel = np.full((nic, njc, 2), 7.0)
    got = _probe(1, nif, njf, ci, cj, r, sentinel, xc=xc)
    want, mag = ref.restrict(r, xc, ci, cj, LD, with_bound=True)
    assert np.array_equal(_perimeter(got), _perimeter(sentinel))   # the perimeter is not written
    if nic >= 3 and njc >= 3:
        err = np.abs(got.astype(LD) - want)[1:-1, 1:-1]
        assert np.all(err <= 32 * EPS * mag[1:-1, 1:-1]), float((err / mag[1:-1, 1:-1]).max() / EPS)
        assert np.abs(want[1:-1, 1:-1]).max() > 0


@pytest.mark.parametrize("nif,njf,ci,cj", TRANSFER_SHAPES)
def test_prolong_add_against_longdouble(nif, njf, ci, cj):
    nic, njc = _coarse_shape(nif, njf, ci, cj)
    ec, e = _rand((nic, njc, 2), 4), _rand((nif, njf, 2), 5)
    got = _probe(2, nif, njf, ci, cj, ec, e)
    add, mag = ref.prolong(ec, nif, njf, ci, cj, LD, with_bound=True)
    assert np.array_equal(_perimeter(got), _perimeter(e))   # interior fine nodes only
    err = np.abs(got.astype(LD) - (e.astype(LD) + add))
    assert np.all(err <= 8 * EPS * (np.abs(e) + mag))
    assert not np.array_equal(got[1:-1, 1:-1], e[1:-1, 1:-1])


@pytest.mark.parametrize("nif,njf,ci,cj", TRANSFER_SHAPES)
def test_scale_is_bit_exact_with_a_zero_perimeter(nif, njf, ci, cj):
    f = _rand((nif, njf, 2), 6)
    got = _probe(3, nif, njf, ci, cj, f, np.full((nif, njf, 2), np.nan), sx=0.8)
    want = np.zeros_like(f)
    want[1:-1, 1:-1] = 0.8 * f[1:-1, 1:-1]
    assert np.array_equal(got, want) and not _perimeter(got).any()


# ------------------------------------------------------------------ the level rule
@pytest.mark.parametrize("name", list(ref.level_blocks()))
def test_handle_builds_the_hierarchy_of_the_level_rule(name):
    mesh = ref.level_blocks(oracle_tfi)[name]()
    xy = mesh.blocks[0].points.data
    with smooth.Smoother(mesh, solver.Option.hip(**MG)) as sm:
        got = sm.mg_levels(0)
    assert got["levels"] == ref.level_rule(xy.shape[0], xy.shape[1], ref.mean_aspect(xy)), name
    assert (got["nu_pre"], got["nu_post"], got["nu_coarsest"], got["omega"]) == (2, 2, 8, 0.8)
    assert (got["dirichlet"], got["perimeter_step"], got["perimeter_sweeps"]) == (False, False, 2)   # a lone block with a fixed perimeter


# ------------------------------------------------------------------ cycle and preconditioner against the reference
_REF = {}


def _build(case):
    """case -> (mesh, control algorithm of the handle, oracle control)"""
    if isinstance(case, tuple):
        return configs.single_block(case[0], case[1], tfi=oracle_tfi, perturb=0.2), None, None
    if case == "stretched":
        return ref.stretched_block(tfi=oracle_tfi), None, None
    if case == "plate_le_white":
        return TOPOLOGIES["plate_le"](tfi=oracle_tfi), wcf.Algorithm(wcf.White(0.02)), WHITE
    return TOPOLOGIES[case](tfi=oracle_tfi), None, None


def _reference(case, info, pq, f, key):
    """(z_float64, z_longdouble, identity rows) of the host reference for the handle's cycle parameters; computed once per key."""
    if key not in _REF:
        mesh, _, control = _build(case)
        om = OracleMesh(mesh)
        coupled = bool(om.connections or om.bcs)
        cycle = dict(nu_pre=info["nu_pre"], nu_post=info["nu_post"], nu_coarsest=info["nu_coarsest"], omega=info["omega"])
        out = []
        for dt in (np.float64, LD):
            rx, ry, _ = ref.oracle_rows(om, control, dt) if coupled else (None, None, None)
            out.append(ref.precondition(om.blocks, f, rx, ry, pq, coupled, info["perimeter_sweeps"], cycle, dt))
        fixed = ((np.diff(rx.indptr) == 1) & (np.diff(ry.indptr) == 1)) if coupled else np.concatenate([ref.perimeter_mask(*b.shape[:2]).ravel() for b in om.blocks])
        _REF[key] = (out[0], out[1], fixed, om)
    return _REF[key]


def _report(case, env, what, d, dist):
    line = f"{str(case).replace(' ', ''):28s} {env:24s} {what:10s} d {d:.3e}  device {dist:.3e}  ratio {dist / d if d > 0 else float('nan'):.2f}"
    print(line)
    if os.environ.get("TM_MG_PARITY_OUT"):
        with open(os.environ["TM_MG_PARITY_OUT"], "a") as fh:
            fh.write(line + "\n")


def _within(case, env, what, z, z64, zld, sel=slice(None)):
    d, dist = ref.rms(z64[sel] - zld[sel]), ref.rms(z[sel].astype(LD) - zld[sel])
    _report(case, env, what, d, dist)
    assert dist <= 16.0 * d, (case, env, what, d, dist, dist / d if d > 0 else None)


def _ring_mask(blocks):
    out = []
    for b in blocks:
        ni, nj = b.shape[:2]
        m = np.zeros((ni, nj), dtype=bool)
        m[1:-1, 1:-1] = True
        m[2:-2, 2:-2] = False
        out.append(m.ravel())
    return np.concatenate(out)


def _run(case, env_name, env, monkeypatch, full=False):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    mesh, algo, _ = _build(case)
    with smooth.Smoother(mesh, solver.Option.hip(**MG), algo) as sm:
        info = sm.mg_levels(0)
        f = _rand((sm.dof, 2), 31)
        pq = sm.control_function() if algo is not None else None
        assert pq is None or np.abs(pq).max() > 1e-3   # the P,Q path and its doubling run on a field that is there
        z, after = sm.precondition_probe(f, return_input=True)
        z2 = sm.precondition_probe(f) if full else None
        key = (case, info["nu_pre"], info["nu_post"], info["nu_coarsest"], info["omega"], info["perimeter_sweeps"])
        z64, zld, fixed, om = _reference(case, info, pq, f, key)
        xy0 = om.blocks[0]
        assert info["levels"] == ref.level_rule(xy0.shape[0], xy0.shape[1], ref.mean_aspect(xy0))
        assert np.array_equal(after, f)   # the ring of the input buffer is restored to the bit
        assert np.array_equal(z[fixed], f[fixed])   # identity rows
        _within(case, env_name, "z", z, z64, zld)
        if full:
            perim = np.concatenate([ref.perimeter_mask(*b.shape[:2]).ravel() for b in om.blocks])
            _within(case, env_name, "perimeter", z, z64, zld, perim)
            _within(case, env_name, "ring", z, z64, zld, _ring_mask(om.blocks))
            assert np.array_equal(z, z2)   # the cycles of the blocks run on streams of their own: fork and join order them
            g = _rand((sm.dof, 2), 32)
            alpha, beta = 1.5, -0.25
            zg, zc = sm.precondition_probe(g), sm.precondition_probe(alpha * f + beta * g)
            rel = 16.0 * ref.rms(z64 - zld) / ref.rms(zld)
            lin = ref.rms(zc.astype(LD) - (alpha * z.astype(LD) + beta * zg.astype(LD)))
            assert lin <= rel * (abs(alpha) * ref.rms(z) + abs(beta) * ref.rms(zg)), (case, lin, rel)
    return z


# (1545, 9), (7700, 5): tall thin blocks whose fine levels take 6- and 18-row chunks by the per-block rule of K2 (more than 512 chunks of
# 3 .. 15 rows), so `unfused` sends them through MODE_MG_FIRST2 / MODE_MG_RESID / MODE_MG_SMOOTH of the six-row-group k_apply; every other
# lone block here fits 512 workgroups at 3 rows
LONE = [(5, 5), (6, 6), (9, 8), (33, 33), (34, 61), (66, 122), (5, 70), (300, 4), "stretched", "plate_le_white", (1545, 9), (7700, 5)]


@pytest.mark.parametrize("case", LONE, ids=str)
@pytest.mark.parametrize("env_name,env", [("default", {}), ("unfused", UNFUSED)])
def test_vcycle_against_the_reference_cycle(case, env_name, env, monkeypatch):
    _run(case, env_name, env, monkeypatch)


@pytest.mark.parametrize("case", [(1545, 9), (7700, 5)], ids=str)
def test_vcycle_of_tall_blocks_is_the_same_bit_for_bit_one_sweep_per_pass(case, monkeypatch):
    # The 16 d bar above cannot see a last bit.  The one-sweep-per-pass cycle (the MODE_MG_* levels of k_apply, here with six-row groups on
    # the fine level) performs the operation sequence of the default cycle (k_mg_pair, the prolongation folded in) node by node -- tests/
    # test_gpu_multigrid.py pins that on whole solves at 3-row chunks -- so one application of the preconditioner gives the same bits.
    out = []
    for env in ({}, UNFUSED):
        for k in UNFUSED:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        mesh, _, _ = _build(case)
        with smooth.Smoother(mesh, solver.Option.hip(**MG)) as sm:
            out.append(sm.precondition_probe(_rand((sm.dof, 2), 31)))
    assert np.isfinite(out[0]).all() and np.abs(out[0]).max() > 0
    assert np.array_equal(out[0], out[1]), float(np.abs(out[0] - out[1]).max())


def test_vcycle_with_the_prolongation_folded_on_every_level(monkeypatch):
    _run((66, 122), "fuse_prolong=2", {"TM_MG_PAIR": "0", "TM_MG_FUSE_PROLONG": "2"}, monkeypatch)
    _run((66, 122), "pair+fuse_prolong=2", {"TM_MG_FUSE_PROLONG": "2"}, monkeypatch)


def test_vcycle_with_one_sweep_each_side_and_odd_ping_pong_counts(monkeypatch):
    # nu_pre = 1: the scale-first path; 1 + 1 and 1 + 3 sweeps: odd flip counts on the fine and on the last level
    monkeypatch.setenv("TM_MG_CYCLE", "1,1,3,0.7")
    mesh, _, _ = _build((34, 61))
    with smooth.Smoother(mesh, solver.Option.hip(**MG)) as sm:
        info = sm.mg_levels(0)
    assert (info["nu_pre"], info["nu_post"], info["nu_coarsest"], info["omega"]) == (1, 1, 3, 0.7)
    _run((34, 61), "cycle=1,1,3,0.7", {}, monkeypatch)


COUPLED = ["strip3_reversed", "two_by_two_junction", "channel_periodic_sliding", "channel_periodic_fixed", "plate_le_white"]


@pytest.mark.parametrize("case", COUPLED)
@pytest.mark.parametrize("env_name,env", [("default", {}), ("perimeter_sweeps=1", {"TM_MG_PERIMETER_SWEEPS": "1"})])
def test_whole_preconditioner_on_coupled_meshes(case, env_name, env, monkeypatch):
    mesh, algo, _ = _build(case)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with smooth.Smoother(mesh, solver.Option.hip(**MG), algo) as sm:
        info = sm.mg_levels(0)
    assert info["dirichlet"] and info["perimeter_step"] and info["perimeter_sweeps"] == (1 if env else 2)
    _run(case, env_name, env, monkeypatch, full=True)


# ------------------------------------------------------------------ the probe itself
@pytest.mark.parametrize("case", ["strip3_reversed", "plate_le_white"])
def test_probe_leaves_the_handle_as_it_found_it(case):
    a, algo, _ = _build(case)
    b, _, _ = _build(case)
    with smooth.Smoother(a, solver.Option.hip(**MG), algo) as sm:
        st_a = [sm.iterate(1), sm.iterate(1)]
        sm.download()
    with smooth.Smoother(b, solver.Option.hip(**MG), algo) as sm:
        f = _rand((sm.dof, 2), 41)
        sm.precondition_probe(f)
        st_b = [sm.iterate(1)]
        sm.precondition_probe(f, return_input=True)
        st_b.append(sm.iterate(1))
        sm.download()
    for x, y in zip(a.blocks, b.blocks):
        assert np.array_equal(x.points.data, y.points.data)
    for x, y in zip(st_a, st_b):
        assert x["inner_iterations"] == y["inner_iterations"] and x["last_residual"] == y["last_residual"] and y["not_converged"] == 0


def test_probes_refuse_a_handle_without_multigrid():
    mesh = configs.single_block(9, 9, tfi=oracle_tfi)
    with smooth.Smoother(mesh, solver.Option.hip(inner=solver.Inner.bicgstab)) as sm:
        with pytest.raises(_capi.TmError) as e:
            sm.precondition_probe(np.zeros((sm.dof, 2)))
        assert e.value.code == _capi.TM_E_UNSUPPORTED
        with pytest.raises(_capi.TmError) as e:
            sm.mg_levels(0)
        assert e.value.code == _capi.TM_E_UNSUPPORTED
        st = sm.iterate(1)
        assert st["not_converged"] == 0
