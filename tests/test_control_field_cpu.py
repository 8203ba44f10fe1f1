"""CPU: the Thomas-Middlecoff / prescribed control field -- what the field does (on the exact-Picard oracle, with the field written into
the oracle's control_function view) and the plumbing of the two new kinds through the front ends.  The device side is
tests/test_gpu_control_field.py."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from oracle import oracle
from tests import control_field_reference as cfr
from turbomesh_amd import _capi
from turbomesh_amd.smoothing import wall_control_function as wcf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a) - np.asarray(b)) ** 2)))


# ------------------------------------------------------------------ the reference itself
def test_reference_edge_function_by_hand():
    # three points: one interior point, both ends copy it
    e = np.array([[0.0, 0.0], [1.0, 0.0], [3.0, 0.0]])
    # d1 = (3 - 0) / 2 = 1.5, d2 = 3 - 2 + 0 = 1, f = -1.5 / 2.25
    f = cfr.edge_function(e)
    assert np.allclose(np.asarray(f, dtype=float), -2.0 / 3.0, rtol=1e-15) and f.shape == (3,)
    assert np.array_equal(cfr.edge_function(e[:2]), np.zeros(2))
    # coincident neighbours: d1 = 0 at k = 1 -> 0 there, finite everywhere
    e = np.array([[0.0, 0.0], [5.0, 1.0], [0.0, 0.0], [1.0, 1.0], [2.0, 3.0]])
    f = np.asarray(cfr.edge_function(e), dtype=float)
    assert f[1] == 0.0 and f[0] == 0.0 and np.isfinite(f).all()
    # a uniform straight edge has no second difference; the absolute variant bounds the signed one
    assert np.array_equal(cfr.edge_function(np.stack([np.arange(7.0), 2 * np.arange(7.0)], axis=1)), np.zeros(7))
    r = cfr.bent_clustered(9, 7)
    assert np.all(np.abs(cfr.block_field(r)) <= cfr.block_field(r, absolute=True))


def test_reference_blend_takes_the_edges_values_on_the_edges():
    r = cfr.bent_clustered(12, 9)
    f = cfr.block_field(r)
    assert np.array_equal(f[:, 0, 0], cfr.edge_function(r[:, 0])) and np.array_equal(f[:, -1, 0], cfr.edge_function(r[:, -1]))
    assert np.array_equal(f[0, :, 1], cfr.edge_function(r[0, :])) and np.array_equal(f[-1, :, 1], cfr.edge_function(r[-1, :]))
    assert cfr.mesh_field([r, r[:5]]).shape == (12 * 9 + 5 * 9, 2)


# ------------------------------------------------------------------ what the field does (exact Picard on the oracle)
def test_separable_clustered_rectangle_is_a_fixed_point_under_the_field_and_not_under_laplace():
    seed = cfr.rectangle(33, 25, bend=0.0)
    om = cfr.OracleBlocks([seed])
    with cfr.field_in_oracle(cfr.tm_field64):
        oracle.picard_exact(om, 5)
    moved = _rms(om.blocks[0], seed)
    print(f"separable rectangle, 5 exact Picard iterations under the field: moved {moved:.3e} rms")
    assert moved <= 1e-13
    om = cfr.OracleBlocks([seed])
    oracle.picard_exact(om, 5)
    moved = _rms(om.blocks[0], seed)
    print(f"... under laplace: moved {moved:.3e} rms")
    assert moved > 1e-2


def test_bent_rectangle_keeps_its_wall_spacing_under_the_field():
    seed = cfr.rectangle(33, 25, bend=cfr.BEND)
    om = cfr.OracleBlocks([seed])
    with cfr.field_in_oracle(cfr.tm_field64):   # evaluated once from the seed, frozen
        hist, _ = oracle.picard_exact(om, 12)
    ratio = cfr.first_cell_height_ratio(om.blocks[0], seed)
    print(f"bent rectangle under the field: first-cell height / seed's in [{ratio.min():.3f}, {ratio.max():.3f}], moved {_rms(om.blocks[0], seed):.2e} rms, "
          f"last Picard residual {hist[-1]:.1e}")
    assert np.isfinite(om.blocks[0]).all()
    assert ratio.min() >= 0.8 and ratio.max() <= 1.1
    om = cfr.OracleBlocks([seed])
    oracle.picard_exact(om, 12)
    ratio = cfr.first_cell_height_ratio(om.blocks[0], seed)
    print(f"... under laplace: [{ratio.min():.1f}, {ratio.max():.1f}], mid-chord {ratio[len(ratio) // 2]:.1f}")
    assert ratio[len(ratio) // 2] > 10


# ------------------------------------------------------------------ plumbing
def test_c_struct_kinds_and_sizes():
    assert (_capi.TM_CF_LAPLACE, _capi.TM_CF_WHITE, _capi.TM_CF_PRESCRIBED, _capi.TM_CF_THOMAS_MIDDLECOFF) == (0, 1, 2, 3)
    assert wcf.Algorithm.laplace().c_struct().kind == 0
    assert wcf.Algorithm(wcf.White(1e-3)).c_struct().kind == 1 and wcf.Algorithm(wcf.White(1e-3)).c_struct().ds_target == 1e-3
    tm = wcf.Algorithm.thomas_middlecoff().c_struct()
    assert (tm.kind, tm.ds_target, tm.theta_target) == (3, 0.0, 0.0)
    fields = [np.zeros((4, 5, 2)), np.ones((3, 3, 2))]
    pre = wcf.Algorithm.prescribed(fields)
    assert pre.c_struct().kind == 2 and len(pre.fields) == 2 and pre.fields[1].flags["C_CONTIGUOUS"]
    with pytest.raises(ValueError):
        wcf.Algorithm.prescribed([np.zeros((4, 5))])
    assert ctypes.sizeof(_capi.tm_control_fn) == 24 and ctypes.sizeof(_capi.tm_solver_opt) == 48
    assert _capi.lib().tm_abi_version() == 1


def test_header_keeps_the_struct_and_declares_the_kinds():
    src = open(os.path.join(ROOT, "include", "tm_hip.h")).read()
    assert re.search(r"TM_CF_LAPLACE = 0, TM_CF_WHITE = 1, TM_CF_PRESCRIBED = 2, TM_CF_THOMAS_MIDDLECOFF = 3", src)
    body = re.search(r"typedef struct tm_control_fn \{(.*?)\} tm_control_fn;", src, flags=re.S).group(1)
    assert [ln.strip() for ln in body.strip().splitlines()] == ["int32_t kind;", "int32_t _pad;", "double ds_target;", "double theta_target;"]
    assert "#define TM_HIP_ABI_VERSION 1" in src


def test_new_symbols_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tm_hip.h")).read(), flags=re.S)
    lib = _capi.lib()
    for name in ("tm_smoother_set_control_function", "tm_smoother_update_control_function"):
        assert re.search(r"\bint " + name + r"\s*\(", src), name
        assert name in _capi.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert lib.tm_smoother_set_control_function.argtypes == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
    assert lib.tm_smoother_update_control_function.argtypes == [ctypes.c_void_p]
    diag = open(os.path.join(ROOT, "include", "tm_hip_diag.h")).read()
    assert "tm_smoother_set_control_function" not in diag and "tm_smoother_update_control_function" not in diag
    # the C++ mirror has the two members too
    hpp = open(os.path.join(ROOT, "turbomesh_amd", "host", "turbomesh.hpp")).read()
    assert "static Algorithm thomas_middlecoff()" in hpp and "static Algorithm prescribed(" in hpp


def test_null_handles_are_refused_without_a_gpu():
    lib = _capi.lib()
    pq = np.zeros(2)
    assert lib.tm_smoother_set_control_function(None, _capi.f64ptr(pq)) == _capi.TM_E_ARG
    assert lib.tm_smoother_update_control_function(None) == _capi.TM_E_ARG


def test_input_file_parses_thomas_middlecoff():
    from turbomesh_amd.input import Input

    j = json.load(open(os.path.join(ROOT, "tests", "golden", "examples", "T106", "T106.json")))
    assert Input.parse(json.dumps(j)).wall_control_function.c_struct().kind == _capi.TM_CF_WHITE   # as the file has it
    j["smoothing"]["wall_control_function"] = {"thomas_middlecoff": {}}
    inp = Input.parse(json.dumps(j))
    assert inp.wall_control_function.c_struct().kind == _capi.TM_CF_THOMAS_MIDDLECOFF and inp.wall_control_function.white is None
    j["smoothing"]["wall_control_function"] = {"laplace": {}}
    assert Input.parse(json.dumps(j)).wall_control_function.c_struct().kind == _capi.TM_CF_LAPLACE
    j["smoothing"]["wall_control_function"] = {"steger_sorenson": {}}
    with pytest.raises(ValueError, match="steger_sorenson"):
        Input.parse(json.dumps(j))


def test_cli_refuses_an_unknown_control(capsys):
    from turbomesh_amd.__main__ import main

    with pytest.raises(SystemExit) as e:
        main(["nowhere.json", "--control", "winslow"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--control" in err and "thomas-middlecoff" in err
