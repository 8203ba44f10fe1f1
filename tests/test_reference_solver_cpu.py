"""CPU side of the reference route (TM_INNER_REFERENCE_GMRES, `--hip reference`): the front door's mapping, the enum's mirrors, and a pin of
the yardstick tests/test_gpu_reference_solver.py holds the device to (tests/reference_yardstick.py)."""
import os
import re

import numpy as np
import pytest

from oracle import oracle
from tests import reference_yardstick as ry
from tests.conftest import OracleMesh
from turbomesh_amd import _capi
from turbomesh_amd.smoothing import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the faithful GMRES(30) + ILU(0) run of the two example inputs: inner iterations (x + y) per outer iteration
COUNTS = {"T106": [391, 191, 182, 136, 135, 108, 89, 76, 80, 70], "LS89": [601, 526, 359, 207, 163, 156, 152, 152, 127, 110]}


def test_as_written_maps_gmres_to_the_reference_route():
    opt, note = solver.Option(tag=solver.Tag.gmres, preconditioner=solver.Preconditioner.ilu0).as_written()
    assert note is None and opt.tag == solver.Tag.hip and opt.inner == solver.Inner.reference_gmres and opt.preconditioner == solver.Preconditioner.ilu0
    assert opt.c_struct().inner == 5 and opt.c_struct().flags & 8
    opt, note = solver.Option(tag=solver.Tag.gmres, preconditioner=solver.Preconditioner.diagonal).as_written()
    assert note is None and opt.inner == solver.Inner.reference_gmres and opt.preconditioner == solver.Preconditioner.diagonal
    assert not opt.c_struct().flags & 8
    # every other tag has no as-written device form: the served_by_hip answer, with its note
    for tag in (solver.Tag.umfpack, solver.Tag.petsc, solver.Tag.bicgstab):
        o = solver.Option(tag=tag, preconditioner=solver.Preconditioner.ilu0)
        (a, na), (b, nb) = o.as_written(), o.served_by_hip()
        assert a == b and na == nb and na
    o = solver.Option.hip(inner=solver.Inner.relax)
    assert o.as_written() == (o, None)


def test_served_by_hip_keeps_its_answer_and_points_to_the_reference_route():
    opt, note = solver.Option(tag=solver.Tag.gmres, preconditioner=solver.Preconditioner.ilu0).served_by_hip()
    assert opt.inner == solver.Inner.gmres and opt.preconditioner == solver.Preconditioner.diagonal
    assert "ilu0 has no device counterpart" in note and "--hip reference" in note


def test_the_enum_value_is_mirrored_everywhere():
    assert _capi.TM_INNER_REFERENCE_GMRES == 5 and int(solver.Inner.reference_gmres) == 5
    header = open(os.path.join(ROOT, "include", "tm_hip.h")).read()
    assert re.search(r"\bTM_INNER_REFERENCE_GMRES\s*=\s*5\b", header)
    host = open(os.path.join(ROOT, "turbomesh_amd", "host", "turbomesh.hpp")).read()
    assert re.search(r"\breference_gmres\s*=\s*5\b", host)
    assert re.search(r"\breference_gmres\s*=\s*5\b", open(os.path.join(ROOT, "INTEGRATION.md")).read())
    assert "tm_smoother_inner_counts" in _capi.EXPORTS and re.search(r"\btm_smoother_inner_counts\s*\(", header)


@pytest.mark.parametrize("name", ry.EXAMPLES)
def test_the_yardstick_is_stable_under_perturbation(name):
    # the perturbation experiment behind the device tests' bound: the inner counts of ALL solves are unchanged and the oracle's distance from
    # itself stays finite and small -- a change of the oracle that makes the yardstick meaningless is noticed here
    mesh, control, iters = ry.case(name)
    base = ry.run(OracleMesh(mesh), iters, oracle.SOLVER_GMRES, oracle.PRECOND_ILU0, control)
    assert base[0] == COUNTS[name]
    dof = sum(b.points.data.shape[0] * b.points.data.shape[1] for b in mesh.blocks)
    for u in (1, ry.ulps_of(dof)):
        counts, self_k = ry.self_distance(mesh, control, iters, u, base=base)
        print(f"{name}: u = {u}: max self rms {max(self_k):.3e}")
        assert counts == COUNTS[name], (u, counts)
        assert np.isfinite(self_k).all() and 0.0 < max(self_k) < 1e-7, (u, self_k)
