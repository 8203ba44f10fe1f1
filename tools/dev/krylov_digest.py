"""One line per inner-solver route: sha256 of the result and the counters that go with it.  Every reduction of the library is in fixed
order and it uses no float atomics, so two builds that enqueue the same launches print the same lines, byte for byte -- the check behind a
change to the host code of the Krylov loops (profiles/krylov_refactor_digest*.txt).  TM_HIP_LIB selects the build, as everywhere.

    python tools/dev/krylov_digest.py > digest.txt"""
import ctypes as C
import hashlib
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np

from tests import refine_reference as rr
from tests.conftest import OracleMesh, mesh_flat
from tests.meshes import TOPOLOGIES
from turbomesh_amd import _capi, configs
from turbomesh_amd.smoothing import smooth, solver, wall_control_function as wcf

WHITE = wcf.Algorithm(wcf.White(0.02, 0.5 * math.pi))
MESHES = {
    "perturbed_33": (lambda: configs.single_block(33, 33, perturb=0.25), None),
    "two_by_two_junction": (lambda: TOPOLOGIES["two_by_two_junction"](None), None),
    "channel_periodic_sliding": (lambda: TOPOLOGIES["channel_periodic_sliding"](None), None),
    "strip3_reversed": (lambda: TOPOLOGIES["strip3_reversed"](None), None),
    "plate_white": (lambda: TOPOLOGIES["plate_le"](None), WHITE),
}
ILU0 = solver.Preconditioner.ilu0
# name -> (options, environment, takes TM_OPT_REFINE)
MODES = {
    "bicgstab": (dict(inner=solver.Inner.bicgstab), {}, True),
    "bicgstab_eager": (dict(inner=solver.Inner.bicgstab, eager_scalars=True), {}, True),
    "bicgstab_fuse2_off": (dict(inner=solver.Inner.bicgstab), {"TM_FUSE_2": "0"}, True),
    "bicgstab_fusep_off": (dict(inner=solver.Inner.bicgstab), {"TM_FUSE_P": "0"}, True),
    "mg_bicgstab": (dict(inner=solver.Inner.mg_bicgstab), {}, True),
    "gmres": (dict(inner=solver.Inner.gmres), {}, True),
    "reference_gmres": (dict(inner=solver.Inner.reference_gmres), {}, False),
    "reference_gmres_ilu0": (dict(inner=solver.Inner.reference_gmres, preconditioner=ILU0), {}, False),
}


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


def handle_case(mesh_name, mode_name, refine):
    build, control = MESHES[mesh_name]
    opts, env, _ = MODES[mode_name]
    mesh = build()
    os.environ.update(env)   # read when the handle is created
    try:
        with smooth.Smoother(mesh, solver.Option.hip(refine=refine, **opts), control) as sm:
            st = sm.iterate(3)
            counts = sm.inner_counts()
            report = sm.refine_report() if refine else None
            sm.download()
    except _capi.TmError as e:   # a combination the library refuses is refused by every build
        return f"refused code={e.code}"
    finally:
        for k in env:
            del os.environ[k]
    line = (f"{sha(mesh_flat(mesh))} inner_iterations={st['inner_iterations']} operator_sweeps={st['operator_sweeps']} "
            f"not_converged={st['not_converged']} inner_counts={counts}")
    return line + (f" refine={report}" if refine else "")


def slot_case(system, guess, **opts):
    p, i, vx, vy, bx, by = system
    ip = C.POINTER(C.c_int32)
    x, y = guess[:, 0].copy(), guess[:, 1].copy()
    o, st = solver.Option.hip(**opts).c_struct(), _capi.tm_stats()
    logged = []   # what the call reports through tm_set_log: the refinement figures
    sink = _capi.LOG_FN(lambda ctx, what, it, value: logged.append((int(what), float(value))))
    _capi.lib().tm_set_log(sink, None)
    try:
        rc = _capi.lib().tm_csr_solve(len(p) - 1, p.ctypes.data_as(ip), i.ctypes.data_as(ip), _capi.f64ptr(vx), _capi.f64ptr(vy), _capi.f64ptr(bx),
                                      _capi.f64ptr(by), _capi.f64ptr(x), _capi.f64ptr(y), C.byref(o), C.byref(st))
    finally:
        _capi.lib().tm_set_log(_capi.LOG_FN(), None)
    d = st.as_dict()
    return (f"{sha(x, y)} rc={rc} inner_iterations={d['inner_iterations']} operator_sweeps={d['operator_sweeps']} not_converged={d['not_converged']} "
            f"scaled_residual_rms={d['scaled_residual_rms']!r} log={logged}")


def main():
    for mesh_name in MESHES:
        for mode_name, (_, _, refinable) in MODES.items():
            for refine in (False, True) if refinable else (False,):
                name = f"handle {mesh_name} {mode_name}" + (" refine" if refine else "")
                print(name, handle_case(mesh_name, mode_name, refine), flush=True)
    for mesh_name in ("two_by_two_junction", "strip3_reversed"):
        mesh = MESHES[mesh_name][0]()
        system, guess = rr.system_of(OracleMesh(mesh)), mesh_flat(mesh).copy()
        for inner in (solver.Inner.bicgstab, solver.Inner.gmres):
            for precond in (solver.Preconditioner.diagonal, ILU0):
                for refine in (False, True):
                    name = f"slot {mesh_name} {inner.name} {precond.name}" + (" refine" if refine else "")
                    print(name, slot_case(system, guess, inner=inner, preconditioner=precond, refine=refine), flush=True)
        for inner in (solver.Inner.bicgstab, solver.Inner.gmres):   # the iteration cap
            print(f"slot {mesh_name} {inner.name} diagonal max_inner=5", slot_case(system, guess, inner=inner, max_inner=5), flush=True)


if __name__ == "__main__":
    main()
