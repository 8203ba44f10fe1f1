"""Timing of the reference route (TM_INNER_REFERENCE_GMRES): one ILU(0) application M^-1 r on the assembled T106 and LS89 systems, by the
level-packed substitution kernels (k_ilu_subst_packed) and by the level-by-level kernels they replace in the substitutions (k_ilu_levels,
unchanged since they were the only path) -- an event pair per repeat, through the measurement build (libtm_hip_dbg.so) -- and the whole
T106 job as its input file writes it (10 outer iterations, White, GMRES(30) + ILU(0)), wall time of iterate() on a warm handle.

    python tools/reference_solve_timing.py [--repeats 7] [--out profiles/reference_solve_timing.txt]      (needs the MI355X)"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("TM_HIP_LIB", os.path.join(ROOT, "turbomesh_amd", "libtm_hip_dbg.so"))   # one library in the process: the measurement build

import numpy as np  # noqa: E402

from oracle import oracle  # noqa: E402
from tests import reference_yardstick as ry  # noqa: E402
from tests.conftest import OracleMesh  # noqa: E402
from turbomesh_amd import _capi  # noqa: E402
from turbomesh_amd.smoothing import smooth, solver, wall_control_function as wcf  # noqa: E402


def spread(v):
    v = np.asarray(v)
    return f"median {np.median(v):9.4f}  min {v.min():9.4f}  max {v.max():9.4f}"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("profiles", "reference_solve_timing.txt"))
    args = ap.parse_args()
    oracle.build()
    L = _capi.lib()
    ip = C.POINTER(C.c_int32)
    L.tm_debug_ilu0_apply_ms.argtypes = [C.c_uint64, ip, ip, C.POINTER(C.c_double), C.c_int, C.c_int, C.POINTER(C.c_double), ip]
    lines = [f"one ILU(0) application M^-1 r (both components), ms, {args.repeats} repeats after a warm-up (tools/reference_solve_timing.py)"]
    for name in ry.EXAMPLES:
        mesh, control, _ = ry.case(name)
        s = oracle.System(OracleMesh(mesh), control)
        s.fill(0)
        s.fill_x_specific()
        p, ci, v = np.array(s.lhs_p, dtype=np.int32), np.array(s.lhs_i, dtype=np.int32), s.lhs_values.copy()   # copies: the views die with the system
        s.close()
        med = {}
        for packed in (0, 1):
            ms = np.zeros(args.repeats)
            lev = C.c_int32(0)
            _capi.check(L.tm_debug_ilu0_apply_ms(len(p) - 1, p.ctypes.data_as(ip), ci.ctypes.data_as(ip), _capi.f64ptr(v), packed, args.repeats, _capi.f64ptr(ms), C.byref(lev)))
            med[packed] = float(np.median(ms))
            lines.append(f"  {name} ({len(p) - 1} rows, {lev.value} levels forward + backward)  {'packed       ' if packed else 'level kernels'}  {spread(ms)}   "
                         f"{1e3 * med[packed] / lev.value:6.3f} us per level")
        lines.append(f"  {name}: packed is {med[0] / med[1]:.2f} x faster (medians)")
    lines.append("")
    lines.append(f"T106 as written, 10 outer iterations (White, GMRES(30) + ILU(0)): seconds of iterate(10), {max(5, args.repeats)} handles, the first discarded as warm-up")
    for packed in (0, 1):
        os.environ["TM_ILU_PACKED"] = str(packed)   # read when a handle is created
        secs, inner = [], None
        for q in range(max(5, args.repeats) + 1):
            mesh, control, iters = ry.case("T106")
            with smooth.Smoother(mesh, solver.Option.hip(inner=solver.Inner.reference_gmres, preconditioner=solver.Preconditioner.ilu0),
                                 wcf.Algorithm(wcf.White(control[1], control[2]))) as sm:
                st = sm.iterate(iters)
            if q:
                secs.append(st["seconds"])
            inner = st["inner_iterations"]
        lines.append(f"  {'packed       ' if packed else 'level kernels'}  {spread(secs)}   ({inner} inner iterations)")
    os.environ.pop("TM_ILU_PACKED", None)
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
