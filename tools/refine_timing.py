"""Cost and effect of the iterative refinement (TM_OPT_REFINE).

Timing (-> profiles/refine_timing.txt): the double-double residual kernel k_csr_residual_dd against the fp64 residual k_csr_apply<true, DOT_NONE>
on the same assembled system -- T106 and a perturbed 2049^2 block assembled by tm_smoother_assemble_csr -- an event pair per repeat after a
warm-up, through the measurement build (libtm_hip_dbg.so); then a refined against an unrefined T106 job as written (ten outer iterations, White)
and one Picard iteration of a perturbed 1025^2 block, wall seconds of iterate() on fresh handles, the first discarded as warm-up.

Parity (--parity, -> profiles/refine_parity.txt): the RMS distance of every iterate of T106 and LS89 as written from the refined exact iteration
(tests/refine_reference.py, COLAMD), refined and unrefined, inner = bicgstab and auto, beside the distance between the two elimination orders.

    python tools/refine_timing.py [--repeats 7] [--parity] [--skip-timing]      (needs the MI355X)"""
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
from tests import refine_reference as rr  # noqa: E402
from tests.conftest import OracleMesh, mesh_flat  # noqa: E402
from turbomesh_amd import _capi, configs  # noqa: E402
from turbomesh_amd.smoothing import smooth, solver, wall_control_function as wcf  # noqa: E402


def spread(v):
    v = np.asarray(v)
    return f"median {np.median(v):9.4f}  min {v.min():9.4f}  max {v.max():9.4f}"


def kernel_ratio(lines, name, p, ci, v, repeats):
    L = _capi.lib()
    ip = C.POINTER(C.c_int32)
    L.tm_debug_csr_residual_ms.argtypes = [C.c_uint64, ip, ip, C.POINTER(C.c_double), C.c_int, C.c_int, C.POINTER(C.c_double)]
    med = {}
    for which in (0, 1):
        ms = np.zeros(repeats)
        _capi.check(L.tm_debug_csr_residual_ms(len(p) - 1, p.ctypes.data_as(ip), ci.ctypes.data_as(ip), _capi.f64ptr(v), which, repeats, _capi.f64ptr(ms)))
        med[which] = float(np.median(ms))
        gbs = (20.0 * len(ci) + 52.0 * (len(p) - 1)) / (1e6 * med[which])   # 20 B per non-zero; per row: row pointer, b and r (16 B each), x once
        lines.append(f"  {name} ({len(p) - 1} rows, {len(ci)} non-zeros)  {'k_csr_residual_dd       ' if which else 'k_csr_apply<true, NONE> '}  ms {spread(ms)}   ~{gbs:7.1f} GB/s")
    lines.append(f"  {name}: double-double / fp64 = {med[1] / med[0]:.2f} (medians; the aim was <= 1.5)")


def job_seconds(build, option, alg, iterations, handles):
    secs, rep = [], None
    for q in range(handles + 1):
        with smooth.Smoother(build(), option, alg) as sm:
            st = sm.iterate(iterations)
            rep = sm.refine_report() if option.refine else None
        if q:
            secs.append(st["seconds"])
    return secs, st["inner_iterations"], rep


def timing(args):
    lines = [f"residual of an assembled system, both components, {args.repeats} repeats after a warm-up (tools/refine_timing.py)"]
    mesh, control, iters = ry.case("T106")
    p, ci, v, _, _, _ = rr.system_of(OracleMesh(mesh), control)
    kernel_ratio(lines, "T106", p, ci, v, args.repeats)
    with smooth.Smoother(configs.single_block(2049, 2049, perturb=0.25), solver.Option.hip()) as sm:
        p, ci, v, _ = sm.assemble_csr()
    kernel_ratio(lines, "2049^2 block", p, ci, v, args.repeats)
    del p, ci, v
    lines.append("")
    handles = max(5, args.repeats)
    lines.append(f"seconds of iterate(), {handles} fresh handles after one discarded as warm-up")
    alg = wcf.Algorithm(wcf.White(control[1], control[2]))
    for label, build, a, n, inner in (("T106 as written, 10 outer iterations, inner = bicgstab", lambda: ry.case("T106", None)[0], alg, iters, solver.Inner.bicgstab),
                                      ("perturbed 1025^2 block, 1 outer iteration, inner = auto", lambda: configs.single_block(1025, 1025, perturb=0.25), None, 1, solver.Inner.auto)):
        med = {}
        for refine in (False, True):
            secs, inner_its, rep = job_seconds(build, solver.Option.hip(inner=inner, refine=refine), a, n, handles)
            med[refine] = float(np.median(secs))
            lines.append(f"  {label}  {'refined  ' if refine else 'unrefined'}  {spread(secs)}   ({inner_its} inner iterations" +
                         (f"; last iteration {rep['steps'][0]} steps, {rep['correction_iterations']} correction iterations in all)" if rep else ")"))
        lines.append(f"  {label}: refined / unrefined = {med[True] / med[False]:.2f}")
    return lines


def parity(args):
    lines = ["RMS distance of every Picard iterate from the refined exact iteration (oracle assembly, sparse LU with COLAMD refined with a longdouble residual to an "
             "update below one ulp), example inputs as written (tools/refine_timing.py --parity)"]
    for name in ry.EXAMPLES:
        mesh, control, iters = ry.case(name, None)
        want = rr.picard_refined(OracleMesh(mesh), iters, control, "COLAMD")
        other = rr.picard_refined(OracleMesh(mesh), iters, control, "MMD_AT_PLUS_A")
        lines.append(f"  {name}  CPU, MMD_AT_PLUS_A against COLAMD, both refined   " + " ".join(f"{ry.rms(a, b):.1e}" for a, b in zip(want, other)))
        alg = wcf.Algorithm(wcf.White(control[1], control[2]))
        for inner in ("bicgstab", "auto"):
            for refine in (True, False):
                mesh, _, _ = ry.case(name, None)
                d = []
                with smooth.Smoother(mesh, solver.Option.hip(inner=getattr(solver.Inner, inner), refine=refine), alg) as sm:
                    for k in range(iters):
                        sm.iterate(1)
                        sm.download()
                        d.append(ry.rms(mesh_flat(mesh), want[k]))
                lines.append(f"  {name}  device, inner = {inner:8s} {'refined  ' if refine else 'unrefined'}            " + " ".join(f"{x:.1e}" for x in d) +
                             f"   max {max(d):.1e}")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--parity", action="store_true", help="also write profiles/refine_parity.txt")
    ap.add_argument("--skip-timing", action="store_true")
    ap.add_argument("--out-dir", default="profiles")
    args = ap.parse_args()
    oracle.build()
    os.makedirs(args.out_dir, exist_ok=True)
    jobs = ([] if args.skip_timing else [("refine_timing.txt", timing)]) + ([("refine_parity.txt", parity)] if args.parity else [])
    for fname, fn in jobs:
        lines = fn(args)
        print("\n".join(lines))
        with open(os.path.join(args.out_dir, fname), "w") as f:
            f.write("\n".join(lines) + "\n")
        print("wrote", os.path.join(args.out_dir, fname))


if __name__ == "__main__":
    main()
