"""Parity of the reference route (TM_INNER_REFERENCE_GMRES) with the faithful oracle, case by case: per outer iteration the inner counts of
the device (x + y) and of the oracle, the device's RMS distance d_k from the oracle's iterate, and the oracle's distance from itself
self_k(u) for u = 1, 64 and round(sqrt(dof)) ulps (tests/reference_yardstick.py) -- the figures tests/test_gpu_reference_solver.py asserts on.

    python tools/reference_solve_parity.py [--out profiles/reference_solve_parity.txt] [case ...]      (needs the MI355X)"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import oracle  # noqa: E402
from tests import reference_yardstick as ry  # noqa: E402
from tests.conftest import OracleMesh, mesh_flat  # noqa: E402
from tests.meshes import TOPOLOGIES  # noqa: E402
from turbomesh_amd.smoothing import smooth, solver, wall_control_function as wcf  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("cases", nargs="*", default=list(ry.EXAMPLES) + list(TOPOLOGIES))
    ap.add_argument("--out", default=os.path.join("profiles", "reference_solve_parity.txt"))
    args = ap.parse_args()
    oracle.build()
    lines = ["reference route on the device against the faithful oracle: GMRES(30) + ILU(0), rtol 1e-6, atol 1e-8 (tools/reference_solve_parity.py)",
             "bound_k = max(1e-10, 3 self_k(round(sqrt(dof))))", ""]
    for name in args.cases:
        mesh, control, iters = ry.case(name, None)
        ref_mesh, _, _ = ry.case(name)
        dof = sum(b.points.data.shape[0] * b.points.data.shape[1] for b in ref_mesh.blocks)
        base = ry.run(OracleMesh(ref_mesh), iters, oracle.SOLVER_GMRES, oracle.PRECOND_ILU0, control)
        us = [1, 64, ry.ulps_of(dof)]
        selfs = {u: ry.self_distance(ref_mesh, control, iters, u, base=base) for u in us}
        algo = None if control is None else wcf.Algorithm(wcf.White(control[1], control[2]))
        lines.append(f"{name}: dof {dof}, {iters} outer iterations, {'white' if control else 'laplace'}")
        lines.append(f"  {'k':>2} {'device x+y':>12} {'oracle':>7} {'d_k':>10} {'bound_k':>10} " + " ".join(f"{'self_k(' + str(u) + ')':>13}" for u in us) + "   counts under perturbation")
        with smooth.Smoother(mesh, solver.Option.hip(inner=solver.Inner.reference_gmres, preconditioner=solver.Preconditioner.ilu0), algo) as sm:
            for k in range(iters):
                st = sm.iterate(1)
                sm.download()
                cx, cy = sm.inner_counts()
                d_k = ry.rms(mesh_flat(mesh), base[1][k])
                bound = max(ry.PARITY_RMS, ry.FACTOR * selfs[us[-1]][1][k])
                same = all(selfs[u][0][k] == base[0][k] for u in us)
                lines.append(f"  {k:>2} {f'{cx}+{cy}={cx + cy}':>12} {base[0][k]:>7} {d_k:>10.3e} {bound:>10.3e} " + " ".join(f"{selfs[u][1][k]:>13.3e}" for u in us) +
                             f"   {'unchanged' if same else 'CHANGED'}{'' if not st['not_converged'] else '  NOT CONVERGED'}")
        lines.append("")
        print("\n".join(lines[-(iters + 3):]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
