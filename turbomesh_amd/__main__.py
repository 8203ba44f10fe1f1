"""`python -m turbomesh_amd <config.json>` -- the reference program's batch path (src/gui/main.zig:27-56 without the GUI):
parse the input file (input.zig:25-41), build the geometry, run the blocking template (TFI of every block on the GPU),
smooth, write the mesh.

The example inputs name the reference's own solvers ("gmres" + "ilu0"), which stay on the Zig side: like a reference build
without UMFPACK answers error.ExternalSolverNotEnabled, this program refuses them -- unless --hip replaces the solver entry
by {"hip": {"inner": "auto"}} (what a user would write into the JSON): the plain Picard + BiCGStab solve on meshes of small blocks
like the reference's examples (T106 / LS89: 7x faster there than the multigrid-preconditioned one), the multigrid-preconditioned
solve once a block has 100 000 nodes or more (1000 when the blocks are not coupled) and the cells' aspect ratio does not vary strongly inside any block (refined O-grids with
boundary-layer clustering keep the plain solve).  --hip reference runs the file's own solver AS WRITTEN on the device: GMRES(30) with ILU(0) or the
diagonal on the assembled system, the reference's tolerances -- the iterates a run of the reference gives (solver.Option.as_written)."""
from __future__ import annotations

import argparse
import logging
import os
import sys

from . import input as tm_input
from . import quality
from .smoothing import smooth, solver, wall_control_function


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m turbomesh_amd", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("config", help="input file in the reference's JSON schema (examples/T106/T106.json)")
    ap.add_argument("--hip", nargs="?", const="auto", choices=["auto", "bicgstab", "mg_bicgstab", "gmres", "relax", "file", "reference"],
                    help="use the hip solver with this inner strategy instead of the solver named in the file; `file` = the device counterpart of "
                         "the solver the file names (gmres -> GMRES(30) on the device, bicgstab -> BiCGStab; ilu0 -> diagonal); `reference` = the file's "
                         "solver as written: gmres + ilu0 / diagonal on the assembled system with the reference's tolerances")
    ap.add_argument("--refine", action="store_true",
                    help="refine every inner solve with a double-double residual (up to 3 steps): each Picard iterate is the exact one rounded to fp64; "
                         "with --hip auto, bicgstab, mg_bicgstab, gmres or file, not with relax or reference")
    ap.add_argument("--control", default="file", choices=["file", "laplace", "thomas-middlecoff"],
                    help="control function (P, Q): `file` = smoothing.wall_control_function of the input file (the default), `laplace` = none, "
                         "`thomas-middlecoff` = every block keeps the point distribution of its own edges in its interior (evaluated once from the "
                         "TFI seed on the device, then frozen)")
    ap.add_argument("--iterations", type=int, help="override smoothing.iterations")
    ap.add_argument("--output", help="override the output file (.xyz / .p3d: multi-block PLOT3D)")
    ap.add_argument("--until", type=float, metavar="TOL",
                    help="iterate until the scaled nonlinear residual is <= TOL (at most `iterations`, default 100) instead of a fixed count")
    ap.add_argument("--quality", action="store_true",
                    help="log a mesh quality report (`quality` logger: one line per block and a total) before and after smoothing")
    ap.add_argument("--fail-on-inverted", action="store_true",
                    help="exit non-zero when the smoothed mesh has inverted or degenerate cells (implies the quality evaluation)")
    args = ap.parse_args(argv)
    if args.refine and args.hip in ("relax", "reference"):
        ap.error("--refine goes with --hip auto, bicgstab, mg_bicgstab, gmres or file (relax has no inner solve to refine; reference keeps the reference's stop test)")
    logging.basicConfig(level=logging.INFO, format="%(levelname)s(%(name)s): %(message)s")

    with open(args.config) as f:
        inp = tm_input.Input.parse(f.read())
    if args.hip == "file":
        inp.solver, note = inp.solver.served_by_hip()
        if note:
            logging.getLogger("smoothing").warning(note)
    elif args.hip == "reference":
        inp.solver, note = inp.solver.as_written()
        if note:
            logging.getLogger("smoothing").warning(note)
    elif args.hip:
        inp.solver = solver.Option.hip(inner=getattr(solver.Inner, args.hip))
    if args.refine:
        inp.solver.refine = True
    if args.control == "laplace":
        inp.wall_control_function = wall_control_function.Algorithm.laplace()
    elif args.control == "thomas-middlecoff":
        inp.wall_control_function = wall_control_function.Algorithm.thomas_middlecoff()
    if inp.solver.tag != solver.Tag.hip:
        sys.exit(f"error.ExternalSolverNotEnabled: solver `{inp.solver.tag.name}` is served by the Zig program; "
                 "use \"solver\": {\"hip\": {}} in the input file or pass --hip")
    geometry = inp.geometry(os.getcwd())   # profile files are named relative to the working directory, as in the reference
    mesh = inp.template.run(geometry)                                   # blocking (O4H.zig:67-118) + TFI per block
    iterations = inp.iterations if args.iterations is None else args.iterations
    slog = logging.getLogger("smoothing")
    with smooth.per_iteration_log(slog.isEnabledFor(logging.INFO) and not args.until), smooth.Smoother(mesh, inp.solver, inp.wall_control_function) as sm:
        slog.info("hip solver, inner strategy: %s%s", sm.inner.name, " (chosen from the block sizes and the spread of the cells' aspect ratios)" if inp.solver.inner == solver.Inner.auto else
                  f", preconditioner: {inp.solver.preconditioner.name}" if sm.inner == solver.Inner.reference_gmres else "")
        qlog = logging.getLogger("quality")
        want_quality = args.quality or args.fail_on_inverted
        if want_quality:
            before = sm.quality()
            if args.quality:
                quality.log_report(qlog, mesh.names, *before, "before")
        if args.until:
            reached, stats = sm.iterate_until(args.until, iterations or 100)
            slog.info("scaled residual %.3e after %d iterations (%s)", stats["scaled_residual_rms"], stats["outer_iterations"], "reached" if reached else "NOT reached")
        else:
            stats = sm.iterate(iterations)
            if stats["not_converged"]:
                slog.warning("hip solve did not converge in %d of %d outer iterations", stats["not_converged"], stats["outer_iterations"])
            slog.info("elapsed time for smoothing: %.2f s", stats["seconds"])
        if args.refine:
            rep = sm.refine_report()
            slog.info("refinement: %d steps in the last iteration, last update %.1e / %.1e of the solution, %d inner iterations in corrections",
                      rep["steps"][0], *rep["last_update_rel"], rep["correction_iterations"])
        sm.download()
        stats["inner"] = sm.inner.name
        if want_quality:
            after = sm.quality()
            if args.quality:
                quality.log_report(qlog, mesh.names, *after, "after")
            stats["quality"] = {"before": before, "after": after}
    out = args.output or inp.output
    if out:
        mesh.write(out)
        logging.getLogger("output").info("wrote %s (%d blocks, %d nodes)", out, len(mesh.blocks), sum(b.points.data.shape[0] * b.points.data.shape[1] for b in mesh.blocks))
    if args.fail_on_inverted and not after[1].ok:
        sys.exit(f"mesh quality: {after[1].inverted} inverted and {after[1].degenerate} degenerate cells after smoothing "
                 f"(worst: block {after[1].worst_block}, i {after[1].worst_i}, j {after[1].worst_j})")
    return stats


if __name__ == "__main__":
    main()
