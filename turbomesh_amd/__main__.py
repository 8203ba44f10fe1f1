"""`python -m turbomesh_amd <config.json>` -- the reference program's batch path (src/gui/main.zig:27-56 without the GUI):
parse the input file (input.zig:25-41), build the geometry, run the blocking template (TFI of every block on the GPU),
smooth, write the mesh.

The example inputs name the reference's own solvers ("gmres" + "ilu0"), which stay on the Zig side: like a reference build
without UMFPACK answers error.ExternalSolverNotEnabled, this program refuses them -- unless --hip replaces the solver entry
by {"hip": {"inner": "auto"}} (what a user would write into the JSON): the plain Picard + BiCGStab solve on meshes of small blocks
like the reference's examples (T106 / LS89: 7x faster there than the multigrid-preconditioned one), the multigrid-preconditioned
solve once a block has 100 000 nodes or more (1000 when the blocks are not coupled) and the cells' aspect ratio does not vary strongly inside any block (refined O-grids with
boundary-layer clustering keep the plain solve).  --hip reference runs the file's own solver AS WRITTEN on the device: GMRES(30) with ILU(0) or the
diagonal on the assembled system, the reference's tolerances -- the iterates a run of the reference gives (solver.Option.as_written).

--stack CFG2 [CFG3 ...] --span z0,z1,... --layers NK: `config` and the further files are the spanwise cuts of one blade.  Every file runs the
path above with its own handle; the smoothed cuts are stacked into 3-D blocks on the device (stack.py, include/tm_hip.h "3-D from 2-D cuts")
and --output becomes a multi-block 3-D PLOT3D file; --stack-quality / --fail-on-inverted-3d report on the hexahedra of that mesh
(include/tm_hip.h "3-D quality of stacked blocks").  --stack-mapping revolution --meridional F0 F1 ... places cuts meshed in the unrolled
plane of stream surfaces of revolution (contoured end walls, mixed-flow and radial stages) on their surfaces, one table `u x r` per cut
(include/tm_hip.h "cuts on stream surfaces of revolution").  Without --stack the program is what it was.

--order P [--nodes equidistant|gauss-lobatto]: the smoothed blocks become curved elements of order P (highorder.py, include/tm_hip.h
"high-order elements"): the cell counts of every block and the interface ranges must be multiples of P, which is checked before
anything is smoothed; the elements are formed on the device from the coordinates resident in the handle, their report is logged per block
and for the mesh, and --output takes the elevated nodes (.vtk: Lagrange quadrilaterals, equidistant nodes only; .xyz / .p3d: PLOT3D).
--certify [DEPTH] with --order: the elements are also judged on their WHOLE area by the Bernstein coefficients of their Jacobian, with up
to DEPTH (default 3, at most 4) subdivisions (include/tm_hip.h "high-order elements: certificate"): proven, invalid or undecided per
element, logged per block and for the mesh next to the nodal report; --fail-on-invalid-elements then also counts the elements that
are folded between their nodes, and --fail-on-unproven-elements exits non-zero when any element is not proven.
With --stack, --order P (1 .. 4) turns the stacked blocks into curved hexahedra of order P, in span as in-plane (stack.Stack.elevate,
include/tm_hip.h "high-order hexahedra of stacked blocks"): the cell counts of every block, the interface ranges and --layers minus one
must be multiples of P, checked before anything is smoothed; the elements are formed on the device straight from the resident cuts, their
report is logged per block and for the mesh, and --output takes the elevated nodes (.vtk: Lagrange hexahedra, equidistant nodes only;
.xyz / .p3d: 3-D PLOT3D).  --stack-certify [DEPTH] with --stack --order: the hexahedra are also judged on their WHOLE volume by the
Bernstein coefficients of their Jacobian, with up to DEPTH (default 2, at most 3) octree subdivisions, from the resident cuts (include/tm_hip.h
"high-order hexahedra: certificate"), logged per block and for the mesh; --fail-on-invalid-elements then also counts the hexahedra folded
between their nodes, and --fail-on-unproven-elements exits non-zero when any is not proven.  --certify itself judges 2-D elements and does
not go with --stack.
--weld with --output NAME.vtk (with or without --order, with or without --stack): the blocks are welded into ONE conforming unstructured mesh
(weld.py, include/tm_hip.h "welded unstructured mesh") -- the interface nodes merged, quadrilaterals / hexahedra (Lagrange cells with --order)
over one node numbering -- and NAME.vtk holds that mesh; one line per mesh on the `weld` logger: nodes in -> out, classes by size, periodic
pairs (periodic sides are not glued), max_gap.  Any other output format with --weld is refused.
--boundary with --weld: NAME.boundary.vtk and NAME.boundary.json next to NAME.vtk -- the boundary faces of the welded mesh over the SAME points,
in patches (the conditions of the template, the two sides of every periodic connection with partner and translation, `unassigned` -- where
the O4H template leaves the blade -- and with --stack hub and shroud), one line per patch on the `weld` logger.  The orientation of the
blocks comes from the quality rule (the handle's, with --stack the 3-D report's), so that every normal points out of the mesh.
--wall-distance [KINDS] with --weld: NAME.vtk also holds POINT_DATA wall_distance, the distance of every welded node to the nearest face of
the patches of those kinds (default wall,unassigned; hub,shroud too with --stack), the neighbouring blades seen through the periodic
translations (planar) or the rotation of --blades N (cylindrical, revolution); one line on the `weld` logger.
--polymesh DIR with --weld: an OpenFOAM polyMesh directory of the welded mesh at order 1 (weld.Faces, include/tm_hip.h "faces of the welded
mesh": interior faces with owner and neighbour in upper-triangular order, then the patches; periodic pairs as cyclic patches) -- the stack's
layers with --stack, otherwise one layer between z = 0 and z = --polymesh-thickness with hub and shroud written as `empty`; --fv-report
logs the finite-volume record (volumes, closedness, non-orthogonality, skewness) on the `weld` logger.  --order with --polymesh is an error.
--stack-smooth N with --stack: N sweeps of the 3-D elliptic equations on every stacked block with its faces held (stack.Stack.smooth,
include/tm_hip.h "elliptic smoothing of stacked blocks"), --stack-smooth-algorithm laplace|thomas-middlecoff, --stack-smooth-omega W,
--stack-smooth-tol T; what follows (--weld, --boundary, --wall-distance, --polymesh, --fail-on-inverted-3d) takes the smoothed planes and
--stack-quality logs the report before and after.  It is refused with --order and --stack-certify, which work straight from the cuts.
Without --order nothing changes; without --certify neither does --order; without --weld every output is what it was, and so it is
without --boundary, without --wall-distance, without --polymesh and without --fv-report."""
from __future__ import annotations

import argparse
import contextlib
import logging
import os
import sys

from . import input as tm_input
from . import quality
from .smoothing import smooth, solver, wall_control_function


def _run(ap, args, config, keep=None, tag="", stack=None):
    """One input file through the existing path: parse, block, seed, smooth, download.  keep: an ExitStack that takes the handle over
    (None: it is closed here, as ever); tag: prefix of the quality report's stage names; stack: the stack.Stack this file is a cut of
    (--order then elevates the stacked blocks, not this cut: only the check runs here, before anything is smoothed)."""
    with open(config) as f:
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
    elevation = None
    if getattr(args, "order", None) is not None:
        from . import _capi, highorder

        elevation = highorder.Elevation(args.order, args.nodes)
        try:   # before anything is smoothed
            if stack is None:
                elevation.check(mesh)
            else:
                stack.check_elevation(mesh, elevation)
        except _capi.TmError as e:
            sys.exit(f"high-order elements of order {args.order}: {e}")
    iterations = inp.iterations if args.iterations is None else args.iterations
    slog = logging.getLogger("smoothing")
    with contextlib.ExitStack() as scope:
        scope.enter_context(smooth.per_iteration_log(slog.isEnabledFor(logging.INFO) and not args.until))
        sm = smooth.Smoother(mesh, inp.solver, inp.wall_control_function)
        (keep if keep is not None else scope).enter_context(sm)   # --stack: the handle outlives this call (its coordinates are stacked on the device)
        slog.info("hip solver, inner strategy: %s%s", sm.inner.name, " (chosen from the block sizes and the spread of the cells' aspect ratios)" if inp.solver.inner == solver.Inner.auto else
                  f", preconditioner: {inp.solver.preconditioner.name}" if sm.inner == solver.Inner.reference_gmres else "")
        qlog = logging.getLogger("quality")
        want_quality = args.quality or args.fail_on_inverted
        after = None
        if want_quality:
            before = sm.quality()
            if args.quality:
                quality.log_report(qlog, mesh.names, *before, tag + "before")
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
                quality.log_report(qlog, mesh.names, *after, tag + "after")
            stats["quality"] = {"before": before, "after": after}
        if elevation is not None and stack is None:
            hom = elevation.mesh(sm)   # from the resident coordinates
            quality.log_report_ho(qlog, hom.names, hom.per_block, hom.total, tag + "elevate")
            stats["highorder"] = hom
            if getattr(args, "certify", None) is not None:
                total, per_block, _, _ = elevation.certify(sm, max_depth=args.certify)   # from the resident coordinates
                quality.log_report_ho_certificate(qlog, hom.names, per_block, total, tag + "certify")
                stats["certificate"] = {"per_block": per_block, "total": total}
        if getattr(args, "weld", False) and stack is None:   # while the handle lives: the linear mesh comes from the resident coordinates
            from . import weld

            want_boundary = getattr(args, "boundary", False)
            if elevation is not None:   # the orientation by the quality rule, from the handle
                welded = stats["highorder"].weld(mesh, boundary=want_boundary, orientation=[q.orientation for q in sm.quality()[0]] if want_boundary else None)
            else:
                welded = sm.weld(boundary=want_boundary)
            weld.log_report(logging.getLogger("weld"), welded.info, tag + os.path.basename(config))
            if want_boundary:
                weld.log_boundary(logging.getLogger("weld"), welded.boundary, tag + os.path.basename(config))
            if getattr(args, "wall_distance", None) is not None:   # of the fine welded nodes, which the element nodes of an equidistant elevation are
                welded.wall_distance = sm.wall_distance(args.wall_kinds)
                weld.log_wall_distance(logging.getLogger("weld"), welded.wall_distance, tag + os.path.basename(config))
            if getattr(args, "fv_report", False):   # of the plane cells, from the resident coordinates
                stats["fv_report"] = sm.fv_report()
                weld.log_fv_report(logging.getLogger("weld"), stats["fv_report"], tag + os.path.basename(config))
            if getattr(args, "polymesh", None):   # one layer of hexahedra over the plane mesh, z = 0 and z = T: the planar-layer path
                import numpy as np

                faces = weld.Weld(mesh).faces(layers=2, orientation=[q.orientation for q in sm.quality()[0]])
                xy = welded.points[:, :2]
                stats["polymesh"] = (np.vstack([np.column_stack([xy, np.full(len(xy), z)]) for z in (0.0, args.polymesh_thickness)]), faces)
            stats["welded"] = welded
    return inp, mesh, sm, stats, after


def _span_clustering(ap, text):
    from . import clustering

    kind, _, rest = text.partition(":")
    try:
        vals = [float(v) for v in rest.split(",")] if rest else []
        if kind == "uniform" and not vals:
            return clustering.Uniform()
        if kind == "roberts" and len(vals) == 2:
            return clustering.Roberts(*vals)
        if kind == "tanh" and len(vals) == 1:
            return clustering.SingleHyperbolicClustering(*vals)
    except ValueError:
        pass
    ap.error(f"--span-clustering {text!r}: uniform, roberts:alpha,beta or tanh:delta_s")


def _main_stack(ap, args):
    """config + --stack files: every cut through _run with its own handle (kept alive), then the 3-D file block by block from the
    coordinates resident in the handles (tm_stack_smoothers)."""
    from . import output, stack

    vtk = (args.order is not None or args.weld) and args.output.lower().endswith(".vtk")
    if not vtk:
        output._format_of(args.output)
    surfaces = None
    if args.stack_mapping == "revolution":
        try:
            surfaces = stack.Surfaces.read(args.meridional, args.reference_radius_values, args.meridional_interpolation)
        except (OSError, ValueError) as e:
            ap.error(f"--meridional: {e}")
    st = stack.Stack(args.span_values, stack.layers_from(args.span_values, args.layers, args.span_clustering_fn), args.stack_interpolation, args.stack_mapping,
                     surfaces=surfaces)
    st.weights()   # a span that is not increasing (or a radius <= 0) is refused before anything is smoothed
    if surfaces is not None:
        st.surface_tables()   # and so are meridional tables the definition does not admit
    files = [args.config] + list(args.stack)
    all_stats, worst = [], None
    with contextlib.ExitStack() as keep:
        handles = []
        for c, config in enumerate(files):
            _, mesh, sm, stats, after = _run(ap, args, config, keep=keep, tag=f"cut {c} ", stack=st)
            handles.append(sm)
            all_stats.append(stats)
            if after is not None and not after[1].ok and worst is None:
                worst = (c, after[1])
        hom = cert = None
        if args.order is not None:   # curved hexahedra straight from the resident cuts: the fine 3-D block is never formed
            from . import highorder

            hom = m3 = st.mesh3d_ho(handles, highorder.Elevation(args.order, args.nodes))
            quality.log_report_ho3(logging.getLogger("quality"), hom.names, hom.per_block, hom.total)
            for b, outside in enumerate(hom.outside):
                for c, n in enumerate(outside):
                    if n:
                        logging.getLogger("stack").warning("block %d (%s), cut %d: %d nodes lie outside the meridional table %s and are extrapolated", b, hom.names[b],
                                                           c, int(n), args.meridional[c])
            if args.stack_certify is not None:   # from the resident cuts as well
                ctotal, cper, _, _ = st.certify(handles, highorder.Elevation(args.order, args.nodes), max_depth=args.stack_certify)
                quality.log_report_ho3_certificate(logging.getLogger("quality"), hom.names, cper, ctotal)
                cert = {"per_block": cper, "total": ctotal}
        elif surfaces is None:
            m3 = st.mesh3d(handles)
        else:   # the same blocks, with the count of extrapolated nodes per cut
            m3 = stack.Mesh3d()
            for b, name in enumerate(handles[0]._mesh.names):
                *planes, outside = st.block(handles, b, return_outside=True)
                m3.names.append(name)
                m3.blocks.append(tuple(planes))
                for c, n in enumerate(outside):
                    if n:
                        logging.getLogger("stack").warning("block %d (%s), cut %d: %d nodes lie outside the meridional table %s and are extrapolated", b, name, c,
                                                           int(n), args.meridional[c])
        q3 = st.quality(handles) if (args.stack_quality or args.fail_on_inverted_3d or args.boundary or args.polymesh or args.fv_report) else None   # from the resident cuts: no 3-D block is formed
        smoothed = bool(args.stack_smooth)
        if smoothed:   # every block stacked again into a device buffer and smoothed there with its faces held (tm_stack_smoothers_smooth)
            records = []
            for b in range(len(m3.blocks)):
                *planes, rec = st.smooth(handles, b, args.stack_smooth, args.stack_smooth_algorithm, args.stack_smooth_omega, args.stack_smooth_tol)
                m3.blocks[b] = tuple(planes)
                records.append(rec)
            stack.log_smooth3d(logging.getLogger("stack"), m3.names, records)
            if q3 is not None:   # what follows judges and orients the smoothed planes
                if args.stack_quality:
                    quality.log_report_3d(logging.getLogger("quality"), m3.names, *q3)
                per_block = [stack.quality_of_planes(*planes, block=b) for b, planes in enumerate(m3.blocks)]
                q3 = (per_block, quality.total_3d(per_block))
    if args.weld:   # sizes and connections are those of any cut
        from . import weld

        welded = weld.Weld(mesh).mesh(m3, args.order or 1, args.nodes or "equidistant", boundary=args.boundary,
                                      orientation=[q.orientation for q in q3[0]] if args.boundary else None)   # the 3-D report's orientation
        weld.log_report(logging.getLogger("weld"), welded.info, "stacked mesh")
        if args.wall_distance is not None:
            images = None   # planar: the periodic translations of the plan
            if args.stack_mapping != "planar":
                import math

                images = weld.rotation_images(2.0 * math.pi / args.blades)[:3 if args.blades else 1] if args.blades else weld.rotation_images(0.0)[:1]
                if not args.blades:
                    logging.getLogger("weld").warning("--wall-distance on a %s stack without --blades N: no periodic images, the neighbouring blades are not seen",
                                                      args.stack_mapping)
            welded.wall_distance = weld.Weld(mesh).wall_distance(welded.points, kinds=args.wall_kinds, images=images)
            weld.log_wall_distance(logging.getLogger("weld"), welded.wall_distance, "stacked mesh")
        welded.write(args.output)
        if args.polymesh or args.fv_report:   # the layers are the stack's; the orientation is the 3-D report's
            faces = weld.Weld(mesh).faces(layers=len(welded.points) // max(1, welded.info.nodes_out), orientation=[q.orientation for q in q3[0]])
            if args.fv_report:
                weld.log_fv_report(logging.getLogger("weld"), faces.metrics(welded.points), "stacked mesh")
            if args.polymesh:
                output.write_polymesh(args.polymesh, welded.points, faces)
                logging.getLogger("output").info("wrote the polyMesh directory %s (%d cells, %d faces)", args.polymesh, faces.ncells, len(faces.faces))
        if args.boundary:
            weld.log_boundary(logging.getLogger("weld"), welded.boundary, "stacked mesh")
            logging.getLogger("output").info("wrote %s and %s", *welded.write_boundary(args.output))
    else:
        m3.write(args.output)
    logging.getLogger("output").info("wrote %s (%d blocks, %d cuts, %d layers, %d nodes)", args.output, len(m3.blocks), len(files), st.nlayers,
                                     len(welded.points) if args.weld else sum(x.size for x, _, _ in m3.blocks))
    if hom is not None:
        logging.getLogger("output").info("%d hexahedra of order %d, %s nodes", hom.total.elements, hom.order, hom.distribution)
    if q3 is not None and args.stack_quality:
        quality.log_report_3d(logging.getLogger("quality"), m3.names, *q3, stage="stack-smooth" if smoothed else "stack")
    if args.fail_on_inverted and worst is not None:
        sys.exit(f"mesh quality: cut {worst[0]} has {worst[1].inverted} inverted and {worst[1].degenerate} degenerate cells after smoothing")
    if args.fail_on_invalid_elements and not hom.total.ok:
        b, bad = next((b, q) for b, q in enumerate(hom.per_block) if not q.ok)
        sys.exit(f"high-order elements: {hom.total.invalid} invalid hexahedra of order {hom.order} in the stacked mesh "
                 f"(first in block {b}: {bad.invalid} of {bad.elements})")
    if args.fail_on_invalid_elements and cert is not None and cert["total"].hidden_invalid:
        sys.exit(f"high-order elements: {cert['total'].hidden_invalid} hexahedra of order {hom.order} are valid at their nodes and folded between them "
                 f"({cert['total'].invalid} invalid by the certificate)")
    if args.fail_on_unproven_elements and not cert["total"].ok:
        t = cert["total"]
        sys.exit(f"high-order elements: {t.elements - t.proven} of {t.elements} hexahedra of order {hom.order} are not proven valid ({t.invalid} invalid, "
                 f"{t.undecided} undecided at depth {t.max_depth}; first: block {t.first_unproven_block}, e {t.first_unproven_e}, f {t.first_unproven_f}, "
                 f"g {t.first_unproven_g})")
    if args.fail_on_inverted_3d and not q3[1].ok:
        b, bad = next((b, q) for b, q in enumerate(q3[0]) if not q.ok)
        sys.exit(f"mesh quality: the stacked mesh has {q3[1].inverted} inverted and {q3[1].degenerate} degenerate hexahedra "
                 f"(block {b}: {bad.inverted} inverted, {bad.degenerate} degenerate, worst cell i {bad.worst_i}, j {bad.worst_j}, k {bad.worst_k})")
    out = {"cuts": all_stats, "blocks": len(m3.blocks), "layers": st.nlayers}
    if hom is not None:
        out["highorder"] = hom
    if cert is not None:
        out["certificate"] = cert
    if q3 is not None:
        out["quality3d"] = {"per_block": q3[0], "total": q3[1]}
    return out


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
    ap.add_argument("--order", type=int, metavar="P",
                    help="curved elements of order P (1 .. 8) from the smoothed blocks: every P x P group of cells is one element; the cell counts "
                         "of every block and the interface ranges must be multiples of P (checked before smoothing).  --output then takes the "
                         "elevated nodes: .vtk (Lagrange quadrilaterals, --nodes equidistant) or PLOT3D.  With --stack: curved hexahedra of order "
                         "P (1 .. 4) from the stacked blocks, --layers minus one a multiple of P as well; .vtk holds Lagrange hexahedra")
    ap.add_argument("--nodes", default=None, choices=["equidistant", "gauss-lobatto"],
                    help="with --order: node distribution inside the elements (default: gauss-lobatto; equidistant for a .vtk output)")
    ap.add_argument("--fail-on-invalid-elements", action="store_true",
                    help="with --order: exit non-zero, after the file is written, when elements with a non-positive Jacobian at a node remain")
    ap.add_argument("--certify", nargs="?", type=int, const=3, default=None, metavar="DEPTH",
                    help="with --order: certify every element on its whole area by the Bernstein coefficients of its Jacobian with up to DEPTH "
                         "(0 .. 4, default 3) subdivisions; logged per block and for the mesh; --fail-on-invalid-elements then counts the "
                         "elements folded between their nodes too")
    ap.add_argument("--stack-certify", nargs="?", type=int, const=2, default=None, metavar="DEPTH",
                    help="with --stack --order: the 3-D certificate -- certify every curved hexahedron on its whole volume by the Bernstein "
                         "coefficients of its Jacobian with up to DEPTH (0 .. 3, default 2) octree subdivisions, from the resident cuts; logged per "
                         "block and for the mesh; --fail-on-invalid-elements then counts the hexahedra folded between their nodes too")
    ap.add_argument("--fail-on-unproven-elements", action="store_true",
                    help="with --certify or --stack-certify: exit non-zero, after the file is written, when any element is not proven valid (invalid or undecided)")
    ap.add_argument("--stack", nargs="+", metavar="CFG", default=None,
                    help="further input files: the spanwise cuts after `config`, in span order.  Every file runs the path above with its own "
                         "handle; the smoothed cuts are then stacked into 3-D blocks on the device and --output becomes a multi-block 3-D PLOT3D file")
    ap.add_argument("--span", metavar="Z0,Z1,...", help="span coordinate of every cut (radius with --stack-mapping cylindrical), strictly increasing; one per file")
    ap.add_argument("--layers", type=int, metavar="NK", help="number of layers of the 3-D blocks, first and last at the end cuts")
    ap.add_argument("--span-clustering", default="uniform", metavar="uniform|roberts:a,b|tanh:d",
                    help="distribution of the layers over the span (clustering.zig: Uniform, Roberts alpha,beta, SingleHyperbolicClustering delta_s)")
    ap.add_argument("--stack-interpolation", default="cubic", choices=["linear", "cubic"], help="between the cuts: linear, or the natural cubic spline")
    ap.add_argument("--stack-mapping", default="planar", choices=["planar", "cylindrical", "revolution"],
                    help="planar: (x, y, s); cylindrical: the cuts are unrolled cylinders (x, r theta) at radius span, output (x, r sin theta, r cos theta); "
                         "revolution: the cuts are unrolled stream surfaces of revolution (u, rref theta) with the meridional curves of --meridional")
    ap.add_argument("--meridional", nargs="+", metavar="FILE", default=None,
                    help="with --stack-mapping revolution: one text file per cut, rows `u x r` (# comments), the meridional curve x(u), r(u) of its surface")
    ap.add_argument("--meridional-interpolation", default=None, choices=["linear", "cubic"], help="of x(u) and r(u) between the rows of a table (default cubic)")
    ap.add_argument("--reference-radius", metavar="R0,R1,...", default=None, help="reference radius of every cut, v = rref theta (default: --span)")
    ap.add_argument("--stack-quality", action="store_true",
                    help="with --stack: log the 3-D quality report of the stacked blocks (`quality` logger: one line per block and a total) -- "
                         "negative and degenerate hexahedra across layers, which --quality (every cut alone) cannot see")
    ap.add_argument("--fail-on-inverted-3d", action="store_true",
                    help="with --stack: exit non-zero, after the file is written, when the stacked mesh has inverted or degenerate hexahedra "
                         "(implies the 3-D quality evaluation)")
    ap.add_argument("--stack-smooth", type=int, default=None, metavar="N",
                    help="with --stack: N Jacobi sweeps of the 3-D elliptic (Winslow) equations on every stacked block, its six faces held, before "
                         "the file is written; --weld, --boundary, --wall-distance and --polymesh take the smoothed planes, --stack-quality logs the "
                         "report before and after, --fail-on-inverted-3d judges the one after; one line per block on the `stack` logger")
    ap.add_argument("--stack-smooth-algorithm", default=None, choices=["laplace", "thomas-middlecoff"],
                    help="with --stack-smooth: plain Laplace, or the Thomas-Middlecoff control field that keeps wall clustering (default)")
    ap.add_argument("--stack-smooth-omega", type=float, default=None, metavar="W", help="with --stack-smooth: relaxation factor, 0 < W <= 1 (default 1)")
    ap.add_argument("--stack-smooth-tol", type=float, default=None, metavar="T",
                    help="with --stack-smooth: stop once the rms update of a sweep is <= T (tested behind every 8th sweep; default 0: all N sweeps)")
    ap.add_argument("--weld", action="store_true",
                    help="with --output NAME.vtk: weld the blocks into one conforming unstructured mesh (interface nodes merged; quadrilaterals, "
                         "hexahedra with --stack, Lagrange cells with --order) and write that; logs node counts, classes and max_gap on the `weld` logger")
    ap.add_argument("--boundary", action="store_true",
                    help="with --weld: also the boundary of the welded mesh -- NAME.boundary.vtk (the faces over the volume file's points, CELL_DATA patch and "
                         "kind) and NAME.boundary.json (the patch table: conditions, periodic sides with partner and translation, unassigned, hub and shroud "
                         "with --stack) next to --output; one line per patch on the `weld` logger")
    ap.add_argument("--wall-distance", nargs="?", const="", default=None, metavar="KINDS",
                    help="with --weld: the distance of every welded node to the nearest wall face as POINT_DATA wall_distance of NAME.vtk; KINDS: "
                         "comma-separated patch kinds that count as wall (default wall,unassigned -- the blade of the O4H template -- and with --stack "
                         "hub,shroud as well).  The nearest wall may be the neighbouring blade: planar meshes use the periodic translations of the "
                         "input, cylindrical and revolution stacks the rotation by 2 pi / N of --blades N.  With --order the distances are those of "
                         "the fine welded nodes, which the equidistant element nodes are; one line on the `weld` logger")
    ap.add_argument("--polymesh", metavar="DIR", default=None,
                    help="with --weld: also an OpenFOAM polyMesh directory DIR (ASCII points, faces, owner, neighbour, boundary) of the welded mesh at "
                         "order 1: with --stack the stacked hexahedra, otherwise the plane mesh extruded by one layer (hub and shroud written as empty)")
    ap.add_argument("--polymesh-thickness", type=float, default=1.0, metavar="T", help="with --polymesh and no --stack: the layer lies between z = 0 and z = T (default 1)")
    ap.add_argument("--fv-report", action="store_true",
                    help="with --weld: log the finite-volume record of the welded mesh on the `weld` logger -- cells and faces, volumes, cells with "
                         "V <= 0, closedness, face non-orthogonality and skewness")
    ap.add_argument("--blades", type=int, default=None, metavar="N", help="with --wall-distance and --stack-mapping cylindrical|revolution: the blade count of the row")
    args = ap.parse_args(argv)
    if args.wall_distance is not None:
        if not args.weld:
            ap.error("--wall-distance is a field of the welded mesh: it goes with --weld and --output NAME.vtk")
        if args.order is not None and args.nodes not in (None, "equidistant"):
            ap.error("wall distance is defined on the fine mesh: --nodes equidistant with --wall-distance")
        from . import weld as _weld

        args.wall_kinds = [k.strip() for k in args.wall_distance.split(",") if k.strip()] or None   # None: the default kinds
        try:
            _weld.kinds_mask(args.wall_kinds or ())
        except ValueError as e:
            ap.error(f"--wall-distance: {e}")
    if args.blades is not None and (args.wall_distance is None or args.blades < 1):
        ap.error("--blades N >= 1 goes with --wall-distance")
    if args.weld and not (args.output and args.output.lower().endswith(".vtk")):
        ap.error(f"--weld writes one welded unstructured mesh as legacy VTK: --output NAME.vtk, not {args.output!r}")
    if (args.polymesh or args.fv_report) and not args.weld:
        ap.error("--polymesh and --fv-report are views of the welded mesh: they go with --weld and --output NAME.vtk")
    if args.polymesh and args.order is not None:
        ap.error("--polymesh writes the fine cells (order 1): it does not go with --order")
    if args.polymesh and not args.polymesh_thickness > 0:
        ap.error("--polymesh-thickness: a positive number")
    if args.boundary and not args.weld:
        ap.error("--boundary lists the boundary faces of the welded mesh: it goes with --weld and --output NAME.vtk")
    if args.stack is None and (args.span or args.layers is not None):
        ap.error("--span and --layers go with --stack")
    if args.stack is None and (args.meridional or args.reference_radius or args.meridional_interpolation):
        ap.error("--meridional, --meridional-interpolation and --reference-radius go with --stack")
    if args.stack is None and (args.stack_quality or args.fail_on_inverted_3d):
        ap.error("--stack-quality and --fail-on-inverted-3d go with --stack")
    if args.stack_smooth is None and (args.stack_smooth_algorithm or args.stack_smooth_omega is not None or args.stack_smooth_tol is not None):
        ap.error("--stack-smooth-algorithm, --stack-smooth-omega and --stack-smooth-tol go with --stack-smooth N")
    if args.stack_smooth is not None:
        if args.stack is None:
            ap.error("--stack-smooth goes with --stack")
        if args.order is not None or args.stack_certify is not None:
            ap.error("--stack-smooth does not go with --order or --stack-certify: curved hexahedra and their certificate are formed straight from the cuts, "
                     "not from a stored block")
        if args.stack_smooth < 1:
            ap.error("--stack-smooth N: at least 1 sweep")
        args.stack_smooth_algorithm = args.stack_smooth_algorithm or "thomas-middlecoff"
        args.stack_smooth_omega = 1.0 if args.stack_smooth_omega is None else args.stack_smooth_omega
        args.stack_smooth_tol = 0.0 if args.stack_smooth_tol is None else args.stack_smooth_tol
        if not 0.0 < args.stack_smooth_omega <= 1.0:
            ap.error("--stack-smooth-omega: 0 < W <= 1")
        if not args.stack_smooth_tol >= 0.0:
            ap.error("--stack-smooth-tol: T >= 0")
    if args.order is None and (args.nodes or args.fail_on_invalid_elements):
        ap.error("--nodes and --fail-on-invalid-elements go with --order")
    if args.certify is None and args.stack_certify is None and args.fail_on_unproven_elements:
        ap.error("--fail-on-unproven-elements goes with --certify or --stack-certify")
    if args.stack_certify is not None:
        if args.stack is None or args.order is None:
            ap.error("--stack-certify goes with --stack and --order")
        if not 0 <= args.stack_certify <= 3:
            ap.error("--stack-certify: 0 .. 3")
    if args.certify is not None:
        if args.order is None:
            ap.error("--certify goes with --order")
        if not 0 <= args.certify <= 4:
            ap.error("--certify: 0 .. 4")
    if args.order is not None:
        if args.stack is not None and args.certify is not None:
            ap.error("--certify judges 2-D elements: a 3-D certificate is not built, so it does not go with --stack")
        if not 1 <= args.order <= (8 if args.stack is None else 4):
            ap.error("--order: 1 .. 8" if args.stack is None else "--order: 1 .. 4 with --stack (curved hexahedra)")
        vtk = bool(args.output) and args.output.lower().endswith(".vtk")
        if args.nodes is None:
            args.nodes = "equidistant" if vtk else "gauss-lobatto"
        if vtk and args.nodes != "equidistant":
            ap.error("a .vtk output holds Lagrange cells, which assume equidistant nodes: --nodes equidistant, or a PLOT3D output")
    if args.stack is not None:
        if not args.span or args.layers is None:
            ap.error("--stack needs --span z0,z1,... and --layers NK")
        try:
            args.span_values = [float(v) for v in args.span.split(",")]
        except ValueError:
            ap.error(f"--span {args.span!r}: comma-separated numbers")
        if len(args.span_values) != 1 + len(args.stack):
            ap.error(f"--span has {len(args.span_values)} values for {1 + len(args.stack)} files (config + --stack)")
        if args.layers < 1:
            ap.error("--layers: at least 1")
        args.span_clustering_fn = _span_clustering(ap, args.span_clustering)
        if not args.output:
            ap.error("--stack needs --output (the 3-D file)")
        args.reference_radius_values = None
        if args.stack_mapping == "revolution":
            if not args.meridional:
                ap.error("--stack-mapping revolution needs --meridional F0 F1 ... (one table per cut)")
            if len(args.meridional) != len(args.span_values):
                ap.error(f"--meridional has {len(args.meridional)} files for {len(args.span_values)} cuts (config + --stack)")
            if args.reference_radius:
                try:
                    args.reference_radius_values = [float(v) for v in args.reference_radius.split(",")]
                except ValueError:
                    ap.error(f"--reference-radius {args.reference_radius!r}: comma-separated numbers")
                if len(args.reference_radius_values) != len(args.span_values):
                    ap.error(f"--reference-radius has {len(args.reference_radius_values)} values for {len(args.span_values)} cuts")
            args.meridional_interpolation = args.meridional_interpolation or "cubic"
        else:
            for flag, given in (("--meridional", args.meridional), ("--reference-radius", args.reference_radius),
                                ("--meridional-interpolation", args.meridional_interpolation)):
                if given:
                    ap.error(f"{flag} goes with --stack-mapping revolution")
    if args.refine and args.hip in ("relax", "reference"):
        ap.error("--refine goes with --hip auto, bicgstab, mg_bicgstab, gmres or file (relax has no inner solve to refine; reference keeps the reference's stop test)")
    logging.basicConfig(level=logging.INFO, format="%(levelname)s(%(name)s): %(message)s")

    if args.stack is not None:
        return _main_stack(ap, args)
    inp, mesh, _, stats, after = _run(ap, args, args.config)
    out = args.output or inp.output
    hom = stats.get("highorder")
    if args.weld:
        welded = stats["welded"]
        welded.write(out)
        logging.getLogger("output").info("wrote %s (%d welded nodes, %d cells of type %d)", out, len(welded.points), len(welded.cells), welded.cell_type)
        if args.boundary:
            logging.getLogger("output").info("wrote %s and %s", *welded.write_boundary(out))
        if args.polymesh:
            from . import output

            pts3, faces = stats["polymesh"]
            output.write_polymesh(args.polymesh, pts3, faces, empty_caps=True)
            logging.getLogger("output").info("wrote the polyMesh directory %s (%d cells, %d faces)", args.polymesh, faces.ncells, len(faces.faces))
    elif out and hom is not None:
        hom.write(out)
        logging.getLogger("output").info("wrote %s (%d blocks, %d elements of order %d, %s nodes)", out, len(hom.blocks), hom.total.elements, hom.order, hom.distribution)
    elif out:
        mesh.write(out)
        logging.getLogger("output").info("wrote %s (%d blocks, %d nodes)", out, len(mesh.blocks), sum(b.points.data.shape[0] * b.points.data.shape[1] for b in mesh.blocks))
    cert = stats.get("certificate")
    if args.fail_on_invalid_elements and hom.total.ok and cert is not None and cert["total"].hidden_invalid:
        sys.exit(f"high-order elements: {cert['total'].hidden_invalid} elements of order {hom.order} are valid at their nodes and folded between them "
                 f"({cert['total'].invalid} invalid by the certificate)")
    if args.fail_on_invalid_elements and not hom.total.ok:
        bad = next(q for q in hom.per_block if not q.ok)
        sys.exit(f"high-order elements: {hom.total.invalid} invalid elements of order {hom.order} after smoothing "
                 f"(first in block {hom.per_block.index(bad)}: {bad.invalid} of {bad.elements})")
    if args.fail_on_unproven_elements and not cert["total"].ok:
        t = cert["total"]
        sys.exit(f"high-order elements: {t.elements - t.proven} of {t.elements} elements of order {hom.order} are not proven valid ({t.invalid} invalid, "
                 f"{t.undecided} undecided at depth {t.max_depth}; first: block {t.first_unproven_block}, e {t.first_unproven_e}, f {t.first_unproven_f})")
    if args.fail_on_inverted and not after[1].ok:
        sys.exit(f"mesh quality: {after[1].inverted} inverted and {after[1].degenerate} degenerate cells after smoothing "
                 f"(worst: block {after[1].worst_block}, i {after[1].worst_i}, j {after[1].worst_j})")
    return stats


if __name__ == "__main__":
    main()
