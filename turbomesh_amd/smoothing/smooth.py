"""Mirror of reference src/core/smoothing/smooth.zig: mesh(mesh_data, iterations, solver_option,
control_function_algorithm) -- executed on the MI355X through libtm_hip.so.

`Smoother` is the persistent-handle form (coordinates stay in HBM between calls)."""
from __future__ import annotations

import ctypes as C
import logging

import numpy as np

from .. import _capi
from . import solver as _solver
from . import wall_control_function as _wcf

log = logging.getLogger("smoothing")   # std.log.scoped(.smoothing), smooth.zig:58


def _log_sink(ctx, what, iteration, value):
    """The reference's two per-iteration lines (smooth.zig:105, 136-137) through Python's logging."""
    if what == 0:
        log.info("iteration: %d", iteration)
    elif what == 1:
        log.info("\tresidual: %r", value)
    elif what == 2:   # tm_csr_solve with TM_OPT_REFINE (include/tm_hip.h tm_set_log): steps, last update per component, correction iterations
        log.info("\trefinement steps: %d", int(value))
    elif what in (3, 4):
        log.info("\tlast refinement update |d|/|%s|: %r", "xy"[what - 3], value)
    elif what == 5:
        log.info("\tinner iterations in corrections: %d", int(value))


_LOG_CB = _capi.LOG_FN(_log_sink)   # kept alive for the lifetime of the module


class per_iteration_log:
    """Context manager: route the per-iteration lines of every smoother call inside it to logging ("smoothing" logger).
    Costs one reduction + host round trip per outer iteration (see include/tm_hip.h tm_set_log)."""

    def __init__(self, enable=True):
        self.enable = enable

    def __enter__(self):
        if self.enable:
            _capi.lib().tm_set_log(_LOG_CB, None)
        return self

    def __exit__(self, *exc):
        if self.enable:
            _capi.lib().tm_set_log(_capi.LOG_FN(), None)


def mesh(mesh_data, iterations: int, solver_option: "_solver.Option | None" = None,
         control_function_algorithm: "_wcf.Algorithm | None" = None):
    """smooth.zig:74-166: mutates mesh_data.blocks[b].points.data in place; returns the stats.  Logs like the reference
    ("iteration: n", "\tresidual: r" per outer iteration, then the elapsed time) when the `smoothing` logger is at INFO."""
    opt = (solver_option or _solver.Option.hip()).c_struct()
    cf = (control_function_algorithm or _wcf.Algorithm.laplace()).c_struct()
    md = _capi.MeshDesc(mesh_data)
    st = _capi.tm_stats()
    with per_iteration_log(log.isEnabledFor(logging.INFO)):
        rc = _capi.check(_capi.lib().tm_smooth_mesh(md.ref(), iterations, C.byref(opt), C.byref(cf), C.byref(st)))
    if rc == _capi.TM_W_NOT_CONVERGED:
        log.warning("hip solve did not converge in %d of %d outer iterations", st.not_converged, st.outer_iterations)
    log.info("elapsed time for smoothing: %.2f s", st.seconds)
    return st.as_dict()


class Smoother:
    """tm_smoother_* handle: upload once, iterate on the device, download when needed."""

    def __init__(self, mesh_data, solver_option=None, control_function_algorithm=None, hooks=None, stream=None):
        self._mesh = mesh_data
        self._md = _capi.MeshDesc(mesh_data)
        opt = (solver_option or _solver.Option.hip()).c_struct()
        cf = (control_function_algorithm or _wcf.Algorithm.laplace()).c_struct()
        h = C.c_void_p()
        self._hooks = hooks
        _capi.check(_capi.lib().tm_smoother_create(self._md.ref(), C.byref(opt), C.byref(cf), C.byref(hooks) if hooks is not None else None,
                                                   C.c_void_p(stream) if stream else None, C.byref(h)))
        self._h = h
        self.dof = int(_capi.lib().tm_smoother_dof(self._h))
        self.inner = _solver.Inner(int(_capi.lib().tm_smoother_inner(self._h)))   # what Inner.auto resolved to
        fields = getattr(control_function_algorithm, "fields", None)
        if fields is not None:   # Algorithm.prescribed(fields): the handle starts from a zero field
            try:
                self.set_control_function(fields)
            except Exception:
                self.close()
                raise

    def close(self):
        if getattr(self, "_h", None):
            _capi.lib().tm_smoother_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def iterate(self, iterations: int):
        st = _capi.tm_stats()
        _capi.check(_capi.lib().tm_smoother_iterate(self._h, iterations, C.byref(st)))
        return st.as_dict()

    def inner_counts(self):
        """Inner iterations of the last outer iteration per component, (x, y) (tm_smoother_inner_counts)."""
        x, y = C.c_uint64(0), C.c_uint64(0)
        _capi.check(_capi.lib().tm_smoother_inner_counts(self._h, C.byref(x), C.byref(y)))
        return int(x.value), int(y.value)

    def write(self, filename, with_control_function=True):
        """smooth.zig:396-414 system.write: the coordinates resident on the device (+ P, Q planes)."""
        from .. import output

        output.write_smoother(self, filename, with_control_function)

    def quality(self):
        """(per_block, total) quality records of the coordinates resident in the handle (tm_smoother_quality): reads them only.
        On a handle with rank hooks the records of other ranks' blocks are zero and `total` covers the owned blocks."""
        from .. import quality

        n = len(self._mesh.blocks)
        per_block = (_capi.tm_quality * max(1, n))()
        total = _capi.tm_quality()
        _capi.check(_capi.lib().tm_smoother_quality(self._h, per_block, C.byref(total)))
        return quality.records(per_block[:n], total)

    def quality_field(self, block: int):
        """Per-cell minimum of the oriented scaled Jacobian of an owned block as an (ni-1, nj-1) array indexed [i, j]; NaN where a
        cell is degenerate (tm_smoother_quality_field hands back the plane with i fastest, like the export planes)."""
        ni, nj = self._mesh.blocks[block].points.size
        plane = np.empty((ni - 1) * (nj - 1), dtype=np.float64)
        _capi.check(_capi.lib().tm_smoother_quality_field(self._h, block, _capi.f64ptr(plane)))
        return plane.reshape(nj - 1, ni - 1).T

    def elevate(self, elevation, block: int):
        """(X, Y, HoQuality, sj) of an owned block's curved elements from the coordinates resident in the handle (tm_smoother_elevate):
        `elevation` is a highorder.Elevation; see Elevation.block."""
        return elevation.block(self, block)

    def certify(self, elevation, block: int = None, max_depth: int = 3):
        """The Bezier certificate of an owned block's curved elements (all blocks: block=None) from the coordinates resident in the
        handle (tm_smoother_certify); see Elevation.certify."""
        return elevation.certify(self, block, max_depth=max_depth)

    def weld(self, order=1, boundary=False):
        """weld.UnstructuredMesh of the coordinates resident in the handle: the blocks welded into one conforming mesh of quadrilaterals
        (tm_smoother_weld: map and points formed on the device from the resident coordinates; order > 1: the fine nodes as equidistant
        Lagrange elements, the sizes checked by tm_ho_check).  boundary=True: with .boundary, the faces in patches, oriented by quality()."""
        from .. import weld

        orientation = [q.orientation for q in self.quality()[0]] if boundary else None
        return weld.Weld(self._mesh).mesh(self, order, boundary=boundary, orientation=orientation)

    def weld_boundary(self, order=1, orientation=None):
        """(faces, face_patch, patches) of the boundary of the welded mesh of the coordinates resident in the handle, measured there
        (tm_smoother_weld_boundary: map, welded points, faces and the sums per patch on the device; the welded points are not
        downloaded).  patches: weld.Patch records with measure, normal and moment; orientation None: the rule of quality()."""
        from .. import weld

        return weld.resident_boundary(self, order, orientation)

    def wall_distance(self, kinds=None, cull=True, orientation=None):
        """weld.WallDistance of the welded nodes of the coordinates resident in the handle to the boundary faces whose kind is in `kinds`
        (default wall and unassigned -- the blade of the O4H template), under the periodic translations of the mesh
        (tm_smoother_wall_distance: weld, faces, primitive table and distances on the device; only the outputs cross).  face indexes the
        faces of weld_boundary(1)."""
        from .. import weld

        return weld.resident_wall_distance(self, kinds, cull, orientation)

    def fv_report(self, orientation=None):
        """weld.FvReport of the welded mesh of the coordinates resident in the handle: cells, faces, volumes, closedness, face
        non-orthogonality and skewness (tm_smoother_fv_report: weld, face lists and metrics on the device; only the record crosses).
        orientation None: the rule of quality()."""
        from .. import weld

        return weld.resident_fv_report(self, orientation)

    def write_quality(self, filename):
        """The per-cell planes of every block as a PLOT3D function file (one variable, sizes (ni-1, nj-1))."""
        from .. import output

        sizes, fields = [], []
        for b, blk in enumerate(self._mesh.blocks):
            ni, nj = blk.points.size
            sizes.append((ni - 1, nj - 1))
            fields.append([np.ascontiguousarray(self.quality_field(b).T).reshape(-1)])
        output.write_plot3d_function(filename, sizes, fields)

    def iterate_until(self, scaled_residual_tol: float, max_iterations: int = 1000):
        """Iterate until the scaled nonlinear residual is <= tol.  Returns (reached, stats)."""
        st = _capi.tm_stats()
        rc = _capi.lib().tm_smoother_iterate_until(self._h, max_iterations, C.c_double(scaled_residual_tol), C.byref(st))
        if rc < 0:
            _capi.check(rc)
        return rc == 0, st.as_dict()

    def iterate_until_update(self, update_rms_tol: float, max_iterations: int = 1000):
        """Iterate until the last outer iteration moved the nodes by <= tol RMS (the reference's per-iteration quantity,
        smooth.zig:112-137).  Returns (reached, stats)."""
        st = _capi.tm_stats()
        rc = _capi.lib().tm_smoother_iterate_until_update(self._h, max_iterations, C.c_double(update_rms_tol), C.byref(st))
        if rc < 0:
            _capi.check(rc)
        return rc == 0, st.as_dict()

    def download(self):
        _capi.check(_capi.lib().tm_smoother_download(self._h, self._md.ref()))

    def upload(self):
        _capi.check(_capi.lib().tm_smoother_upload(self._h, self._md.ref()))

    def apply(self, vec, scaled=False):
        """out = A(X) vec (optionally row-equilibrated) for a (dof, 2) host array."""
        vec = np.ascontiguousarray(vec, dtype=np.float64)
        assert vec.shape == (self.dof, 2)
        out = np.empty_like(vec)
        _capi.check(_capi.lib().tm_smoother_apply(self._h, _capi.f64ptr(vec), _capi.f64ptr(out), 1 if scaled else 0))
        return out

    def assemble_csr(self):
        """The reference's assembled system for the current device coordinates (tm_smoother_assemble_csr): (Ap, Ai, Ax_x, Ax_y)."""
        n = C.c_uint64(0)
        _capi.check(_capi.lib().tm_smoother_assemble_csr(self._h, None, None, None, None, 0, C.byref(n)))
        nnz = int(n.value)
        Ap, Ai = np.empty(self.dof + 1, dtype=np.int32), np.empty(nnz, dtype=np.int32)
        Ax, Ay = np.empty(nnz), np.empty(nnz)
        ip = C.POINTER(C.c_int32)
        _capi.check(_capi.lib().tm_smoother_assemble_csr(self._h, Ap.ctypes.data_as(ip), Ai.ctypes.data_as(ip), _capi.f64ptr(Ax), _capi.f64ptr(Ay), nnz, C.byref(n)))
        return Ap, Ai, Ax, Ay

    def apply_reference_order(self, vec):
        """out = A(X) vec through the assembled system, rows summed in CSR order (the reference's mat-vec, bit for bit)."""
        vec = np.ascontiguousarray(vec, dtype=np.float64)
        assert vec.shape == (self.dof, 2)
        out = np.empty_like(vec)
        _capi.check(_capi.lib().tm_smoother_apply_reference_order(self._h, _capi.f64ptr(vec), _capi.f64ptr(out)))
        return out

    def rhs(self):
        out = np.empty((self.dof, 2))
        _capi.check(_capi.lib().tm_smoother_rhs(self._h, _capi.f64ptr(out)))
        return out

    def refine_report(self):
        """What the refinement of a handle created with Option(refine=True) did (tm_smoother_refine_report): steps of the last outer
        iteration, |d| / |x| of its last step per component, inner iterations spent in corrections over the handle's life."""
        steps, rel, its = (C.c_uint32 * 2)(), (C.c_double * 2)(), C.c_uint64(0)
        _capi.check(_capi.lib().tm_smoother_refine_report(self._h, steps, rel, C.byref(its)))
        return {"steps": (int(steps[0]), int(steps[1])), "last_update_rel": (float(rel[0]), float(rel[1])), "correction_iterations": int(its.value)}

    def residual(self, xy=None):
        """b - A(X) xy against the system assembled from the resident coordinates X, in double-double arithmetic rounded once to fp64
        (tm_smoother_residual); xy: (dof, 2) host array, None = the resident coordinates themselves."""
        out = np.empty((self.dof, 2))
        if xy is not None:
            xy = np.ascontiguousarray(xy, dtype=np.float64)
            assert xy.shape == (self.dof, 2)
        _capi.check(_capi.lib().tm_smoother_residual(self._h, None if xy is None else _capi.f64ptr(xy), _capi.f64ptr(out)))
        return out

    def row_kinds(self):
        out = np.empty(self.dof, dtype=np.int32)
        _capi.check(_capi.lib().tm_smoother_row_kinds(self._h, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def profile(self, every=1):
        """Bracket every `every`-th launch of the dominant kernel with a hipEvent pair (0 / False = off)."""
        _capi.check(_capi.lib().tm_smoother_profile(self._h, int(every)))

    def profile_read(self):
        """(milliseconds summed over the bracketed launches, how many were bracketed, launches in total) since the last read."""
        ms = C.c_double(0)
        timed = C.c_uint64(0)
        n = C.c_uint64(0)
        _capi.check(_capi.lib().tm_smoother_profile_read(self._h, C.byref(ms), C.byref(timed), C.byref(n)))
        return ms.value, int(timed.value), int(n.value)

    QUEUE_ORDERING = {-1: "none", 0: "counters", 1: "events (TM_PAIR_SYNC=events)", 2: "events (several multi-rank handles in this process)",
                      3: "events (self-test: both streams on one hardware queue)"}

    def queue_ordering(self):
        """How the handle orders the two queues of a pipelined pass (include/tm_hip_diag.h): code and its meaning."""
        code = int(_capi.lib().tm_smoother_queue_ordering(self._h))
        return code, self.QUEUE_ORDERING.get(code, "?")

    def mg_levels(self, block: int = 0):
        """The multigrid hierarchy and cycle of one block of an Inner.mg_bicgstab handle (tm_smoother_mg_levels): a dict with
        `levels` = [(ni, nj, ci, cj), ...], nu_pre, nu_post, nu_coarsest, omega, dirichlet, perimeter_step, perimeter_sweeps."""
        i32 = C.POINTER(C.c_int32)
        n, omega = C.c_int32(0), C.c_double(0)
        shape, cycle = np.zeros(4 * 32, dtype=np.int32), np.zeros(6, dtype=np.int32)
        _capi.check(_capi.lib().tm_smoother_mg_levels(self._h, block, C.byref(n), shape.ctypes.data_as(i32), 32, cycle.ctypes.data_as(i32), C.byref(omega)))
        return {"levels": [tuple(int(v) for v in shape[4 * l:4 * l + 4]) for l in range(n.value)], "nu_pre": int(cycle[0]), "nu_post": int(cycle[1]),
                "nu_coarsest": int(cycle[2]), "omega": omega.value, "dirichlet": bool(cycle[3]), "perimeter_step": bool(cycle[4]),
                "perimeter_sweeps": int(cycle[5])}

    def precondition_probe(self, f, return_input=False):
        """z = M^-1 f: one application of the multigrid preconditioner for the resident field (tm_smoother_precondition_probe);
        with return_input also the device's input buffer as it stands afterwards."""
        f = np.ascontiguousarray(f, dtype=np.float64)
        assert f.shape == (self.dof, 2)
        z = np.empty_like(f)
        after = np.empty_like(f) if return_input else None
        _capi.check(_capi.lib().tm_smoother_precondition_probe(self._h, _capi.f64ptr(f), _capi.f64ptr(z), _capi.f64ptr(after) if return_input else None))
        return (z, after) if return_input else z

    def control_function(self):
        out = np.empty((self.dof, 2))
        _capi.check(_capi.lib().tm_smoother_control_function(self._h, _capi.f64ptr(out)))
        return out

    def set_control_function(self, fields):
        """Replace the resident (P, Q) field (tm_smoother_set_control_function): one (ni, nj, 2) array per block in block order, or
        the getter's flat (dof, 2) array.  Prescribed and Thomas-Middlecoff handles; on the latter it holds until the next
        update_control_function() or upload()."""
        if isinstance(fields, np.ndarray):
            flat = np.ascontiguousarray(fields, dtype=np.float64)
        else:
            blocks = self._mesh.blocks
            if len(fields) != len(blocks):
                raise ValueError(f"{len(fields)} fields for {len(blocks)} blocks")
            for f, b in zip(fields, blocks):
                if tuple(np.shape(f)) != (b.points.size[0], b.points.size[1], 2):
                    raise ValueError(f"field of shape {np.shape(f)} for a block of {tuple(b.points.size)} nodes")
            flat = np.ascontiguousarray(np.concatenate([np.asarray(f, dtype=np.float64).reshape(-1, 2) for f in fields]))
        if flat.shape != (self.dof, 2):
            raise ValueError(f"the control function has shape {flat.shape}, the handle {self.dof} nodes")
        _capi.check(_capi.lib().tm_smoother_set_control_function(self._h, _capi.f64ptr(flat)))

    def update_control_function(self):
        """Evaluate the Thomas-Middlecoff field again from the coordinates resident now (tm_smoother_update_control_function)."""
        _capi.check(_capi.lib().tm_smoother_update_control_function(self._h))


def plan_rows(mesh_data):
    """Host-only: the perimeter-row table (tm_plan_build) as numpy arrays.  Works without a GPU."""
    md = _capi.MeshDesc(mesh_data, with_coordinates=False)
    rows = _capi.tm_plan_rows()
    _capi.check(_capi.lib().tm_plan_build(md.ref(), C.byref(rows)))
    try:
        n = int(rows.nrows)
        as_np = np.ctypeslib.as_array
        out = {
            "row": as_np(rows.row, (n,)).copy(), "kind": as_np(rows.kind, (n,)).copy(), "ncols": as_np(rows.ncols, (n,)).copy(),
            "cols": as_np(rows.cols, (n * 9,)).reshape(n, 9).copy(), "coef_x": as_np(rows.coef_x, (n * 9,)).reshape(n, 9).copy(),
            "coef_y": as_np(rows.coef_y, (n * 9,)).reshape(n, 9).copy(), "rhs": as_np(rows.rhs, (n * 2,)).reshape(n, 2).copy(),
            "slot": as_np(rows.slot, (n * 9,)).reshape(n, 9).copy(),
        }
    finally:
        _capi.lib().tm_plan_free(C.byref(rows))
    return out
