"""ctypes binding of libtm_hip.so (include/tm_hip.h) -- the drop-in C-ABI boundary.

The product path has NO CPU fallback: if the shared library is missing, or no gfx950 device
is present, calls raise TmError / OSError.  Only `plan_build` (host-side planning) works
without a GPU.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TM_HIP_LIB") or os.path.join(_HERE, "libtm_hip.so")   # TM_HIP_LIB: experiment builds only
DBG_LIB_PATH = os.path.join(_HERE, "libtm_hip_dbg.so")   # the same library + the tm_debug_* / tm_tune_* / tm_diag_* helpers of tools/

# tm_error
TM_OK, TM_W_NOT_CONVERGED = 0, 1
TM_E_SIZE, TM_E_TOPOLOGY, TM_E_MISMATCH, TM_E_OVERFLOW, TM_E_UNSUPPORTED, TM_E_ARG, TM_E_MEMORY, TM_E_HIP, TM_E_COMM = -1, -2, -3, -4, -5, -6, -7, -8, -9
_ERR_NAMES = {-1: "InconsistentSize", -2: "Topology", -3: "Mismatch", -4: "Overflow", -5: "ExternalSolverNotEnabled", -6: "Argument",
              -7: "OutOfMemory", -8: "Hip", -9: "Comm"}
TM_SOLVER_GMRES, TM_SOLVER_BICGSTAB, TM_SOLVER_UMFPACK, TM_SOLVER_PETSC, TM_SOLVER_HIP = 0, 1, 2, 3, 4
TM_INNER_BICGSTAB, TM_INNER_RELAX, TM_INNER_MG_BICGSTAB, TM_INNER_AUTO, TM_INNER_GMRES, TM_INNER_REFERENCE_GMRES = 0, 1, 2, 3, 4, 5
TM_CF_LAPLACE, TM_CF_WHITE, TM_CF_PRESCRIBED, TM_CF_THOMAS_MIDDLECOFF = 0, 1, 2, 3
TM_OPT_REFINE = 16
TM_STACK_MAX_CUTS = 16
TM_STACK_LINEAR, TM_STACK_CUBIC = 0, 1
TM_STACK_PLANAR, TM_STACK_CYLINDRICAL, TM_STACK_REVOLUTION = 0, 1, 2
TM_STACK_MAX_KNOTS = 256
TM_SURF_LINEAR, TM_SURF_CUBIC = 0, 1
TM_HO_MAX_ORDER = 8
TM_HO_EQUIDISTANT, TM_HO_GAUSS_LOBATTO, TM_HO_PRESCRIBED = 0, 1, 2
TM_HO_CERT_MAX_DEPTH = 4
TM_HO3_MAX_ORDER = 4
TM_HO3_CERT_MAX_DEPTH = 3
TM_HO_PROVEN, TM_HO_INVALID, TM_HO_UNDECIDED = 0, 1, 2
TM_BC_WALL, TM_BC_INLET, TM_BC_OUTLET = 0, 1, 2
TM_PATCH_PERIODIC, TM_PATCH_UNASSIGNED, TM_PATCH_HUB, TM_PATCH_SHROUD = 16, 17, 18, 19


class TmError(RuntimeError):
    """A negative tm_error code mapped to a Python error (the Zig side maps it to an error union)."""

    def __init__(self, code, msg):
        super().__init__(f"error.{_ERR_NAMES.get(code, 'Unknown')} ({code}): {msg}")
        self.code = code
        self.name = _ERR_NAMES.get(code, "Unknown")


class tm_range(C.Structure):
    _fields_ = [("block", C.c_uint64), ("side", C.c_uint32), ("_pad", C.c_uint32), ("start", C.c_uint64), ("end", C.c_uint64)]


class tm_connection(C.Structure):
    _fields_ = [("r", tm_range * 2), ("has_periodicity", C.c_int32), ("_pad", C.c_int32), ("periodicity", C.c_double * 2)]


class tm_condition(C.Structure):
    _fields_ = [("range", tm_range), ("kind", C.c_uint32), ("_pad", C.c_uint32)]


class tm_block(C.Structure):
    _fields_ = [("xy", C.POINTER(C.c_double)), ("ni", C.c_uint64), ("nj", C.c_uint64)]


class tm_mesh_desc(C.Structure):
    _fields_ = [("blocks", C.POINTER(tm_block)), ("nblocks", C.c_uint64), ("conns", C.POINTER(tm_connection)), ("nconns", C.c_uint64),
                ("bcs", C.POINTER(tm_condition)), ("nbcs", C.c_uint64)]


class tm_control_fn(C.Structure):
    _fields_ = [("kind", C.c_int32), ("_pad", C.c_int32), ("ds_target", C.c_double), ("theta_target", C.c_double)]


class tm_solver_opt(C.Structure):
    _fields_ = [("tag", C.c_int32), ("inner", C.c_int32), ("rtol", C.c_double), ("atol", C.c_double), ("max_inner", C.c_uint64),
                ("check_every", C.c_uint32), ("flags", C.c_uint32), ("omega", C.c_double)]


class tm_stats(C.Structure):
    _fields_ = [("outer_iterations", C.c_uint64), ("inner_iterations", C.c_uint64), ("operator_sweeps", C.c_uint64),
                ("last_residual", C.c_double), ("last_dx2", C.c_double), ("last_dy2", C.c_double), ("scaled_residual_rms", C.c_double),
                ("seconds", C.c_double), ("not_converged", C.c_int32), ("_pad", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("_")}


EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p)
EXCHANGE_WAIT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p)


LOG_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int32, C.c_uint64, C.c_double)


class tm_comm_hooks(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("rank", C.c_int32), ("nranks", C.c_int32), ("owner", C.POINTER(C.c_int32)),
                ("exchange", EXCHANGE_FN), ("allreduce_sum", ALLREDUCE_FN), ("exchange_wait", EXCHANGE_WAIT_FN), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_uint64)]


class tm_plan_rows(C.Structure):
    _fields_ = [("nrows", C.c_uint64), ("row", C.POINTER(C.c_int64)), ("kind", C.POINTER(C.c_int32)), ("ncols", C.POINTER(C.c_int32)),
                ("cols", C.POINTER(C.c_int64)), ("coef_x", C.POINTER(C.c_double)), ("coef_y", C.POINTER(C.c_double)),
                ("rhs", C.POINTER(C.c_double)), ("slot", C.POINTER(C.c_int32))]


class tm_plan_local_info(C.Structure):
    _fields_ = [("n_owned", C.c_int64), ("n_ghost", C.c_int64), ("n_send", C.c_int64), ("npeers", C.c_int32), ("nowned_blocks", C.c_int32),
                ("owned_blocks", C.POINTER(C.c_int64)), ("local_start", C.POINTER(C.c_int64)), ("ghost_gid", C.POINTER(C.c_int64)),
                ("send_ids", C.POINTER(C.c_int32)), ("send_gid", C.POINTER(C.c_int64)), ("peer_rank", C.POINTER(C.c_int32)),
                ("send_offset", C.POINTER(C.c_int64)), ("send_count", C.POINTER(C.c_int64)), ("recv_offset", C.POINTER(C.c_int64)),
                ("recv_count", C.POINTER(C.c_int64)), ("send_first", C.POINTER(C.c_int64)), ("direct_send", C.c_int32), ("_pad", C.c_int32),
                ("n_ghost_rows", C.c_int64), ("ghost_row_gid", C.POINTER(C.c_int64)), ("ghost_row_kind", C.POINTER(C.c_int32)),
                ("ghost_row_cols", C.POINTER(C.c_int64))]


class tm_rccl_peer_table(C.Structure):
    _fields_ = [("npeers", C.c_int32), ("direct_send", C.c_int32), ("send_rows", C.c_int64), ("recv_rows", C.c_int64),
                ("peer", C.POINTER(C.c_int32)), ("send_off", C.POINTER(C.c_int64)), ("send_cnt", C.POINTER(C.c_int64)),
                ("recv_off", C.POINTER(C.c_int64)), ("recv_cnt", C.POINTER(C.c_int64))]


_i32p = C.POINTER(C.c_int32)


class tm_edge_tables_info(C.Structure):
    _fields_ = ([("nrows", C.c_int64), ("nruns", C.c_int64), ("nwg", C.c_int64)] +
                [(k, _i32p) for k in ("first", "count", "row0", "row_stride", "col0", "col_stride", "met0", "met_stride", "kind", "ncols", "self", "flags",
                                     "wg_run", "wg_k0")] +
                [("gid", C.POINTER(C.c_int64)), ("nstrips", C.c_int64), ("ntasks", C.c_int64), ("strip_off", _i32p), ("task", _i32p)])


class tm_quality(C.Structure):
    _fields_ = [("cells", C.c_uint64), ("inverted", C.c_uint64), ("degenerate", C.c_uint64), ("orientation", C.c_int32), ("_pad", C.c_int32),
                ("min_scaled_jacobian", C.c_double), ("worst_block", C.c_uint64), ("worst_i", C.c_uint64), ("worst_j", C.c_uint64),
                ("min_angle_deg", C.c_double), ("max_angle_deg", C.c_double), ("max_aspect", C.c_double), ("max_growth_i", C.c_double),
                ("max_growth_j", C.c_double), ("min_area", C.c_double), ("max_area", C.c_double), ("total_area", C.c_double),
                ("hist", C.c_uint64 * 10)]


class tm_quality3d(C.Structure):
    _fields_ = [("cells", C.c_uint64), ("inverted", C.c_uint64), ("degenerate", C.c_uint64), ("orientation", C.c_int32), ("_pad", C.c_int32),
                ("min_scaled_jacobian", C.c_double), ("worst_block", C.c_uint64), ("worst_i", C.c_uint64), ("worst_j", C.c_uint64),
                ("worst_k", C.c_uint64), ("max_aspect", C.c_double), ("max_growth_k", C.c_double), ("min_volume", C.c_double),
                ("max_volume", C.c_double), ("total_volume", C.c_double), ("hist", C.c_uint64 * 10)]


class tm_stack_opt(C.Structure):
    _fields_ = [("ncuts", C.c_uint64), ("span", C.POINTER(C.c_double)), ("nlayers", C.c_uint64), ("layers", C.POINTER(C.c_double)),
                ("interpolation", C.c_int32), ("mapping", C.c_int32)]


class tm_stack_surfaces(C.Structure):
    _fields_ = [("ncuts", C.c_uint64), ("nknots", C.POINTER(C.c_uint64)), ("u", C.POINTER(C.POINTER(C.c_double))),
                ("x", C.POINTER(C.POINTER(C.c_double))), ("r", C.POINTER(C.POINTER(C.c_double))), ("rref", C.POINTER(C.c_double)),
                ("interpolation", C.c_int32), ("_pad", C.c_int32)]


class tm_ho_opt(C.Structure):
    _fields_ = [("order", C.c_int32), ("distribution", C.c_int32), ("nodes", C.POINTER(C.c_double))]


class tm_ho_quality(C.Structure):
    _fields_ = [("elements", C.c_uint64), ("invalid", C.c_uint64), ("orientation", C.c_int32), ("order", C.c_int32),
                ("min_scaled_jacobian", C.c_double), ("worst_block", C.c_uint64), ("worst_e", C.c_uint64), ("worst_f", C.c_uint64),
                ("min_jacobian", C.c_double), ("max_jacobian", C.c_double), ("hist", C.c_uint64 * 10)]


class tm_ho3_quality(C.Structure):   # 160 bytes
    _fields_ = [("elements", C.c_uint64), ("invalid", C.c_uint64), ("orientation", C.c_int32), ("order", C.c_int32),
                ("min_scaled_jacobian", C.c_double), ("worst_block", C.c_uint64), ("worst_e", C.c_uint64), ("worst_f", C.c_uint64),
                ("worst_g", C.c_uint64), ("min_jacobian", C.c_double), ("max_jacobian", C.c_double), ("hist", C.c_uint64 * 10)]


class tm_ho_certificate(C.Structure):   # 152 bytes
    _fields_ = [("elements", C.c_uint64), ("proven", C.c_uint64), ("invalid", C.c_uint64), ("undecided", C.c_uint64), ("hidden_invalid", C.c_uint64),
                ("orientation", C.c_int32), ("order", C.c_int32), ("max_depth", C.c_int32), ("has_unproven", C.c_int32),
                ("decided_at", C.c_uint64 * 5), ("min_scaled_bound", C.c_double), ("worst_block", C.c_uint64), ("worst_e", C.c_uint64),
                ("worst_f", C.c_uint64), ("first_unproven_block", C.c_uint64), ("first_unproven_e", C.c_uint64), ("first_unproven_f", C.c_uint64)]


class tm_ho3_certificate(C.Structure):   # 160 bytes
    _fields_ = [("elements", C.c_uint64), ("proven", C.c_uint64), ("invalid", C.c_uint64), ("undecided", C.c_uint64), ("hidden_invalid", C.c_uint64),
                ("orientation", C.c_int32), ("order", C.c_int32), ("max_depth", C.c_int32), ("has_unproven", C.c_int32),
                ("decided_at", C.c_uint64 * 4), ("min_scaled_bound", C.c_double), ("worst_block", C.c_uint64), ("worst_e", C.c_uint64),
                ("worst_f", C.c_uint64), ("worst_g", C.c_uint64), ("first_unproven_block", C.c_uint64), ("first_unproven_e", C.c_uint64),
                ("first_unproven_f", C.c_uint64), ("first_unproven_g", C.c_uint64)]


class tm_weld_info(C.Structure):   # 88 bytes
    _fields_ = [("nodes_in", C.c_uint64), ("nodes_out", C.c_uint64), ("classes_2", C.c_uint64), ("classes_3", C.c_uint64), ("classes_4", C.c_uint64),
                ("classes_5_up", C.c_uint64), ("max_class", C.c_uint64), ("periodic_pairs", C.c_uint64), ("gap_node", C.c_uint64),
                ("max_gap", C.c_double), ("periodic_gap", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class tm_weld_patch(C.Structure):   # 88 bytes
    _fields_ = [("kind", C.c_int32), ("source", C.c_int32), ("partner", C.c_int32), ("_pad", C.c_int32), ("face_begin", C.c_uint64), ("faces", C.c_uint64),
                ("translation", C.c_double * 2), ("measure", C.c_double), ("normal", C.c_double * 3), ("moment", C.c_double)]


class tm_weld_boundary_info(C.Structure):   # 56 bytes
    _fields_ = [("patches", C.c_uint64), ("faces", C.c_uint64), ("nodes_per_face", C.c_uint64), ("lateral_faces", C.c_uint64), ("cap_faces", C.c_uint64),
                ("loops", C.c_uint64), ("irregular_nodes", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class tm_wall_image(C.Structure):   # 40 bytes
    _fields_ = [("t", C.c_double * 3), ("c", C.c_double), ("s", C.c_double)]


class tm_wall_info(C.Structure):   # 88 bytes
    _fields_ = [("points", C.c_uint64), ("faces", C.c_uint64), ("primitives", C.c_uint64), ("images", C.c_uint64), ("groups", C.c_uint64),
                ("on_wall", C.c_uint64), ("nan_points", C.c_uint64), ("nearest_via_image", C.c_uint64), ("max_point", C.c_uint64),
                ("pairs_evaluated", C.c_uint64), ("max_distance", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class tm_fv_plan(C.Structure):   # 40 bytes
    _fields_ = [("cells", C.c_uint64), ("internal_faces", C.c_uint64), ("boundary_faces", C.c_uint64), ("nodes_per_face", C.c_uint64),
                ("faces_per_cell", C.c_uint64)]


class tm_fv_info(C.Structure):   # 144 bytes
    _fields_ = [("cells", C.c_uint64), ("internal_faces", C.c_uint64), ("boundary_faces", C.c_uint64), ("min_volume_cell", C.c_uint64),
                ("max_volume_cell", C.c_uint64), ("negative_cells", C.c_uint64), ("first_negative_cell", C.c_uint64), ("max_closedness_cell", C.c_uint64),
                ("min_cos_face", C.c_uint64), ("nonorthogonal_faces", C.c_uint64), ("inverted_faces", C.c_uint64), ("max_skewness_face", C.c_uint64),
                ("min_volume", C.c_double), ("max_volume", C.c_double), ("total_volume", C.c_double), ("max_closedness", C.c_double),
                ("min_cos", C.c_double), ("max_skewness", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class tm_fv_fields(C.Structure):   # 56 bytes
    _fields_ = [(k, C.POINTER(C.c_double)) for k in ("volume", "centre", "closedness", "area", "face_centre", "cos", "skewness")]


class tm_smooth3d_opt(C.Structure):   # 56 bytes
    _fields_ = [("algorithm", C.c_int32), ("_pad", C.c_int32), ("sweeps", C.c_uint64), ("omega", C.c_double), ("tol", C.c_double),
                ("f1", C.POINTER(C.c_double)), ("f2", C.POINTER(C.c_double)), ("f3", C.POINTER(C.c_double))]


class tm_smooth3d_info(C.Structure):   # 136 bytes
    _fields_ = [(k, C.c_uint64) for k in ("nodes", "interior", "sweeps_done", "frozen", "first_neg", "first_pos", "first_zero_or_nan", "last_neg",
                                          "last_pos", "last_zero_or_nan", "last_max_node")] + \
               [("first_sum_sq", C.c_double), ("last_sum_sq", C.c_double), ("last_max_update", C.c_double), ("control_max", C.c_double * 3)]


TM_S3_LAPLACE, TM_S3_THOMAS_MIDDLECOFF, TM_S3_PRESCRIBED = 0, 1, 2
S3_TI, S3_TJ, S3_KCHUNK = 32, 8, 16   # csrc/tm_smooth3d.hip: the (i, j) tile of a workgroup and the node layers of a k-chunk
TM_WALL_NO_CULL = 1
WD_G = 32.0        # csrc/tm_wall_distance.hpp: |d2 - exact d2| <= WD_G * 2^-53 * rho2
WD_GROUP = 64      # primitives per group
WD_CHUNK = 64      # group records per LDS chunk of the kernel

# every symbol include/tm_hip.h declares (checked by tests/test_capi_symbols.py)
EXPORTS = [
    "tm_last_error", "tm_abi_version", "tm_set_log", "tm_csr_solve", "tm_tfi_block", "tm_tfi_linear2d", "tm_smooth_mesh", "tm_smoother_create",
    "tm_smoother_workspace_bytes", "tm_smoother_iterate", "tm_smoother_iterate_until", "tm_smoother_iterate_until_update", "tm_smoother_download", "tm_smoother_upload", "tm_smoother_destroy",
    "tm_smoother_exchange_plan", "tm_smoother_apply", "tm_smoother_rhs", "tm_smoother_row_kinds", "tm_smoother_dof",
    "tm_smoother_control_function", "tm_smoother_profile", "tm_smoother_profile_read", "tm_plan_build", "tm_plan_free", "tm_plan_local", "tm_plan_local_free", "tm_dev_tfi_block", "tm_dev_relax_sweep",
    "tm_dev_relax_partials_needed", "tm_export_soa", "tm_smoother_export_soa", "tm_rccl_unique_id", "tm_rccl_comm_create", "tm_rccl_comm_destroy", "tm_rccl_hooks",
    "tm_rccl_peer_table_build", "tm_rccl_peer_table_free", "tm_white_math_probe", "tm_stream_probe", "tm_smoother_queue_ordering", "tm_smoother_inner", "tm_csr_ilu0_probe", "tm_rccl_hooks_for", "tm_smoother_assemble_csr", "tm_smoother_apply_reference_order",
    "tm_smoother_inner_counts", "tm_mesh_quality", "tm_mesh_quality_host", "tm_smoother_quality", "tm_smoother_quality_field",
    "tm_csr_residual", "tm_smoother_residual", "tm_smoother_refine_report",
    "tm_smoother_set_control_function", "tm_smoother_update_control_function",
    "tm_stack_weights", "tm_stack_block", "tm_stack_block_host", "tm_stack_smoothers",
    "tm_quality3d_planes_host", "tm_stack_quality", "tm_stack_quality_host", "tm_stack_smoothers_quality", "tm_stack_smoothers_quality_field",
    "tm_quality3d_total",
    "tm_stack_surface_tables", "tm_stack_block_surf", "tm_stack_block_surf_host", "tm_stack_smoothers_surf",
    "tm_stack_quality_surf", "tm_stack_quality_surf_host", "tm_stack_smoothers_quality_surf", "tm_stack_smoothers_quality_field_surf",
    "tm_ho_tables", "tm_ho_check", "tm_ho_elevate", "tm_ho_elevate_host", "tm_smoother_elevate", "tm_ho_quality_total",
    "tm_ho_certify_tables", "tm_ho_certify", "tm_ho_certify_host", "tm_smoother_certify", "tm_ho_jacobian_bezier_host", "tm_ho_certificate_total",
    "tm_ho3_check", "tm_ho3_planes_host", "tm_stack_elevate", "tm_stack_elevate_host", "tm_stack_smoothers_elevate", "tm_ho3_quality_total",
    "tm_ho3_certify_tables", "tm_ho3_jacobian_bezier_host", "tm_ho3_certify_planes_host", "tm_stack_certify", "tm_stack_certify_host",
    "tm_stack_smoothers_certify", "tm_ho3_certificate_total",
    "tm_weld_map", "tm_weld_map_host", "tm_weld_points", "tm_weld_points_host", "tm_smoother_weld", "tm_weld_cells", "tm_weld_cells_host",
    "tm_weld_periodic_pairs",
    "tm_weld_boundary_plan", "tm_weld_boundary_faces", "tm_weld_boundary_faces_host", "tm_weld_faces_measure", "tm_weld_faces_measure_host",
    "tm_smoother_weld_boundary",
    "tm_wall_distance", "tm_wall_distance_host", "tm_wall_select", "tm_smoother_wall_distance",
    "tm_weld_faces_plan", "tm_weld_faces", "tm_weld_faces_host", "tm_fv_metrics", "tm_fv_metrics_host", "tm_smoother_fv_report",
    "tm_smooth3d_planes", "tm_smooth3d_planes_host", "tm_smooth3d_control", "tm_smooth3d_control_host", "tm_stack_smoothers_smooth",
    "tm_stack_smoothers_smooth_surf",
    "tm_mg_transfer_probe", "tm_smoother_mg_levels", "tm_smoother_precondition_probe", "tm_edge_tables_probe", "tm_edge_tables_free",
]

_lib = None
_dp = C.POINTER(C.c_double)


def _share_hip_runtime():
    """A process must run on ONE HIP runtime.  libtm_hip.so is linked against the system's libamdhip64; PyTorch ships its own
    copy and, loaded second, finds no GPU ("No HIP GPUs are available").  When torch is installed but not imported yet, its
    copy is loaded first so that both resolve to it -- the order every test and bench.py already has."""
    import importlib.util
    import sys

    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    rt = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(rt):
        try:
            C.CDLL(rt, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    """Load libtm_hip.so; raises OSError when it has not been built (no silent fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "or `make -C turbomesh_amd/csrc`; turbomesh_amd has no CPU fallback")
        _share_hip_runtime()
        L = C.CDLL(LIB_PATH)
        L.tm_last_error.restype = C.c_char_p
        L.tm_csr_solve.argtypes = [C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _dp, _dp, _dp, _dp, _dp, _dp, C.POINTER(tm_solver_opt),
                                   C.POINTER(tm_stats)]
        L.tm_csr_residual.argtypes = [C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)] + [_dp] * 8
        L.tm_set_log.argtypes = [LOG_FN, C.c_void_p]
        L.tm_set_log.restype = None
        L.tm_smoother_dof.restype = C.c_uint64
        L.tm_smoother_dof.argtypes = [C.c_void_p]
        L.tm_dev_relax_partials_needed.restype = C.c_uint64
        L.tm_dev_relax_partials_needed.argtypes = [C.c_uint64, C.c_uint64]
        L.tm_tfi_block.argtypes = [_dp, C.c_uint64, C.c_uint64] + [_dp] * 8
        L.tm_tfi_linear2d.argtypes = [_dp, C.c_uint64, C.c_uint64] + [_dp] * 4
        L.tm_smooth_mesh.argtypes = [C.POINTER(tm_mesh_desc), C.c_uint64, C.POINTER(tm_solver_opt), C.POINTER(tm_control_fn), C.POINTER(tm_stats)]
        L.tm_smoother_create.argtypes = [C.POINTER(tm_mesh_desc), C.POINTER(tm_solver_opt), C.POINTER(tm_control_fn), C.POINTER(tm_comm_hooks),
                                         C.c_void_p, C.POINTER(C.c_void_p)]
        L.tm_smoother_workspace_bytes.argtypes = [C.POINTER(tm_mesh_desc), C.POINTER(tm_solver_opt), C.POINTER(tm_control_fn),
                                                  C.POINTER(tm_comm_hooks), C.POINTER(C.c_uint64)]
        L.tm_smoother_iterate.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(tm_stats)]
        L.tm_smoother_iterate_until.argtypes = [C.c_void_p, C.c_uint64, C.c_double, C.POINTER(tm_stats)]
        L.tm_smoother_iterate_until_update.argtypes = [C.c_void_p, C.c_uint64, C.c_double, C.POINTER(tm_stats)]
        L.tm_smoother_download.argtypes = [C.c_void_p, C.POINTER(tm_mesh_desc)]
        L.tm_smoother_upload.argtypes = [C.c_void_p, C.POINTER(tm_mesh_desc)]
        L.tm_smoother_destroy.argtypes = [C.c_void_p]
        L.tm_smoother_destroy.restype = None
        L.tm_smoother_exchange_plan.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.POINTER(C.c_int32))] + [C.POINTER(C.POINTER(C.c_int64))] * 4
        L.tm_smoother_apply.argtypes = [C.c_void_p, _dp, _dp, C.c_int]
        L.tm_smoother_rhs.argtypes = [C.c_void_p, _dp]
        L.tm_smoother_residual.argtypes = [C.c_void_p, _dp, _dp]
        L.tm_smoother_refine_report.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), _dp, C.POINTER(C.c_uint64)]
        L.tm_smoother_assemble_csr.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _dp, _dp, C.c_uint64, C.POINTER(C.c_uint64)]
        L.tm_smoother_apply_reference_order.argtypes = [C.c_void_p, _dp, _dp]
        L.tm_smoother_row_kinds.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.tm_smoother_control_function.argtypes = [C.c_void_p, _dp]
        L.tm_smoother_set_control_function.argtypes = [C.c_void_p, _dp]
        L.tm_smoother_update_control_function.argtypes = [C.c_void_p]
        L.tm_smoother_profile.argtypes = [C.c_void_p, C.c_int]
        L.tm_smoother_profile_read.argtypes = [C.c_void_p, _dp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.tm_smoother_queue_ordering.argtypes = [C.c_void_p]
        L.tm_smoother_inner.argtypes = [C.c_void_p]
        L.tm_smoother_inner_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.tm_csr_ilu0_probe.argtypes = [C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _dp, _dp, _dp, _dp]
        L.tm_plan_build.argtypes = [C.POINTER(tm_mesh_desc), C.POINTER(tm_plan_rows)]
        L.tm_plan_free.argtypes = [C.POINTER(tm_plan_rows)]
        L.tm_plan_free.restype = None
        L.tm_export_soa.argtypes = [_dp, C.c_uint64, C.c_uint64, _dp, _dp]
        L.tm_smoother_export_soa.argtypes = [C.c_void_p, C.c_uint64, _dp, _dp, _dp, _dp]
        L.tm_mesh_quality.argtypes = [C.POINTER(tm_mesh_desc), C.POINTER(tm_quality), C.POINTER(tm_quality)]
        L.tm_mesh_quality_host.argtypes = [C.POINTER(tm_mesh_desc), C.POINTER(tm_quality), C.POINTER(tm_quality)]
        L.tm_smoother_quality.argtypes = [C.c_void_p, C.POINTER(tm_quality), C.POINTER(tm_quality)]
        L.tm_smoother_quality_field.argtypes = [C.c_void_p, C.c_uint64, _dp]
        L.tm_stack_weights.argtypes = [C.POINTER(tm_stack_opt), _dp]
        L.tm_stack_block.argtypes = [C.POINTER(C.POINTER(tm_mesh_desc)), C.POINTER(tm_stack_opt), C.c_uint64, C.c_uint64, C.c_uint64, _dp, _dp, _dp]
        L.tm_stack_block_host.argtypes = L.tm_stack_block.argtypes
        L.tm_stack_smoothers.argtypes = [C.POINTER(C.c_void_p), C.POINTER(tm_stack_opt), C.c_uint64, C.c_uint64, C.c_uint64, _dp, _dp, _dp]
        L.tm_quality3d_planes_host.argtypes = [_dp, _dp, _dp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(tm_quality3d), _dp]
        L.tm_stack_quality.argtypes = [C.POINTER(C.POINTER(tm_mesh_desc)), C.POINTER(tm_stack_opt), C.c_uint64, C.POINTER(tm_quality3d)]
        L.tm_stack_quality_host.argtypes = L.tm_stack_quality.argtypes
        L.tm_stack_smoothers_quality.argtypes = [C.POINTER(C.c_void_p), C.POINTER(tm_stack_opt), C.c_uint64, C.POINTER(tm_quality3d)]
        L.tm_stack_smoothers_quality_field.argtypes = [C.POINTER(C.c_void_p), C.POINTER(tm_stack_opt), C.c_uint64, C.c_uint64, C.c_uint64, _dp]
        L.tm_quality3d_total.argtypes = [C.POINTER(tm_quality3d), C.c_uint64, C.POINTER(tm_quality3d)]
        _sfp, _u64p = C.POINTER(tm_stack_surfaces), C.POINTER(C.c_uint64)
        L.tm_stack_surface_tables.argtypes = [C.POINTER(tm_stack_opt), _sfp, _dp]
        L.tm_stack_block_surf.argtypes = [C.POINTER(C.POINTER(tm_mesh_desc)), C.POINTER(tm_stack_opt), _sfp, C.c_uint64, C.c_uint64, C.c_uint64, _dp, _dp, _dp, _u64p]
        L.tm_stack_block_surf_host.argtypes = L.tm_stack_block_surf.argtypes
        L.tm_stack_smoothers_surf.argtypes = [C.POINTER(C.c_void_p), C.POINTER(tm_stack_opt), _sfp, C.c_uint64, C.c_uint64, C.c_uint64, _dp, _dp, _dp, _u64p]
        L.tm_stack_quality_surf.argtypes = [C.POINTER(C.POINTER(tm_mesh_desc)), C.POINTER(tm_stack_opt), _sfp, C.c_uint64, C.POINTER(tm_quality3d)]
        L.tm_stack_quality_surf_host.argtypes = L.tm_stack_quality_surf.argtypes
        L.tm_stack_smoothers_quality_surf.argtypes = [C.POINTER(C.c_void_p), C.POINTER(tm_stack_opt), _sfp, C.c_uint64, C.POINTER(tm_quality3d)]
        L.tm_stack_smoothers_quality_field_surf.argtypes = [C.POINTER(C.c_void_p), C.POINTER(tm_stack_opt), _sfp, C.c_uint64, C.c_uint64, C.c_uint64, _dp]
        L.tm_ho_tables.argtypes = [C.POINTER(tm_ho_opt), _dp, _dp, _dp]
        L.tm_ho_check.argtypes = [C.POINTER(tm_mesh_desc), C.POINTER(tm_ho_opt)]
        L.tm_ho_elevate.argtypes = [C.POINTER(tm_mesh_desc), C.POINTER(tm_ho_opt), C.c_uint64, _dp, _dp, C.POINTER(tm_ho_quality), _dp]
        L.tm_ho_elevate_host.argtypes = L.tm_ho_elevate.argtypes
        L.tm_smoother_elevate.argtypes = [C.c_void_p, C.POINTER(tm_ho_opt), C.c_uint64, _dp, _dp, C.POINTER(tm_ho_quality), _dp]
        L.tm_ho_quality_total.argtypes = [C.POINTER(tm_ho_quality), C.c_uint64, C.POINTER(tm_ho_quality)]
        L.tm_ho_certify_tables.argtypes = [C.POINTER(tm_ho_opt), _dp, _dp, _dp, _dp, _dp]
        L.tm_ho_certify.argtypes = [C.POINTER(tm_mesh_desc), C.POINTER(tm_ho_opt), C.c_int32, C.c_uint64, C.POINTER(tm_ho_certificate), C.POINTER(C.c_uint8), _dp]
        L.tm_ho_certify_host.argtypes = L.tm_ho_certify.argtypes
        L.tm_smoother_certify.argtypes = [C.c_void_p, C.POINTER(tm_ho_opt), C.c_int32, C.c_uint64, C.POINTER(tm_ho_certificate), C.POINTER(C.c_uint8), _dp]
        L.tm_ho_jacobian_bezier_host.argtypes = [C.POINTER(tm_mesh_desc), C.POINTER(tm_ho_opt), C.c_uint64, C.c_uint64, C.c_uint64, _dp]
        L.tm_ho_certificate_total.argtypes = [C.POINTER(tm_ho_certificate), C.c_uint64, C.POINTER(tm_ho_certificate)]
        L.tm_ho3_check.argtypes = [C.POINTER(tm_mesh_desc), C.POINTER(tm_stack_opt), C.POINTER(tm_ho_opt)]
        L.tm_ho3_planes_host.argtypes = [_dp, _dp, _dp, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(tm_ho_opt), C.c_uint64, _dp, _dp, _dp, C.POINTER(tm_ho3_quality), _dp]
        _ho3_tail = [_sfp, C.POINTER(tm_ho_opt), C.c_uint64, C.c_uint64, C.c_uint64, _dp, _dp, _dp, C.POINTER(tm_ho3_quality), _dp, _u64p]
        L.tm_stack_elevate.argtypes = [C.POINTER(C.POINTER(tm_mesh_desc)), C.POINTER(tm_stack_opt)] + _ho3_tail
        L.tm_stack_elevate_host.argtypes = L.tm_stack_elevate.argtypes
        L.tm_stack_smoothers_elevate.argtypes = [C.POINTER(C.c_void_p), C.POINTER(tm_stack_opt)] + _ho3_tail
        L.tm_ho3_quality_total.argtypes = [C.POINTER(tm_ho3_quality), C.c_uint64, C.POINTER(tm_ho3_quality)]
        _u8p, _c3p = C.POINTER(C.c_uint8), C.POINTER(tm_ho3_certificate)
        L.tm_ho3_certify_tables.argtypes = [C.POINTER(tm_ho_opt), _dp, _dp, _dp, _dp, _dp]
        L.tm_ho3_jacobian_bezier_host.argtypes = [_dp, _dp, _dp, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(tm_ho_opt), C.c_uint64, C.c_uint64, C.c_uint64, _dp]
        L.tm_ho3_certify_planes_host.argtypes = [_dp, _dp, _dp, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(tm_ho_opt), C.c_int32, C.c_uint64, _c3p, _u8p, _dp]
        _h3_tail = [_sfp, C.POINTER(tm_ho_opt), C.c_int32, C.c_uint64, _c3p, _u8p, _dp, _u64p]
        L.tm_stack_certify.argtypes = [C.POINTER(C.POINTER(tm_mesh_desc)), C.POINTER(tm_stack_opt)] + _h3_tail
        L.tm_stack_certify_host.argtypes = L.tm_stack_certify.argtypes
        L.tm_stack_smoothers_certify.argtypes = [C.POINTER(C.c_void_p), C.POINTER(tm_stack_opt)] + _h3_tail
        L.tm_ho3_certificate_total.argtypes = [_c3p, C.c_uint64, _c3p]
        _wip, _dpp = C.POINTER(tm_weld_info), C.POINTER(_dp)
        L.tm_weld_map.argtypes = [C.POINTER(tm_mesh_desc), _i32p, _wip]
        L.tm_weld_map_host.argtypes = L.tm_weld_map.argtypes
        L.tm_weld_points.argtypes = [C.POINTER(tm_mesh_desc), _i32p, C.c_int32, C.c_uint64, _dpp, _dpp, _wip]
        L.tm_weld_points_host.argtypes = L.tm_weld_points.argtypes
        L.tm_smoother_weld.argtypes = [C.c_void_p, _i32p, _dp, _dp, _wip]
        L.tm_weld_cells.argtypes = [C.POINTER(tm_mesh_desc), _i32p, C.c_uint64, C.c_int32, C.c_uint64, _i32p]
        L.tm_weld_cells_host.argtypes = L.tm_weld_cells.argtypes
        L.tm_weld_periodic_pairs.argtypes = [C.POINTER(tm_mesh_desc), _i32p, _i32p]
        _wpp = C.POINTER(tm_weld_patch)
        L.tm_weld_boundary_plan.argtypes = [C.POINTER(tm_mesh_desc), C.c_int32, C.c_uint64, C.POINTER(tm_weld_boundary_info), _wpp]
        L.tm_weld_boundary_faces.argtypes = [C.POINTER(tm_mesh_desc), _i32p, C.c_uint64, C.c_int32, C.c_uint64, _i32p, _i32p, _i32p, _i32p]
        L.tm_weld_boundary_faces_host.argtypes = L.tm_weld_boundary_faces.argtypes
        L.tm_weld_faces_measure.argtypes = [C.c_int32, C.c_int32, C.c_uint64, _i32p, _i32p, C.c_uint64, C.c_uint64, C.c_int32, _dpp, _wpp]
        L.tm_weld_faces_measure_host.argtypes = L.tm_weld_faces_measure.argtypes
        L.tm_smoother_weld_boundary.argtypes = [C.c_void_p, C.c_int32, _i32p, _i32p, _i32p, _wpp]
        _wimp, _winp = C.POINTER(tm_wall_image), C.POINTER(tm_wall_info)
        L.tm_wall_distance.argtypes = [C.c_int32, C.c_uint64, _i32p, C.c_uint64, _dpp, C.c_uint64, _wimp, C.c_uint32, _dp, _i32p, _i32p, _winp]
        L.tm_wall_distance_host.argtypes = L.tm_wall_distance.argtypes
        L.tm_wall_select.argtypes = [C.POINTER(tm_mesh_desc), C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64), _i32p, C.POINTER(C.c_uint64), _wimp]
        L.tm_smoother_wall_distance.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, _i32p, _dp, _i32p, _i32p, _winp]
        L.tm_weld_faces_plan.argtypes = [C.POINTER(tm_mesh_desc), C.c_uint64, C.POINTER(tm_fv_plan)]
        L.tm_weld_faces.argtypes = [C.POINTER(tm_mesh_desc), _i32p, C.c_uint64, C.c_uint64, _i32p, _i32p, _i32p, _i32p, _i32p]
        L.tm_weld_faces_host.argtypes = L.tm_weld_faces.argtypes
        L.tm_fv_metrics.argtypes = [C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64, _i32p, _i32p, _i32p, _i32p, C.c_uint64, _dpp, C.POINTER(tm_fv_fields),
                                    C.POINTER(tm_fv_info)]
        L.tm_fv_metrics_host.argtypes = L.tm_fv_metrics.argtypes
        L.tm_smoother_fv_report.argtypes = [C.c_void_p, _i32p, C.POINTER(tm_fv_info)]
        _s3o, _s3i = C.POINTER(tm_smooth3d_opt), C.POINTER(tm_smooth3d_info)
        L.tm_smooth3d_planes.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, _dp, _dp, _dp, _s3o, _s3i]
        L.tm_smooth3d_planes_host.argtypes = L.tm_smooth3d_planes.argtypes
        L.tm_smooth3d_control.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64] + [_dp] * 6
        L.tm_smooth3d_control_host.argtypes = L.tm_smooth3d_control.argtypes
        L.tm_stack_smoothers_smooth.argtypes = [C.POINTER(C.c_void_p), C.POINTER(tm_stack_opt), C.c_uint64, _s3o, _dp, _dp, _dp, _s3i]
        L.tm_stack_smoothers_smooth_surf.argtypes = [C.POINTER(C.c_void_p), C.POINTER(tm_stack_opt), C.POINTER(tm_stack_surfaces), C.c_uint64, _s3o, _dp, _dp, _dp, _s3i]
        L.tm_rccl_unique_id.argtypes =[C.c_char_p, C.c_void_p]
        L.tm_rccl_comm_create.argtypes = [C.c_char_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        L.tm_rccl_comm_destroy.argtypes = [C.c_void_p]
        L.tm_rccl_comm_destroy.restype = None
        L.tm_rccl_hooks.argtypes = [C.c_void_p, C.POINTER(tm_mesh_desc), C.POINTER(C.c_int32), C.POINTER(tm_comm_hooks)]
        L.tm_rccl_hooks_for.argtypes = [C.c_void_p, C.POINTER(tm_mesh_desc), C.POINTER(C.c_int32), C.POINTER(tm_solver_opt), C.POINTER(tm_control_fn), C.POINTER(tm_comm_hooks)]
        L.tm_plan_local.argtypes = [C.POINTER(tm_mesh_desc), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.POINTER(tm_plan_local_info)]
        L.tm_plan_local_free.argtypes = [C.POINTER(tm_plan_local_info)]
        L.tm_plan_local_free.restype = None
        L.tm_dev_tfi_block.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64] + [C.c_void_p] * 8 + [C.c_void_p]
        L.tm_dev_relax_sweep.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_double, C.c_void_p, C.c_uint64,
                                         C.POINTER(C.c_uint64), C.c_void_p]
        L.tm_rccl_peer_table_build.argtypes = [C.POINTER(tm_mesh_desc), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.POINTER(tm_rccl_peer_table)]
        L.tm_rccl_peer_table_free.argtypes = [C.POINTER(tm_rccl_peer_table)]
        L.tm_rccl_peer_table_free.restype = None
        L.tm_white_math_probe.argtypes = [_dp, _dp, C.c_uint64, _dp, _dp]
        L.tm_stream_probe.argtypes = [C.c_uint64, C.c_int32, _dp, _dp]
        L.tm_mg_transfer_probe.argtypes = [C.c_int32, C.c_uint64, C.c_uint64, C.c_int32, C.c_int32, _dp, _dp, C.c_double, C.c_double, _dp]
        L.tm_smoother_mg_levels.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_uint32, C.POINTER(C.c_int32), _dp]
        L.tm_smoother_precondition_probe.argtypes = [C.c_void_p, _dp, _dp, _dp]
        L.tm_edge_tables_probe.argtypes = [C.POINTER(tm_mesh_desc), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(tm_edge_tables_info)]
        L.tm_edge_tables_free.argtypes = [C.POINTER(tm_edge_tables_info)]
        L.tm_edge_tables_free.restype = None
        if hasattr(L, "tm_tune_apply"):   # measurement build (TM_HIP_LIB=.../libtm_hip_dbg.so, tools/)
            L.tm_debug_null_hooks.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(tm_comm_hooks)]
            L.tm_diag_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p]
            L.tm_tune_fuse.argtypes = [C.c_int]
            L.tm_tune_apply.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
        _lib = L
    return _lib


def check(rc):
    if rc < 0:
        raise TmError(rc, lib().tm_last_error().decode())
    return rc


def f64ptr(a):
    return a.ctypes.data_as(_dp)


class MeshDesc:
    """Marshals a discrete.Mesh into a tm_mesh_desc; keeps the ctypes arrays alive."""

    def __init__(self, mesh, with_coordinates=True):
        blocks = mesh.blocks
        self._blocks = (tm_block * max(1, len(blocks)))()
        for k, b in enumerate(blocks):
            data = b.points.data
            if with_coordinates and data is not None:
                if data.dtype != np.float64 or not data.flags["C_CONTIGUOUS"]:
                    raise TmError(TM_E_ARG, "block coordinates must be C-contiguous float64")
                self._blocks[k] = tm_block(f64ptr(data), b.points.size[0], b.points.size[1])
            else:
                self._blocks[k] = tm_block(None, b.points.size[0], b.points.size[1])
        conns = mesh.connections
        self._conns = (tm_connection * max(1, len(conns)))()
        for k, c in enumerate(conns):
            tc = tm_connection()
            for s in range(2):
                r = c.ranges[s]
                tc.r[s] = tm_range(r.block, int(r.side), 0, r.start, r.end)
            tc.has_periodicity = 0 if c.periodicity is None else 1
            if c.periodicity is not None:
                tc.periodicity[0], tc.periodicity[1] = float(c.periodicity[0]), float(c.periodicity[1])
            self._conns[k] = tc
        bcs = mesh.boundary_conditions
        self._bcs = (tm_condition * max(1, len(bcs)))()
        for k, bc in enumerate(bcs):
            r = bc.range
            self._bcs[k] = tm_condition(tm_range(r.block, int(r.side), 0, r.start, r.end), int(bc.kind), 0)
        self.desc = tm_mesh_desc(self._blocks, len(blocks), self._conns, len(conns), self._bcs, len(bcs))

    def ref(self):
        return C.byref(self.desc)
