/*
 * tm_hip_diag.h -- measurement and diagnostic entry points of libtm_hip.so.  NOT part of the drop-in surface (include/tm_hip.h): nothing
 * here replaces a seam of the reference, a Zig binding needs none of it.  bench.py and the tests use them; they are exported from the
 * same library so that what is measured is the product build.
 */
#ifndef TM_HIP_DIAG_H
#define TM_HIP_DIAG_H

#include "tm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Measurement support (bench.py roofline): with every = k > 0, every k-th launch of the dominant kernel (K2
 * `winslow_apply` / K2x2 / K2x3) is bracketed by a pair of HIP events recorded on the handle's stream (0 = off); read returns
 * the summed elapsed milliseconds of the bracketed launches, how many were bracketed and how many ran since the last
 * read (and resets all three). */
int tm_smoother_profile(tm_smoother* s, int every);
int tm_smoother_profile_read(tm_smoother* s, double* k2_ms_total, uint64_t* k2_launches_timed, uint64_t* k2_launches);

/* Diagnostic: the STREAM-style ceiling of this GPU at a footprint of `bytes` per array (SURVEY 8d asks for it beside the 8 TB/s
 * specification): copy (b = a: 2 x bytes moved) and triad (a = b + s c: 3 x bytes), 16 B per lane, non-temporal loads and stores --
 * the access pattern of the library's vector kernels -- averaged over `iters` launches after 3 warm-up launches; GB/s = 1e9 B/s. */
int tm_stream_probe(uint64_t bytes, int32_t iters, double* copy_GBps, double* triad_GBps);

/* Diagnostic: acos(x[i]) and atan2(y[i], x[i]) exactly as the White kernels evaluate them on the device (csrc/tm_refmath.h: the
 * reference's libm algorithm, Zig std.math = musl's, wall_control_function.zig:298-308).  Host arrays in and out. */
int tm_white_math_probe(const double* x, const double* y, uint64_t n, double* out_acos, double* out_atan2);

/* Diagnostic: ILU(0) of one CSR matrix on the device as tm_csr_solve's TM_OPT_PRECOND_ILU0 builds it -- the factor in A's own pattern into
 * lu_out [nnz] and, when rhs / z_out are given, M^-1 rhs into z_out [n] (BiCGStab.zig:178-277, 384-422).  Host arrays. */
int tm_csr_ilu0_probe(uint64_t n, const int32_t* Ap, const int32_t* Ai, const double* Ax, const double* rhs /* may be NULL */, double* lu_out,
                      double* z_out /* may be NULL */);

/* How the handle orders the two queues of a pipelined pass (interior pass on its stream, perimeter-row chain + halo exchange on a second,
 * high-priority stream of its own): counters in device memory with one-wave announce / wait kernels need the two streams on different
 * hardware queues, which HIP does not promise -- so the handle TESTS it once, when the second stream is created (one announce-and-wait
 * round in both directions, limit 5 ms), and falls back to hipEvent ordering when the round does not complete.
 *   -1  no two-queue schedule has run on this handle (yet)
 *    0  counters (the self-test passed)
 *    1  events: TM_PAIR_SYNC=events in the environment when the handle was created
 *    2  events: several multi-rank handles live in this process (they could block each other through shared queues)
 *    3  events: the self-test found both streams on one hardware queue */
int tm_smoother_queue_ordering(const tm_smoother* s);

/* ---- The multigrid preconditioner of TM_INNER_MG_BICGSTAB as an operator (tests/test_gpu_mg_operator.py pins it against a host reference). */

/* Diagnostic: ONE of the four stand-alone multigrid transfer kernels on host arrays, launched the way the cycle launches it (grid capping
 * included).  Interleaved x,y arrays, node (i,j) at i*nj + j.  The fine level has nif x njf nodes; a direction with its flag set is
 * coarsened to n/2 + 1 nodes, the other keeps its size.
 *   kind 0  injection      in = fine,            out = coarse (every node written):  out = (scale_x, scale_y) * in(min(2c, n-1))
 *   kind 1  restriction    in = fine residual,   x_coarse = coarse coordinates, out = coarse right-hand side: interior nodes written, the
 *                          perimeter keeps what the caller put there
 *   kind 2  prolong-add    in = coarse,          out = fine, read and written (interior nodes)
 *   kind 3  scale          in = fine,            out = fine: scale_x * in on interior nodes, 0 on the perimeter (the flags are ignored) */
int tm_mg_transfer_probe(int32_t kind, uint64_t nif, uint64_t njf, int32_t ci, int32_t cj, const double* in, const double* x_coarse /* kind 1 */,
                         double scale_x, double scale_y, double* out);

/* Diagnostic: the level hierarchy and the cycle a TM_INNER_MG_BICGSTAB handle uses for one owned block.  shape[4 l + 0..3] = ni, nj, ci, cj of
 * level l (ci / cj: coarsened from the next finer level in i / j; 0 on level 0) for l < min(*nlevels, capacity);
 * cycle[0..5] = nu_pre, nu_post, nu_coarsest, mg_dirichlet, mg_perimeter_step, mg_perimeter_sweeps.  TM_E_UNSUPPORTED without multigrid. */
int tm_smoother_mg_levels(const tm_smoother* s, uint64_t block, int32_t* nlevels, int32_t* shape, uint32_t capacity, int32_t* cycle, double* omega);

/* Diagnostic: z = M^-1 f, one application of the handle's preconditioner (Smoother::precondition) for the coordinates (and P,Q) resident in
 * the handle: the level hierarchy is refreshed from them as an outer iteration does in front of its solve (P,Q are taken as they stand),
 * no solve runs and no coordinate moves.  f, z, f_after: interleaved x,y in the handle's local node order (tm_smoother_dof nodes);
 * f_after (may be NULL) receives the device's input buffer as it stands after the application.  Single-process handles;
 * TM_E_UNSUPPORTED without multigrid. */
int tm_smoother_precondition_probe(tm_smoother* s, const double* f, double* z, double* f_after);

/* ---- The run tables of the perimeter-row launches and the strip plan of the fused level kernel (csrc/tm_edge_tables.cpp), host only: no
 * device is touched (tests/test_edge_tables_cpu.py pins them against tm_plan_build / tm_plan_local).
 * The rank-local plan is the one tm_plan_local reports (owner[b] = rank owning block b; single process: all 0, rank 0, nranks 1).
 *   table 0  every perimeter row the rank owns            3  level 1 of the coupled sweep triples: the rows of table 1, the interior nodes
 *         1  the rows that are not `fixed`                    within 4 of a side whose rows move, the depth-2 ghost rows
 *         2  table 1 + the depth-1 ghost rows              4  level 2: ... within 3, the depth-1 ghost rows      5  level 3: ... within 2
 * Per run r (flat arrays, malloc'ed, released by tm_edge_tables_free): row k < count[r] of the run sits at position first[r] + k of the run
 * order and has the local id row0[r] + k row_stride[r], columns col0[9 r + q] + k col_stride[9 r + q] (q < ncols[r]) and, kind 1 (smoothed),
 * the metric neighbours met0[4 r + q] + k met_stride[4 r + q]; gid[p] = global id of the row at position p; workgroup w serves the points
 * wg_k0[w] .. of run wg_run[w].  Table 5 also returns the strip plan (the three level tables are built together): strip s runs the tasks
 * strip_off[4 s + l] .. strip_off[4 s + l + 1] at level l + 1; task t = task[4 t + 0..3] = level (1..3), run of that level's table, first
 * point, points.  level_strip = positions of a level-3 line per strip; 0 = the library's default (60). */
typedef struct tm_edge_tables_info {
    int64_t nrows, nruns, nwg;
    int32_t *first, *count, *row0, *row_stride;        /* [nruns] */
    int32_t *col0, *col_stride;                        /* [9 nruns] */
    int32_t *met0, *met_stride;                        /* [4 nruns] */
    int32_t *kind, *ncols, *self, *flags;              /* [nruns] */
    int32_t *wg_run, *wg_k0;                           /* [nwg] */
    int64_t* gid;                                      /* [nrows] */
    int64_t nstrips, ntasks;
    int32_t *strip_off, *task;                         /* [4 nstrips], [4 ntasks] */
} tm_edge_tables_info;
int tm_edge_tables_probe(const tm_mesh_desc* mesh, const int32_t* owner, int32_t rank, int32_t nranks, int32_t table, int32_t level_strip,
                         tm_edge_tables_info* out);
void tm_edge_tables_free(tm_edge_tables_info* info);

#ifdef __cplusplus
}
#endif
#endif /* TM_HIP_DIAG_H */
