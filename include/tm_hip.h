/*
 * tm_hip.h -- C ABI of libtm_hip.so: MI355X (gfx950) structured-grid smoother for
 * turbomesh's src/core hot path (2D linear TFI seeding + Winslow/Poisson elliptic block
 * smoothing with inter-block coupling).
 *
 * Every entry point replaces one Zig-level seam of the reference (pascalPost/turbomesh);
 * the seam is cited next to the declaration as reference file:line.  The Zig binding a
 * maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers and sizes only; all host arrays are caller-owned, never retained past
 *     the call (handle API excepted: it keeps DEVICE copies only);
 *   - coordinates are Vec2d = struct{data:[2]f64} slices reinterpret-cast to double*
 *     (reference src/core/types.zig:16-37): x,y interleaved, node (i,j) at i*nj + j
 *     (types.zig:94-96), 16 B per node;
 *   - every function returns int: 0 = ok, >0 = warning status, <0 = tm_error; the message is
 *     available from tm_last_error() (pattern: cg_get_error, reference src/core/cgns.zig:19-22);
 *     nothing aborts the process;
 *   - not re-entrant per handle; no hidden global state besides the HIP runtime;
 *   - measurement and diagnostic entry points (event timing of the dominant kernel, the STREAM-style probe, the White math probe,
 *     how a handle orders its two queues) are declared in tm_hip_diag.h, not here: a binding needs none of them.
 */
#ifndef TM_HIP_H
#define TM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TM_HIP_ABI_VERSION 1

/* ------------------------------------------------------------------ errors */
typedef enum tm_error {
    TM_OK = 0,
    TM_W_NOT_CONVERGED = 1,   /* warning only, like BiCGStab.zig:368-369 / GMRES.zig:422 */
    TM_E_SIZE = -1,           /* error.InconsistentSize (tfi.zig:30)                       */
    TM_E_TOPOLOGY = -2,       /* asserts of smooth.zig:562, 627-631, 719; boundary.zig:280 */
    TM_E_MISMATCH = -3,       /* connectionDataCheck panic (smooth.zig:220-275)            */
    TM_E_OVERFLOW = -4,       /* BoundedArray overflow (smooth.zig:1191-1206)              */
    TM_E_UNSUPPORTED = -5,    /* error.ExternalSolverNotEnabled (solver.zig:48,56,82,89)   */
    TM_E_ARG = -6,
    TM_E_MEMORY = -7,
    TM_E_HIP = -8,            /* HIP runtime failure / no gfx950 device                    */
    TM_E_COMM = -9            /* exchange / all-reduce hook failed                         */
} tm_error;

const char* tm_last_error(void);
int tm_abi_version(void);

/* The reference logs two lines per outer iteration (std.log scope .smoothing): "iteration: {n}" before the fill and
 * "\tresidual: {(sum dx^2 + sum dy^2)^2}" after the solve (reference src/core/smoothing/smooth.zig:105, 136-137).  A caller
 * that wants them installs a sink: what = 0 announces iteration `iteration`, what = 1 carries its residual in `value`.
 * Process-wide like the reference's logger; NULL (the default) switches it off.  With a sink installed every outer
 * iteration ends with a reduction and a host round trip -- in TM_INNER_RELAX mode (one sweep = one outer iteration)
 * that means one sweep per kernel pass and one synchronisation per sweep, so install it for diagnosis, not for speed.
 * tm_csr_solve with TM_OPT_REFINE reports its refinement through the same sink, once per call behind the last step (`iteration` = 0):
 * what = 2: `value` = refinement steps taken (0 .. 3); what = 3 / what = 4: ||d||_2 / ||x||_2 of the last step's update for the x- / the
 * y-component (0 when no step ran); what = 5: `value` = inner iterations spent in the correction solves. */
typedef void (*tm_log_fn)(void* ctx, int32_t what, uint64_t iteration, double value);
void tm_set_log(tm_log_fn sink, void* ctx);

/* ------------------------------------------------------------------ data model
 * POD mirrors of the reference types, enum values in declaration order. */
enum { TM_SIDE_I_MIN = 0, TM_SIDE_I_MAX = 1, TM_SIDE_J_MIN = 2, TM_SIDE_J_MAX = 3 };   /* boundary.zig:8-13   */
enum { TM_BC_WALL = 0, TM_BC_INLET = 1, TM_BC_OUTLET = 2 };                              /* boundary.zig:178-182 */

typedef struct tm_range {        /* boundary.zig:15-19 */
    uint64_t block;
    uint32_t side;
    uint32_t _pad;
    uint64_t start, end;         /* inclusive; start > end = reversed */
} tm_range;

typedef struct tm_connection {   /* boundary.zig:119-123 */
    tm_range r[2];
    int32_t has_periodicity;     /* periodicity: ?Vec2d */
    int32_t _pad;
    double periodicity[2];       /* maps range[0] onto range[1] */
} tm_connection;

typedef struct tm_condition {    /* boundary.zig:184-187 */
    tm_range range;
    uint32_t kind;
    uint32_t _pad;
} tm_condition;

typedef struct tm_block {        /* discrete.zig:138-141 + types.zig:78-80 */
    double* xy;                  /* ni*nj*2 doubles, mutated in place by the smoother */
    uint64_t ni, nj;             /* size[0], size[1] */
} tm_block;

typedef struct tm_mesh_desc {    /* discrete.zig:166-171 (names omitted) */
    tm_block* blocks;
    uint64_t nblocks;
    tm_connection* conns;
    uint64_t nconns;
    tm_condition* bcs;
    uint64_t nbcs;
} tm_mesh_desc;

/* wall_control_function.zig:10-20, 56-68 */
/* Two kinds the reference does not have, for any topology (its stencil, smooth.zig:192-208, takes a per-node P, Q as it is):
 *   TM_CF_PRESCRIBED          the caller's field: zero after create, set with tm_smoother_set_control_function (handles only:
 *                             tm_smooth_mesh has no way to pass a field and answers TM_E_ARG)
 *   TM_CF_THOMAS_MIDDLECOFF   block-local field that keeps the boundary point distribution in the interior.  For an edge polyline
 *                             e[0..n-1]: d1 = (e[k+1] - e[k-1]) / 2, d2 = e[k+1] - 2 e[k] + e[k-1], f[k] = -(d1.d2) / (d1.d1) for
 *                             k = 1..n-2 (0 where d1.d1 == 0), f[0] = f[1], f[n-1] = f[n-2]; n < 3: f = 0.  With phi_lo / phi_hi = f of
 *                             the j = 0 / j = nj-1 edge and psi_lo / psi_hi = f of the i = 0 / i = ni-1 edge:
 *                             P[i][j] = (1-t) phi_lo[i] + t phi_hi[i], t = j/(nj-1); Q[i][j] = (1-s) psi_lo[j] + s psi_hi[j], s = i/(ni-1),
 *                             every node of every block.  Evaluated on the device from the resident coordinates at the end of
 *                             create and of tm_smoother_upload, then FROZEN over the outer iterations;
 *                             tm_smoother_update_control_function evaluates it again.  Needs no halo: works with rank hooks.
 * Both run in every inner mode; relaxation sweeps go one per kernel pass (as with White).  ds_target / theta_target are White's. */
enum { TM_CF_LAPLACE = 0, TM_CF_WHITE = 1, TM_CF_PRESCRIBED = 2, TM_CF_THOMAS_MIDDLECOFF = 3 };
typedef struct tm_control_fn {
    int32_t kind;
    int32_t _pad;
    double ds_target;
    double theta_target;
} tm_control_fn;

/* solver.zig:10-27: Tag in declaration order + the new `hip` member.  Only TM_SOLVER_HIP is
 * served by this library; the reference's own tags return TM_E_UNSUPPORTED exactly like a
 * build without -Duse-umfpack returns error.ExternalSolverNotEnabled. */
enum { TM_SOLVER_GMRES = 0, TM_SOLVER_BICGSTAB = 1, TM_SOLVER_UMFPACK = 2, TM_SOLVER_PETSC = 3, TM_SOLVER_HIP = 4 };
/* inner strategy of the hip solver */
enum {
    TM_INNER_BICGSTAB = 0,   /* Picard outer iteration (smooth.zig:104-154), each frozen-coefficient system solved by
                                matrix-free BiCGStab on the row-equilibrated operator D^-1 A (replaces BiCGStab.zig:279-370) */
    TM_INNER_RELAX = 1,      /* every outer iteration is ONE fused Jacobi elliptic sweep X <- X + omega D^-1 (b - A(X) X)   */
    TM_INNER_MG_BICGSTAB = 2,/* TM_INNER_BICGSTAB, right-preconditioned by one geometric-multigrid V(2,2) cycle per block
                                (damped Jacobi, full weighting, rediscretised Winslow operator on vertex-coarsened levels;
                                the perimeter rows are applied to the interior corrections behind the cycles).  Same Picard iterates, far fewer inner iterations on
                                large blocks: what makes "to 1e-8 residual at 4096^2" practical               */
    TM_INNER_GMRES = 4,      /* the Picard outer iteration with the reference's OTHER Krylov solver restated on the device: restarted GMRES(30),
                                left-preconditioned with the diagonal, modified Gram-Schmidt Arnoldi, Givens rotations (GMRES.zig:300-423,
                                510-524; restart 30 as GMRES.zig:21).  Same scale-aware stop test as TM_INNER_BICGSTAB.  What a front end
                                maps "solver": {"gmres": {"preconditioner": "diagonal"}} of an input file to; ILU(0) (GMRES.zig:199-298) is served
                                on the assembled system -- tm_csr_solve and TM_INNER_REFERENCE_GMRES -- the matrix-free modes use the diagonal */
    TM_INNER_REFERENCE_GMRES = 5, /* the reference's route as its example inputs write it ("gmres" + "ilu0"), same algorithm, same tolerances: per outer
                                iteration system.fill into a device-resident CSR (the reference's assembled, UNSCALED system, bit for bit), then
                                GMRES(30) left-preconditioned with ILU(0) (TM_OPT_PRECOND_ILU0; factor and substitutions bit-identical to
                                GMRES.zig:199-298, 437-475) or with the diagonal (flag clear), mat-vec in CSR order, stop test
                                ||M^-1 (b - A x)|| <= max(atol, rtol ||b||_2) per component on the unscaled b (GMRES.zig:305-306, 319, 388).
                                Defaults in this mode: rtol 0 -> 1e-6, atol 0 -> 1e-8, max_inner 0 -> 1000 per component and solve
                                (GMRES.zig:21-24), check_every 0 -> 1.  The iterates are the REFERENCE's (they differ from the exact-solve
                                iterates of the other modes by what its loose stop test leaves: 1e-7 .. 2e-5 RMS); what differs from a run of
                                the reference is the summation order of dot products and norms.  Nothing travels to or from the host per
                                iteration but the flags.  Single-process handles only (rank hooks: TM_E_UNSUPPORTED at create and in
                                tm_smoother_workspace_bytes); its buffers are allocated at create (TM_E_MEMORY there, not in a solve)      */
    TM_INNER_AUTO = 3        /* resolved when the handle is created, from the mesh alone (every rank of a job decides alike):
                                TM_INNER_MG_BICGSTAB when the largest block has >= 100 000 nodes, TM_INNER_BICGSTAB below -- on the
                                reference's example meshes (T106 / LS89: 8 blocks of 10^2..10^4 nodes) every multigrid level is a handful
                                of launch-bound kernels and the plain solver is 7x faster in wall time; from ~300^2 nodes per block on
                                the cycle's O(1) iteration count wins; blocks that no connection couples take
                                the cycle from 1000 nodes on (it is block-local: a lone block needs ~25 iterations at any size, coupled
                                blocks hundreds).  A single-process handle (no rank hooks)
                                also looks at the coordinates it is given: where the cells' aspect ratio varies strongly INSIDE a block
                                (standard deviation of log(|x_xi|^2 / |x_eta|^2) over the block's nodes above 1: boundary-layer
                                clustering) the point-Jacobi cycle is a poor preconditioner and the plain solve is chosen at any size.
                                Same Picard iterates either way.                                                                    */
};
/* tm_solver_opt.flags */
enum {
    TM_OPT_SINGLE_SWEEP = 1, /* TM_INNER_RELAX: one kernel pass per sweep.  Default (bit clear): sweeps are taken three per pass
                                on blocks whose perimeter rows are all `fixed`, two per pass on coupled blocks (same arithmetic,
                                bit-identical coordinates, a third / half of the HBM traffic) */
    TM_OPT_EAGER_SCALARS = 2, /* Krylov modes: the textbook launch sequence of BiCGStab.zig:279-370 -- one kernel per vector update, one
                                scalar-update launch per reduction.  Default (bit clear) on single-process handles: the vector updates
                                are formed inside the two operator applications (two kernels per iteration; rho from r_hat.s -
                                omega r_hat.t, equal in exact arithmetic) and, on small meshes, the scalar steps travel with the
                                kernels that consume them.  Same method, iterates equal to rounding */
    TM_OPT_PRECOND_ILU0 = 8, /* tm_csr_solve and TM_INNER_REFERENCE_GMRES ONLY (the two places that have the assembled matrix): ILU(0) -- the reference's second preconditioner
                                (preconditioner.zig:1-4; BiCGStab.zig:178-277, 384-422) -- as right preconditioner of the device BiCGStab: factor
                                and substitutions level by level on the device, bit-identical to the reference's recurrence (left preconditioner of
                                GMRES(30) in TM_INNER_REFERENCE_GMRES).  The matrix-free inner strategies answer TM_E_UNSUPPORTED: they never
                                assemble a matrix to factorise                                                                          */
    TM_OPT_REFINE = 16,      /* iterative refinement of every inner solve.  Up to 3 times behind the solve: r = b - A x in double-double arithmetic,
                                rounded once to fp64 (the kernel of tm_csr_residual); A d = r solved from d = 0 by the same solver and
                                preconditioner, stop test relative to ||D^-1 r|| with the mode's own rtol (the stall guard ends a correction that
                                cannot get there); x <- x + d in fp64.  Stops early behind a step with ||d||_2 <= 2^-52 ||x||_2 in both components.
                                The result is the exact solution of the system rounded to fp64, within an ulp or two at the top of its range,
                                where the plain solve leaves conditioning x rtol.
                                tm_csr_solve: all four solver x preconditioner combinations, on the caller's A and b; stats count the correction
                                iterations too, the figures of the refinement reach the caller through tm_set_log (what = 2 .. 5).
                                Handles: TM_INNER_BICGSTAB, TM_INNER_MG_BICGSTAB, TM_INNER_GMRES (TM_INNER_AUTO resolves first), single process.
                                Per outer iteration the handle fills the reference-order assembled system of the frozen coordinates
                                (tm_smoother_assemble_csr: the reference's matrix bit for bit; allocated at create) and refines the solution
                                against THAT system and its right-hand side -- the refined Picard iterate is defined by the reference's matrix,
                                not by the factored matrix-free operator, on which the corrections run (coefficients within 16 eps: harmless for
                                a correction).  Residual and copy-back, the White update, tm_stats and iterate_until* are as without the flag;
                                tm_smoother_refine_report has the figures.  TM_E_UNSUPPORTED at create, in tm_smoother_workspace_bytes and in
                                tm_smooth_mesh with TM_INNER_RELAX (no solve to refine), TM_INNER_REFERENCE_GMRES (its contract is the
                                reference's loose stop test), TM_OPT_RTOL_INITIAL (inexact Picard by intent) and rank hooks (the assembled system
                                is single-process).  Flag clear: not one launch more, bit-identical results                                  */
    TM_OPT_RTOL_INITIAL = 4  /* Krylov modes: `rtol` is relative to the INITIAL residual of each inner solve (inexact Picard: stop at
                                ||D^-1(b-Ax)|| <= max(atol, rtol ||D^-1(b-A x0)||), rtol = 0 -> 1e-2) instead of ||D^-1 b||.  Every solve then
                                does work in proportion to what is left -- same fixed point, several times fewer inner iterations on the way
                                (tools/converge_probe.py); the Picard ITERATES are no longer the exact-solve ones, so parity per iterate is
                                a statement about the default mode only */
};
typedef struct tm_solver_opt {
    int32_t tag;             /* TM_SOLVER_* */
    int32_t inner;           /* TM_INNER_* */
    double rtol;             /* stop the inner solve at ||D^-1(b-Ax)||_2 <= max(atol, rtol*||D^-1 b||_2); 0 -> size-aware default: 7.5e-9 / nodes clamped to [1e-16, 1e-14] (1e-14 up to 866^2 nodes; the error of the solve is conditioning x residual and the conditioning grows with the mesh); 1e-14 at every size with the multigrid preconditioner, which makes the conditioning O(1) */
    double atol;             /* 0 -> 0 */
    uint64_t max_inner;      /* BiCGStab iteration cap per Picard solve; 0 -> max(10000, 12 sqrt(nodes)) (the reference caps at 1000, BiCGStab.zig:19, with its far looser stop test) */
    uint32_t check_every;    /* host convergence poll interval in inner iterations; 0 -> 8 (1 with the multigrid preconditioner) */
    uint32_t flags;          /* TM_OPT_* bits; 0 = defaults */
    double omega;            /* relaxation factor of TM_INNER_RELAX; 0 -> 1.0 */
} tm_solver_opt;

typedef struct tm_stats {
    uint64_t outer_iterations;
    uint64_t inner_iterations;   /* BiCGStab iterations summed over the outer iterations (both components advance together) */
    uint64_t operator_sweeps;    /* applications of the 9-point operator to the whole mesh */
    double last_residual;        /* (sum dx^2 + sum dy^2)^2 of the last outer iteration, smooth.zig:136 */
    double last_dx2, last_dy2;   /* sum (x_old-x_new)^2, sum (y_old-y_new)^2, smooth.zig:112-134 */
    double scaled_residual_rms;  /* sqrt(||D^-1(b - A(X)X)||^2 / (2*dof)) at the start of the last outer iteration */
    double seconds;              /* wall time of the call, like smooth.zig:156-160 */
    int32_t not_converged;       /* inner solves that hit max_inner */
    int32_t _pad;
} tm_stats;

/* ------------------------------------------------------------------ seam 3: TFI
 * Replaces tfi.linear2dBoundaryBlendedControlFunction (reference src/core/tfi.zig:112-208),
 * called from Block2d.init (src/core/discrete.zig:146-157).  Host pointers; xy_out[ni*nj*2]
 * is overwritten for ALL nodes (boundary nodes included, tfi.zig:164-205).
 * s1,s2 [ni] / t1,t2 [nj]: clusterings of the i_min,i_max / j_min,j_max edges, first 0, last
 * exactly 1 (tfi.zig:135-145) else TM_E_ARG; corner points must agree within 1e-10
 * (tfi.zig:150-162) else TM_E_MISMATCH. */
int tm_tfi_block(double* xy_out, uint64_t ni, uint64_t nj,
                 const double* x_i_min, const double* x_i_max,   /* ni*2 each */
                 const double* x_j_min, const double* x_j_max,   /* nj*2 each */
                 const double* s1, const double* s2, const double* t1, const double* t2);

/* Replaces tfi.linear2d (reference src/core/tfi.zig:19-67): plain TFI, xi=i/(ni-1), eta=j/(nj-1),
 * corners from the i edges. */
int tm_tfi_linear2d(double* xy_out, uint64_t ni, uint64_t nj,
                    const double* e_i_min, const double* e_i_max, const double* e_j_min, const double* e_j_max);

/* ------------------------------------------------------------------ seam 1: whole smoother
 * Replaces smooth.mesh(allocator, *Mesh, iterations, solver.Option, Algorithm)
 * (reference src/core/smoothing/smooth.zig:74-80); callers gui/main.zig:52, wasm/lib.zig:46-52.
 * Mutates mesh->blocks[b].xy in place.  iterations == 0 is legal and leaves the mesh untouched. */
int tm_smooth_mesh(const tm_mesh_desc* mesh, uint64_t iterations, const tm_solver_opt* opt,
                   const tm_control_fn* cf, tm_stats* stats /* may be NULL */);

/* ------------------------------------------------------------------ seam 2: the linear-solver slot
 * Replaces a backend of solver.Solver (reference src/core/smoothing/solver.zig:40-93; pattern umfpack.zig:18-55): the
 * caller has ASSEMBLED RowCompressedMatrixSystem2d (smooth.zig:277-307) and hands over its CSR arrays -- Ap = lhs_p[n+1],
 * Ai = lhs_i, values = lhs_values -- with both right-hand sides and the solution vectors x_new / y_new, which carry the
 * initial guess in and the solution out (warm start, BiCGStab.zig:136-153).  The x- and the y-system share the pattern and
 * differ in the two entries of every sliding row (system.fillXSpecific / fillYSpecific, smooth.zig:1115-1165): pass the
 * values after fillXSpecific as Ax_x and a copy taken after fillYSpecific as Ax_y (NULL = same values for both; exact
 * whenever the mesh has no inlet / outlet condition).  Both components are solved together on the device by BiCGStab
 * -- or, with opt->inner == TM_INNER_GMRES, by the reference's restarted GMRES(30) (GMRES.zig:300-423), left-preconditioned; with
 * TM_OPT_PRECOND_ILU0 in opt->flags either of them takes ILU(0) instead of the diagonal: the four combinations of solver.zig:18-27 --
 * on D^-1 A with the stop test of tm_solver_opt (rtol, atol, max_inner, check_every; opt may be NULL = defaults; rtol 0 -> 1e-14 here at
 * every size: the size-aware default belongs to the matrix-free path's own operator).  A recurrence residual that fails to halve over
 * max(4000, 4 sqrt(n)) iterations ends the solve as not converged.
 * Returns TM_OK, TM_W_NOT_CONVERGED (warning, like BiCGStab.zig:368-369) or a negative error; host pointers throughout;
 * the matrix is uploaded per call -- this is the faithful "reference-assembled, GPU-solved" mode, not the fast path
 * (that is seam 1, which never assembles a matrix). */
int tm_csr_solve(uint64_t n, const int32_t* Ap, const int32_t* Ai, const double* Ax_x, const double* Ax_y /* may be NULL */,
                 const double* bx, const double* by, double* x /* in: guess, out */, double* y, const tm_solver_opt* opt /* may be NULL */,
                 tm_stats* stats /* may be NULL */);

/* The residual of ANY solution of such a system -- this library's or not: r = b - A x per component, every product a_ij x_j formed exactly,
 * the sum carried in double-double arithmetic (an unevaluated pair of doubles, error-free additions) with b in the same sum, rounded once to
 * fp64.  Same arguments as tm_csr_solve (host pointers; Ax_y NULL = the x values for both); rx / ry [n] receive the residuals.  Valid for
 * finite inputs whose products neither overflow nor fall into the subnormal range: there
 *     |r_i - exact| <= 2^-53 |r_i| + (nnz_i + 1) 2^-104 (sum_j |a_ij x_j| + |b_i|)
 * however much cancels (an fp64 residual of a good solution is wrong in every digit); outside it the result is an fp64 residual's. */
int tm_csr_residual(uint64_t n, const int32_t* Ap, const int32_t* Ai, const double* Ax_x, const double* Ax_y /* may be NULL */,
                    const double* bx, const double* by, const double* x, const double* y, double* rx, double* ry);

/* ------------------------------------------------------------------ persistent handle
 * Same smoother with the coordinates resident in HBM between calls (for callers that iterate,
 * inspect, iterate ...).  create uploads the mesh; iterate runs `iterations` outer iterations on
 * the device; download writes the current coordinates back into the caller's arrays. */
typedef struct tm_smoother tm_smoother;

/* Optional hooks that make ONE rank of a multi-GPU job out of a handle (one process per GPU):
 * the mesh description handed to create() is the GLOBAL topology, `owner[b]` names the rank
 * that owns block b, only owned blocks need coordinates.  exchange() must fill recv_buf (device)
 * from the peers' send_buf (device) according to the plan returned by tm_smoother_exchange_plan;
 * allreduce_sum() sums n doubles in place (device) over all ranks.  Every call names the stream it must be ordered on:
 * the handle's stream, or -- for the exchanges of relaxation sweep pairs -- a second stream the handle owns, on which the
 * exchanges and perimeter rows run beside the interior pass. */
typedef struct tm_comm_hooks {
    void* ctx;
    int32_t rank, nranks;
    const int32_t* owner;   /* [nblocks] */
    int (*exchange)(void* ctx, const double* send_buf, double* recv_buf, void* stream);
    int (*allreduce_sum)(void* ctx, double* buf, int32_t n, void* stream);
    /* Optional split form: when exchange_wait != NULL, exchange() only STARTS the transfer (it may return before the
     * ghost rows have arrived) and exchange_wait() makes `stream` wait for it.  The library then runs the interior-row
     * kernel K2 -- which never reads ghost rows -- between the two, hiding the transfer behind it. */
    int (*exchange_wait)(void* ctx, void* stream);
    /* Optional caller-provided device memory (e.g. a torch tensor, so the hooks can hand views of it to
     * torch.distributed): when workspace != NULL every device buffer of the handle is carved from it.
     * Size it with tm_smoother_workspace_bytes. */
    void* workspace;
    uint64_t workspace_bytes;
} tm_comm_hooks;
/* Device bytes a handle for this mesh/options/partition needs (hooks may be NULL = single process). */
int tm_smoother_workspace_bytes(const tm_mesh_desc* mesh, const tm_solver_opt* opt, const tm_control_fn* cf,
                                const tm_comm_hooks* hooks, uint64_t* bytes);

int tm_smoother_create(const tm_mesh_desc* mesh, const tm_solver_opt* opt, const tm_control_fn* cf,
                       const tm_comm_hooks* hooks /* NULL = single process */, void* stream /* hipStream_t or NULL */,
                       tm_smoother** out);
int tm_smoother_iterate(tm_smoother* s, uint64_t iterations, tm_stats* stats);
/* Outer iterations until the scaled nonlinear residual stats->scaled_residual_rms = sqrt(||D^-1 (b - A(X) X)||^2 / (2 dof)) is
 * <= scaled_residual_tol, at most max_iterations of them (the reference iterates a fixed count from its input file,
 * smooth.zig:104; it has no stop test).  TM_OK = reached; TM_W_NOT_CONVERGED = max_iterations hit or an inner solve did not
 * converge.  stats->outer_iterations = iterations actually performed (Picard: solves; relax: sweeps, tested every 32). */
int tm_smoother_iterate_until(tm_smoother* s, uint64_t max_iterations, double scaled_residual_tol, tm_stats* stats);
/* ... until the update of the last outer iteration, sqrt((sum dx^2 + sum dy^2) / nodes) over the whole mesh, is <= update_rms_tol:
 * the quantity the reference forms and logs per iteration (smooth.zig:112-137) -- convergence of the COORDINATES.  Returns
 * TM_W_NOT_CONVERGED when max_iterations ran out first (stats are valid either way). */
int tm_smoother_iterate_until_update(tm_smoother* s, uint64_t max_iterations, double update_rms_tol, tm_stats* stats);
int tm_smoother_download(tm_smoother* s, const tm_mesh_desc* mesh);
int tm_smoother_upload(tm_smoother* s, const tm_mesh_desc* mesh);
void tm_smoother_destroy(tm_smoother* s);

/* Built-in transport for the hooks above: RCCL point-to-point (xGMI) + all-reduce issued by the library itself, so that no
 * host-language callback sits in the sweep loop.  librccl is dlopen'ed: pass the path of the copy the process already uses
 * (e.g. <torch>/lib/librccl.so) or NULL for the default search.  Rank 0 calls tm_rccl_unique_id and hands the 128 bytes
 * to the other ranks by whatever rendezvous the host has (torch.distributed broadcast, MPI, a file); every rank then calls
 * tm_rccl_comm_create (collective) with the current HIP device set.  tm_rccl_hooks fills `hooks` for a mesh partition:
 * exchange/exchange_wait = grouped ncclRecv/ncclSend per neighbouring rank on a side stream, fenced with events against
 * the handle's stream; allreduce_sum = ncclAllReduce.  The hooks (and hooks->owner) stay valid while `comm` lives. */
typedef struct tm_rccl_comm tm_rccl_comm;
#define TM_RCCL_ID_BYTES 128
int tm_rccl_unique_id(const char* librccl_path, void* id_out /* TM_RCCL_ID_BYTES */);
int tm_rccl_comm_create(const char* librccl_path, const void* id, int32_t rank, int32_t nranks, tm_rccl_comm** out);
void tm_rccl_comm_destroy(tm_rccl_comm* comm);
int tm_rccl_hooks(tm_rccl_comm* comm, const tm_mesh_desc* mesh, const int32_t* owner /* [nblocks] */, tm_comm_hooks* hooks);
/* The same when the options of the handle the hooks are for are known (pass the very structures given to tm_smoother_create): a handle that
 * never runs sweep triples -- the Krylov modes, any control function but laplace, TM_OPT_SINGLE_SWEEP -- then exchanges the depth-2 halo only
 * (tm_rccl_hooks sizes its tables by the topology alone: depth 3 wherever every block has at least 16 x 16 nodes, whatever the handle does with it).
 * A handle created with the library's own hooks follows the depth their tables were built for. */
int tm_rccl_hooks_for(tm_rccl_comm* comm, const tm_mesh_desc* mesh, const int32_t* owner, const tm_solver_opt* opt, const tm_control_fn* cf /* NULL = laplace */,
                      tm_comm_hooks* hooks);

/* The table tm_rccl_hooks builds for a rank, host-only (no communicator, no GPU): per neighbouring rank the offset and count
 * (rows of 16 B) handed to ncclSend / ncclRecv in one group per exchange.  Pairwise symmetry -- send_cnt of a towards b ==
 * recv_cnt of b from a, peers mutual, offsets inside send_rows / recv_rows -- is what keeps ncclGroupEnd from hanging; a caller
 * (or a test) can check it for every rank of a partition before any process joins a communicator.
 * send_off indexes the rank's own vector when direct_send (n_owned + n_ghost rows), the packed send buffer otherwise. */
typedef struct tm_rccl_peer_table {
    int32_t npeers, direct_send;
    int64_t send_rows, recv_rows;   /* extent of the buffers the offsets index */
    int32_t* peer;                  /* [npeers] ascending                      */
    int64_t *send_off, *send_cnt, *recv_off, *recv_cnt;   /* [npeers] each      */
} tm_rccl_peer_table;
int tm_rccl_peer_table_build(const tm_mesh_desc* mesh, const int32_t* owner, int32_t rank, int32_t nranks, tm_rccl_peer_table* out);
void tm_rccl_peer_table_free(tm_rccl_peer_table* table);

/* Exchange plan of a handle created with hooks: npeers peers; for peer k, send_count[k] rows
 * (16 B each) start at send_offset[k] rows into send_buf, same for recv.  Rows are double2.
 * send_buf is a packed buffer -- or, when every peer's rows are one contiguous run of the rank's vector (interfaces along
 * whole block rows), the vector itself, with send_offset[k] the run's first row: no pack kernel runs then.  Either way the
 * hook sends send_count[k] rows from send_buf + send_offset[k]. */
int tm_smoother_exchange_plan(const tm_smoother* s, int32_t* npeers, const int32_t** peer_rank,
                              const int64_t** send_offset, const int64_t** send_count,
                              const int64_t** recv_offset, const int64_t** recv_count);

/* Introspection used by the parity tests (and by a Zig caller that wants the operator only):
 * out = A(X) * in over the rank's owned rows, A assembled matrix-free from the CURRENT device
 * coordinates; scaled != 0 applies the row equilibration D^-1.  in/out are host arrays with
 * 2*dof doubles in global row order (smooth.zig:1643-1645).  Single-process handles only. */
int tm_smoother_apply(tm_smoother* s, const double* in_xy, double* out_xy, int scaled);
/* The system of the CURRENT device coordinates as the reference ASSEMBLES it -- RowCompressedMatrixSystem2d (smooth.zig:277-385: lhs_p,
 * lhs_i in the reference's column order) filled by system.fill (smooth.zig:923-1113) on the device: interior rows StencilData.init's nine
 * values in the reference's expression order (smooth.zig:171-216), perimeter rows from the plan; Ax_x / Ax_y = lhs_values after fillXSpecific
 * / fillYSpecific (smooth.zig:1115-1165).  Ap [dof + 1], Ai / Ax_x / Ax_y [nnz]; any of them may be NULL (all NULL: *nnz only); the
 * right-hand sides come from tm_smoother_rhs.  What a Zig caller gets from its own system.fill -- the arrays tm_csr_solve takes -- and what
 * the parity tests compare with the faithful oracle bit for bit.  Single-process handles only. */
int tm_smoother_assemble_csr(tm_smoother* s, int32_t* Ap, int32_t* Ai, double* Ax_x, double* Ax_y, uint64_t nnz_capacity, uint64_t* nnz);
/* out = A(X) * in evaluated THROUGH that assembled system: every row the sum of its products in CSR order, un-fused -- the reference's own
 * mat-vec (BiCGStab.zig:424-435) bit for bit, interior rows included.  (tm_smoother_apply is the matrix-free fast path: the same perimeter
 * rows, interior rows in a factored form within 16 eps sum |c_k w_k| of this.)  Single-process handles only. */
int tm_smoother_apply_reference_order(tm_smoother* s, const double* in_xy, double* out_xy);
/* Right-hand side b (2*dof doubles) for the current coordinates (smooth.zig:780-921, 1060-1061). */
int tm_smoother_rhs(tm_smoother* s, double* rhs_xy);
/* r = b - A(X) xy by the kernel of tm_csr_residual, against the system ASSEMBLED from the resident coordinates X (tm_smoother_assemble_csr:
 * the reference's matrix bit for bit) and its right-hand side (tm_smoother_rhs), nothing leaving the device but the result: how far a
 * field is from solving the frozen-coefficient system of the current coordinates.  xy: 2*dof doubles in global row order, NULL = the
 * resident coordinates themselves (the nonlinear residual of the mesh); r_xy: 2*dof doubles.  Single-process handles only. */
int tm_smoother_residual(tm_smoother* s, const double* xy /* NULL = the resident coordinates */, double* r_xy);
/* What the refinement of a handle created with TM_OPT_REFINE did (TM_E_UNSUPPORTED without the flag); any pointer may be NULL. */
int tm_smoother_refine_report(const tm_smoother* s, uint32_t* steps_x_y /* [2]: steps of the last outer iteration (both components advance together) */,
                              double* last_update_rel /* [2]: ||d||_2 / ||x||_2 of its last step */,
                              uint64_t* correction_iterations /* inner iterations spent in corrections, summed over the handle's life */);
/* Row kind per global row: -1 interior, else BlockBoundaryPointKind (smooth.zig:1168-1174). */
int tm_smoother_row_kinds(const tm_smoother* s, int32_t* kinds /* [dof] */);
uint64_t tm_smoother_dof(const tm_smoother* s);
/* The inner strategy the handle runs (TM_INNER_*): what TM_INNER_AUTO resolved to, else the option as given. */
int tm_smoother_inner(const tm_smoother* s);
/* Inner iterations of the LAST outer iteration per component (x, y): the reference solves the two systems one after the other and each has
 * its own count (solver.zig:69-78).  TM_INNER_REFERENCE_GMRES: the columns each component built; the older Krylov modes, where both
 * components advance together: the common count twice; TM_INNER_RELAX answers 0, 0. */
int tm_smoother_inner_counts(const tm_smoother* s, uint64_t* x_iterations, uint64_t* y_iterations);
/* Current control function (P,Q) per node, 2*dof doubles (wall_control_function.zig:22-54). */
int tm_smoother_control_function(tm_smoother* s, double* pq);
/* Replace the resident field; same layout and extent as the getter above (2 doubles per owned node, owned blocks in order).
 * TM_CF_PRESCRIBED and TM_CF_THOMAS_MIDDLECOFF handles (there it overrides the evaluated field until the next
 * tm_smoother_update_control_function or tm_smoother_upload); TM_E_UNSUPPORTED on laplace and White handles.  A non-finite
 * entry: TM_E_ARG, the resident field unchanged.  Everything that depends on the field follows at the next call. */
int tm_smoother_set_control_function(tm_smoother* s, const double* pq);
/* Evaluate the Thomas-Middlecoff field again from the coordinates as they are now (TM_CF_THOMAS_MIDDLECOFF handles; the other
 * three kinds: TM_E_UNSUPPORTED). */
int tm_smoother_update_control_function(tm_smoother* s);

/* ------------------------------------------------------------------ export (the step right after the path)
 * The reference's structured output hands the writer one plane per coordinate with i fastest: plane[j*ni + i] =
 * block(i,j) (reference src/core/cgns.zig:75-104, called from discrete.zig:197-216 Mesh.write and smooth.zig:396-414);
 * optionally the control function as planes "P" and "Q" (cgns.zig:106-154).  Both entry points do that de-interleaving
 * transpose on the device.  tm_export_soa: host block in, host planes out.  tm_smoother_export_soa: planes of an owned
 * block from the coordinates resident in the handle; p, q may both be NULL (laplace exports zeros). */
int tm_export_soa(const double* xy /* ni*nj*2 */, uint64_t ni, uint64_t nj, double* x_out /* ni*nj */, double* y_out /* ni*nj */);
int tm_smoother_export_soa(tm_smoother* s, uint64_t block, double* x, double* y, double* p, double* q);

/* ------------------------------------------------------------------ mesh quality
 * Is the mesh usable?  One read of the coordinates gives, per block and for the whole mesh: folded and degenerate cells, the
 * scaled Jacobian with its worst cell and a histogram, corner angles, aspect ratio, edge growth and areas.  (The reference has no
 * such report.)  Cell (i, j), 0 <= i < ni-1, 0 <= j < nj-1, has corners A = (i,j), B = (i+1,j), C = (i+1,j+1), D = (i,j+1); at each
 * corner u = next - corner, v = previous - corner in the order A B C D.  All arithmetic IEEE fp64, nothing fused.
 *   per corner   J = u.x*v.y - u.y*v.x;  P = (u.x*u.x + u.y*u.y) * (v.x*v.x + v.y*v.y);  s = J / sqrt(P);  c = (u.x*v.x + u.y*v.y) / sqrt(P)
 *   cell area    a = 0.5*((C.x-A.x)*(D.y-B.y) - (D.x-B.x)*(C.y-A.y))
 *   orientation  o = sign(sum a) over the block's cells (blocks of one mesh differ in handedness); 0 when |sum a| <= cells * 2^-53 * sum |a|,
 *                and then everything is reported as for +1
 *   classes      degenerate: a corner with P == 0 or a non-finite P or J;  else inverted: min over corners of o*J <= 0;  else valid
 *   min_scaled_jacobian   min of o*s over the corners of non-degenerate cells, (worst_block, worst_i, worst_j) its cell, ties to the
 *                lowest (block, i, j); NaN and 0, 0, 0 when every cell is degenerate
 *   hist[k]      valid cells with k/10 <= m < (k+1)/10, m the cell's min o*s; m >= 0.9 in hist[9]; sum hist == cells - inverted - degenerate
 *   angles       from the largest / smallest c (clamped to [-1, 1]) over corners of non-degenerate cells, acos taken once on the host
 *   max_aspect   max over non-degenerate cells of max(li, lj) / min(li, lj), li = |AB| + |DC|, lj = |AD| + |BC|
 *   max_growth_i / _j   max of max(l0, l1) / min(l0, l1) over pairs of consecutive edges along every grid line of that direction, boundary
 *                lines included, pairs with a zero-length edge skipped; 1.0 with fewer than two edges along the direction.  Inside
 *                blocks only: growth across a connection is not reported
 *   areas        min_area / max_area: o*a over non-degenerate cells; total_area = o * sum a
 * `total`: counts and hist summed, extremes combined, total_area summed, the worst cell the one with the smallest value,
 * orientation the blocks' common one or 0.  A block with ni < 2 or nj < 2: TM_E_SIZE. */
typedef struct tm_quality {              /* 208 bytes */
    uint64_t cells, inverted, degenerate;
    int32_t  orientation, _pad;
    double   min_scaled_jacobian;
    uint64_t worst_block, worst_i, worst_j;
    double   min_angle_deg, max_angle_deg;
    double   max_aspect, max_growth_i, max_growth_j;
    double   min_area, max_area, total_area;
    uint64_t hist[10];
} tm_quality;

/* host coordinates in, evaluated on the device */
int tm_mesh_quality(const tm_mesh_desc* mesh, tm_quality* per_block /* [nblocks], may be NULL */, tm_quality* total /* may be NULL */);
/* the same definitions evaluated on the host: no GPU touched, works in a process without a device.  Every field equals the device's
 * bit for bit but total_area (a sum: equal within cells * 2^-53 * sum |a|) */
int tm_mesh_quality_host(const tm_mesh_desc* mesh, tm_quality* per_block, tm_quality* total);
/* coordinates resident in the handle; does not modify them nor any solver state.  On a handle with rank hooks the records of
 * blocks the rank does not own are zeroed and `total` covers the OWNED blocks only: there is no all-reduce -- combine the ranks'
 * records on the host if the whole mesh is wanted.  The buffers (a few KB of partial records, one cell plane for the field) are
 * allocated on first use with the HIP allocator, outside a caller-provided workspace, and freed by tm_smoother_destroy. */
int tm_smoother_quality(tm_smoother* s, tm_quality* per_block, tm_quality* total);
/* per-cell minimum of o*s of an owned block, i fastest like the export planes: out[j*(ni-1)+i]; NaN for degenerate cells */
int tm_smoother_quality_field(tm_smoother* s, uint64_t block, double* min_scaled_jacobian /* (ni-1)*(nj-1) */);

/* ------------------------------------------------------------------ 3-D from 2-D cuts
 * The reference's first open roadmap item is "extension to 3D based on meshed 2d cuts", its second "rotational configurations".  A
 * layer k of a 3-D block is a fixed linear combination of the same node in the K cuts:
 *     v[k][i][j] = sum_c A[k][c] * v_c[i][j]
 * A is an nlayers x ncuts weight matrix that depends only on the span positions.  It is not per node.
 * Inputs:
 *   - Cut span coordinates z[0..K-1] are finite and strictly increasing, with 2 <= K <= TM_STACK_MAX_CUTS = 16.
 *   - Layer coordinates s[0..nk-1] are finite, each in [z[0], z[K-1]], with nk >= 1.  No order is required.
 *   - Any violation answers TM_E_ARG.  There is no extrapolation.
 * Weights:
 *   - If s[k] == z[c] in fp64, the weight row is exactly the unit vector e_c.  A layer at a cut then reproduces the cut, numerically
 *     equal in both coordinates.
 *   - Otherwise c is the largest index <= K-2 with z[c] <= s, and h = z[c+1] - z[c].
 *   - TM_STACK_LINEAR: t = (s - z[c])/h, A[c] = 1 - t, A[c+1] = t.
 *   - TM_STACK_CUBIC: the natural cubic spline through the cuts, with zero second derivative at both end cuts.  With a = (z[c+1]-s)/h
 *     and b = (s-z[c])/h: S = a v_c + b v_{c+1} + ((a^3-a) M_c + (b^3-b) M_{c+1}) h^2/6.  The second derivatives M are linear in v, so
 *     S is a weight row.  At K = 2 it equals linear.
 *   - Weights are formed on the host in long double and rounded once to fp64.
 * Mappings:
 *   - TM_STACK_PLANAR: the output is (x, y, s[k]).  The third coordinate is s[k] itself, stored and not computed.
 *   - TM_STACK_CYLINDRICAL: the cuts are unrolled cylinders (x, r theta) at radius z[c] > 0.  Any z[c] <= 0 answers TM_E_ARG.  Per cut,
 *     theta_c = y_c / z[c] with one rounding.  x and theta are interpolated with A.  The output is (x, r sin theta, r cos theta) with
 *     r = s[k].
 * Output:
 *   - Per block and per layer window [k_begin, k_begin + k_count), three planes X, Y, Z in PLOT3D order.
 *   - Element ((k - k_begin)*nj + j)*ni + i, with i fastest.  This is the same transposition K8 (k_soa_planes) does for 2-D.
 * Every sum runs over c = 0 .. K-1 in that order, products and sums rounded separately (nothing fused), on the device and on the host. */
#define TM_STACK_MAX_CUTS 16
enum { TM_STACK_LINEAR = 0, TM_STACK_CUBIC = 1 };
enum { TM_STACK_PLANAR = 0, TM_STACK_CYLINDRICAL = 1, TM_STACK_REVOLUTION = 2 /* needs tm_stack_surfaces: see below */ };
typedef struct tm_stack_opt {
    uint64_t ncuts;
    const double* span;      /* [ncuts] z */
    uint64_t nlayers;
    const double* layers;    /* [nlayers] s */
    int32_t interpolation;   /* TM_STACK_LINEAR / TM_STACK_CUBIC */
    int32_t mapping;         /* TM_STACK_PLANAR / TM_STACK_CYLINDRICAL (TM_STACK_REVOLUTION: the *_surf calls only) */
} tm_stack_opt;
/* the weight matrix, nlayers * ncuts doubles, row = layer.  Host only: no GPU touched */
int tm_stack_weights(const tm_stack_opt* opt, double* weights);
/* Block `block` of K meshes given on the host (cuts[c]->blocks[block].xy): uploads the K copies of the block, stacks them on the device,
 * writes the window's planes to x, y, z (k_count * ni * nj doubles each).  The cuts must agree in block count and in (ni, nj) of `block`:
 * otherwise TM_E_SIZE.  A window that is empty or reaches past nlayers, a block index past the mesh, a NULL pointer: TM_E_ARG. */
int tm_stack_block(const tm_mesh_desc* const* cuts, const tm_stack_opt* opt, uint64_t block, uint64_t k_begin, uint64_t k_count,
                   double* x, double* y, double* z);
/* the same definition evaluated on the host: no GPU touched, works in a process without a device (as tm_mesh_quality_host).  Planar
 * results equal the device's bit for bit; cylindrical y, z differ by what the two sine / cosine implementations differ */
int tm_stack_block_host(const tm_mesh_desc* const* cuts, const tm_stack_opt* opt, uint64_t block, uint64_t k_begin, uint64_t k_count,
                        double* x, double* y, double* z);
/* The same kernel on the coordinates RESIDENT in K handles, one handle per cut (a combined K*B-block handle would run White on cut 0
 * only).  Ordered behind the pending work of every handle; nothing moves to the host but the result; no handle is modified.  `block` must
 * be owned by every handle, every entry must be a live handle: otherwise TM_E_ARG.  Handles that disagree in block count or in (ni, nj) of
 * `block`: TM_E_SIZE.  Cuts spread over ranks are not served.  Bit-identical to tm_stack_block on the downloaded coordinates. */
int tm_stack_smoothers(tm_smoother* const* cuts, const tm_stack_opt* opt, uint64_t block, uint64_t k_begin, uint64_t k_count,
                       double* x, double* y, double* z);

/* ------------------------------------------------------------------ cuts on stream surfaces of revolution
 * No real machine has cylindrical end walls: hub and shroud of an axial turbine are contoured, a mixed-flow or radial stage turns from
 * axial to radial.  The 2-D cut of such a machine is meshed in the unrolled plane (m', theta) of a stream surface of revolution, which is
 * described by a meridional curve x(m), r(m).  The reference's roadmap lists this as open ("possible extension to radial
 * configurations", beside "rotational configurations").  TM_STACK_REVOLUTION = 2 generalises the cylinder to an arbitrary surface of
 * revolution per cut.  It needs per-cut meridional tables, which tm_stack_opt has no room for: they travel in a second record,
 * tm_stack_surfaces.
 *   - Any violation of what the record's comments say answers TM_E_ARG.
 *   - The entry points above answer TM_E_ARG for mapping 2, because they have no tables.  The ones below answer TM_E_ARG for any other
 *     mapping.
 * Cuts.  The 2-D coordinates of cut c are (u, v).
 *   - u is the parameter of the cut's meridional curve.  For an angle-preserving cut u = rref_c * integral dm / r.
 *   - v = rref_c * theta.
 *   - The library does not enforce conformality.  It maps what it is given.
 *   - A cylinder of radius R is x = u, r = R, rref = R.  That is the cylindrical mapping above.
 * Tables.  On interval n of cut c, with h = u[n+1] - u[n], both x and r are the cubic a + t(b + t(c + t d)) in t = u - u[n]:
 *   - a = v[n] exactly, the knot value itself;
 *   - b = (v[n+1] - v[n])/h - h(2M[n] + M[n+1])/6;
 *   - c = M[n]/2;
 *   - d = (M[n+1] - M[n])/(6h).
 *   M is the vector of second derivatives of the natural cubic spline through the knots, with M[0] = M[N-1] = 0.  For TM_SURF_LINEAR, or
 *   for N = 2, M is 0, so c and d are exact zeros.  Everything is formed on the host in long double and rounded once to fp64.
 *   tm_stack_surface_tables is host only, touches no GPU, and returns the coefficients: sum_c (N_c - 1) * 8 doubles, cut after cut,
 *   interval after interval, within an interval in the order ax bx cx dx ar br cr dr.
 * Evaluation per node and cut.  All arithmetic is IEEE fp64.  Nothing is fused.  The device and the host compute the same way.
 *   - n is the largest index <= N-2 with u[n] <= u_node, and n = 0 when u_node < u[0].  Outside the table the end interval's polynomial
 *     is continued.  This is extrapolation, and it is counted (see below).
 *   - t = u_node - u[n], with one rounding.
 *   - x_c = a + t*(b + t*(c + t*d)), innermost first, every operation rounded.  r_c is formed the same way.
 *   - theta_c = v_node / rref[c], with one rounding.
 *   - A node on a knot u[n], n <= N-2, gives t = 0 and returns the knot value bit for bit.
 * Layer k.
 *   - X = sum_c A[k][c] x_c,  R = sum_c A[k][c] r_c,  Theta = sum_c A[k][c] theta_c.
 *   - The sums run over c = 0 .. K-1 in that order, products and sums rounded separately, as above.
 *   - The output is (X, R sin Theta, R cos Theta).
 *   - A is the weight matrix of span, layers and interpolation (tm_stack_weights).  s[k] itself is not used by this mapping.
 *   - r_c(u) <= 0 is not checked per node.
 * Extrapolated nodes.  The three stacking calls take uint64_t* outside, which may be NULL.  They write outside[c], the number of nodes of
 * the block whose u lies outside [u[0], u[N_c-1]] of table c.  The count is independent of the layer window.  On the device it is formed
 * with integer atomics only, so it is deterministic.
 * Error codes, the ordering behind the handles' pending work, the "no handle is modified" rule and the window rules are exactly those of
 * the calls they extend.  The 3-D quality counterparts see bit for bit what the stacking kernel writes, as for the other two mappings. */
#define TM_STACK_MAX_KNOTS 256
enum { TM_SURF_LINEAR = 0, TM_SURF_CUBIC = 1 };
typedef struct tm_stack_surfaces {
    uint64_t ncuts;              /* == opt->ncuts, else TM_E_ARG */
    const uint64_t* nknots;      /* [ncuts], 2 .. TM_STACK_MAX_KNOTS each; may differ between cuts */
    const double* const* u;      /* [ncuts][nknots[c]]  finite, strictly increasing */
    const double* const* x;      /* [ncuts][nknots[c]]  finite */
    const double* const* r;      /* [ncuts][nknots[c]]  finite, > 0 */
    const double* rref;          /* [ncuts] finite, > 0; NULL: rref[c] = span[c] (then every span[c] must be > 0) */
    int32_t interpolation, _pad; /* TM_SURF_LINEAR / TM_SURF_CUBIC: of x(u) and r(u) along the curve */
} tm_stack_surfaces;
int tm_stack_surface_tables(const tm_stack_opt* opt, const tm_stack_surfaces* surfaces, double* coeff);
/* tm_stack_block, tm_stack_block_host and tm_stack_smoothers with the tables (kernel K11 with the surface stage K15) */
int tm_stack_block_surf(const tm_mesh_desc* const* cuts, const tm_stack_opt* opt, const tm_stack_surfaces* surfaces, uint64_t block,
                        uint64_t k_begin, uint64_t k_count, double* x, double* y, double* z, uint64_t* outside /* [ncuts] or NULL */);
int tm_stack_block_surf_host(const tm_mesh_desc* const* cuts, const tm_stack_opt* opt, const tm_stack_surfaces* surfaces, uint64_t block,
                             uint64_t k_begin, uint64_t k_count, double* x, double* y, double* z, uint64_t* outside);
int tm_stack_smoothers_surf(tm_smoother* const* cuts, const tm_stack_opt* opt, const tm_stack_surfaces* surfaces, uint64_t block,
                            uint64_t k_begin, uint64_t k_count, double* x, double* y, double* z, uint64_t* outside);

/* ------------------------------------------------------------------ 3-D quality of stacked blocks
 * Is the stacked mesh usable?  The 2-D report above sees each cut alone; cuts that are clean in 2-D can still enclose negative hexahedra
 * between layers (twist, lean, a spline overshooting between unevenly spaced cuts, a cylindrical wrap of cuts of different pitch, layers
 * given out of order).  A stacked block with nk layers, in the order the caller gave them, has cells (i, j, k), 0 <= i < ni-1,
 * 0 <= j < nj-1, 0 <= k < nk-1.  Corner (a, b, c), each in {0, 1}, is node (i+a, j+b, k+c); x0 .. x7 below number the corners a + 2b + 4c.
 * All arithmetic IEEE fp64, nothing fused, divisions and square roots correctly rounded, sums in the order written.
 *   nodes        exactly what tm_stack_block returns for the layer: the same weight table, the same sum over the cuts c = 0 .. K-1, the
 *                same theta_c = y_c / z[c] and sincos of the cylindrical mapping.  The device report sees bit for bit what K11 writes.
 *   edge         d = upper node - lower node; l2 = d.x*d.x + d.y*d.y + d.z*d.z (left to right), l = sqrt(l2).  One value per edge,
 *                whichever cell asks ((q-p)^2 == (p-q)^2 bit for bit).
 *   corner       u, v, w: the edges leaving the corner along i, j, k, multiplied by (1-2a), (1-2b), (1-2c), so that all eight corners
 *                measure the same handedness (that product IS the edge's d: subtraction is antisymmetric, negation exact).
 *                J = u.x*(v.y*w.z - v.z*w.y) + u.y*(v.z*w.x - v.x*w.z) + u.z*(v.x*w.y - v.y*w.x);  s = J / ((lu*lv)*lw)
 *   cell volume  the exact volume of the trilinear hexahedron, det[p,q,r] = p.(q x r) expanded as J:
 *                12 V = (det[(x7-x1)+(x6-x0), x7-x2, x3-x0] + det[x6-x0, (x7-x2)+(x5-x0), x7-x4]) + det[x7-x1, x5-x0, (x7-x4)+(x3-x0)]
 *                and V = that sum / 12.  (The "long diagonal" 1/6 formula is not exact for warped faces and is not used.)
 *   orientation  o = sign(sum V) over the block's cells; 0 when |sum V| <= cells * 2^-53 * sum |V|, and then everything is reported as
 *                for +1 (the 2-D rule)
 *   classes      degenerate: a corner with (lu*lv)*lw == 0 or non-finite, or a non-finite J;  else inverted: min over corners of
 *                o*J <= 0;  else valid
 *   min_scaled_jacobian   min of o*s over the corners of non-degenerate cells, (worst_block, worst_i, worst_j, worst_k) its cell, ties
 *                to the lowest (block, k, j, i); NaN and 0, 0, 0, 0 when every cell is degenerate
 *   hist[k]      valid cells by their min o*s, the bins of the 2-D report; sum hist == cells - inverted - degenerate
 *   max_aspect   max over non-degenerate cells of max(Li, Lj, Lk) / min(Li, Lj, Lk), L* the sum of the cell's four edges of that
 *                direction added in corner order: Li = ((|x0x1| + |x2x3|) + |x4x5|) + |x6x7|, Lj = ((|x0x2| + |x1x3|) + |x4x6|) + |x5x7|,
 *                Lk = ((|x0x4| + |x1x5|) + |x2x6|) + |x3x7|
 *   max_growth_k max of max(l0, l1) / min(l0, l1) over pairs of consecutive k-edges along every spanwise grid line, pairs with a
 *                zero-length edge skipped; 1.0 when nk < 3.  Growth along i and j inside a layer stays the 2-D report's subject
 *                (tm_smoother_quality on the cuts); growth across block connections is not reported
 *   volumes      min_volume / max_volume: o*V over non-degenerate cells; total_volume = o * sum V
 * tm_quality3d_total: counts and hist summed, extremes combined, total_volume summed, the worst cell the one with the smallest value,
 * orientation the blocks' common one or 0; records with cells == 0 are left out.  Host only. */
typedef struct tm_quality3d {            /* 192 bytes */
    uint64_t cells, inverted, degenerate;
    int32_t  orientation, _pad;
    double   min_scaled_jacobian;
    uint64_t worst_block, worst_i, worst_j, worst_k;
    double   max_aspect, max_growth_k;
    double   min_volume, max_volume, total_volume;
    uint64_t hist[10];
} tm_quality3d;

/* Any 3-D block in PLOT3D order (planes x, y, z of nk*nj*ni doubles, i fastest: what tm_stack_block returned, or a file read back).
 * No GPU touched.  `block` only labels the record.  field, when given, receives the per-cell min of o*s (NaN for degenerate cells),
 * element (k*(nj-1) + j)*(ni-1) + i.  ni, nj or nk < 2: TM_E_SIZE.  NULL x, y, z or out: TM_E_ARG. */
int tm_quality3d_planes_host(const double* x, const double* y, const double* z, uint64_t ni, uint64_t nj, uint64_t nk,
                             uint64_t block, tm_quality3d* out, double* field /* may be NULL: (nk-1)*(nj-1)*(ni-1), i fastest */);
/* Block `block` of the stack of K meshes given on the host, all layers of `opt`, evaluated on the device (kernel K12) straight from
 * the K cuts: the 3-D block is never stored.  Every field equals tm_quality3d_planes_host of the planes tm_stack_block returns, bit
 * for bit, but total_volume (a sum: equal within cells * 2^-53 * sum |V|).  Errors as tm_stack_block; in addition nlayers < 2 or a
 * block with ni < 2 or nj < 2 (no cells): TM_E_SIZE. */
int tm_stack_quality(const tm_mesh_desc* const* cuts, const tm_stack_opt* opt, uint64_t block, tm_quality3d* out);
/* tm_stack_block_host followed by tm_quality3d_planes_host, two layers held at a time; no GPU touched */
int tm_stack_quality_host(const tm_mesh_desc* const* cuts, const tm_stack_opt* opt, uint64_t block, tm_quality3d* out);
/* The same kernel on the coordinates RESIDENT in K handles.  Ordered behind the pending work of every handle exactly as
 * tm_stack_smoothers is; modifies no handle; nothing but the record crosses to the host.  Errors as tm_stack_smoothers, plus the
 * TM_E_SIZE cases above.  Bit-identical to tm_stack_quality on the downloaded coordinates. */
int tm_stack_smoothers_quality(tm_smoother* const* cuts, const tm_stack_opt* opt, uint64_t block, tm_quality3d* out);
/* per-cell min of o*s (NaN for degenerate cells) of the cell layers [k_begin, k_begin + k_count), element
 * ((k-k_begin)*(nj-1) + j)*(ni-1) + i; runs the report first to learn o.  A window that is empty or reaches past nlayers-1: TM_E_ARG. */
int tm_stack_smoothers_quality_field(tm_smoother* const* cuts, const tm_stack_opt* opt, uint64_t block,
                                     uint64_t k_begin, uint64_t k_count /* cell layers */, double* min_scaled_jacobian);
/* The four calls above for TM_STACK_REVOLUTION ("cuts on stream surfaces of revolution"): the nodes are exactly what
 * tm_stack_block_surf returns, evaluated once per node and cut before the march (K12 with the surface stage K15). */
int tm_stack_quality_surf(const tm_mesh_desc* const* cuts, const tm_stack_opt* opt, const tm_stack_surfaces* surfaces, uint64_t block,
                          tm_quality3d* out);
int tm_stack_quality_surf_host(const tm_mesh_desc* const* cuts, const tm_stack_opt* opt, const tm_stack_surfaces* surfaces, uint64_t block,
                               tm_quality3d* out);
int tm_stack_smoothers_quality_surf(tm_smoother* const* cuts, const tm_stack_opt* opt, const tm_stack_surfaces* surfaces, uint64_t block,
                                    tm_quality3d* out);
int tm_stack_smoothers_quality_field_surf(tm_smoother* const* cuts, const tm_stack_opt* opt, const tm_stack_surfaces* surfaces,
                                          uint64_t block, uint64_t k_begin, uint64_t k_count /* cell layers */, double* min_scaled_jacobian);
int tm_quality3d_total(const tm_quality3d* per_block, uint64_t n, tm_quality3d* total);

/* ------------------------------------------------------------------ high-order elements
 * The reference's roadmap lists "high order meshes -- equidistant / other distributions".  Curved elements of order p come from a smoothed
 * block by agglomeration: every p x p group of cells is one element with (p+1)^2 nodes, equidistant in index space because they are the
 * fine mesh itself; any other node distribution is the element's degree-p tensor-product interpolant evaluated at the wanted parametric
 * points, and the elements are judged by the Jacobian of that same polynomial.
 * Order and elements:
 *   - 1 <= p <= TM_HO_MAX_ORDER = 8.  A block of ni x nj nodes qualifies iff (ni-1) % p == 0 and (nj-1) % p == 0 (and ni, nj >= 2); it
 *     then has Ei = (ni-1)/p by Ej = (nj-1)/p elements.  Anything else: TM_E_SIZE.
 *   - Element (e, f) owns the source nodes X[e*p + m][f*p + n], m, n = 0 .. p, which sit at the parametric positions u = m, v = n on [0, p].
 * Target nodes t_0 = 0 < t_1 < ... < t_p = 1 by `distribution`:
 *   - TM_HO_EQUIDISTANT: u_a = a exactly; T is the identity by definition (it is not derived from a/p).
 *   - TM_HO_GAUSS_LOBATTO: t_a = (1 + x_a)/2, x_a the ascending roots of (1 - x^2) P'_p(x), found on the host in long double by Newton
 *     iteration, rounded once to fp64, the end nodes exactly 0 and 1.
 *   - TM_HO_PRESCRIBED: the caller's nodes[0..p]: finite, strictly increasing, nodes[0] == 0, nodes[p] == 1; anything else TM_E_ARG.
 * Tables, formed on the host in long double from u_a = p * t_a (t_a the fp64 node), every entry rounded once to fp64:
 *   T[a][m] = prod_{n != m} (u_a - n)/(m - n);   D[a][m] = sum_{k != m} 1/(m-k) * prod_{n != m,k} (u_a - n)/(m - n)   (d/du of the former at u_a)
 *   Rows 0 and p of T are exact unit vectors, and so is any row whose u_a is an exact integer.
 * Elevated nodes and derivatives.  All arithmetic IEEE fp64, nothing fused, both components alike.  For (A, B) in {(T,T), (D,T), (T,D)}:
 *   W[m][b] = B[b][0]*X[m][0], then + B[b][n]*X[m][n] for n = 1 .. p in that order;
 *   R[a][b] = A[a][0]*W[0][b], then + A[a][m]*W[m][b] for m = 1 .. p.
 *   (T,T): the elevated node Y[e*p+a][f*p+b];  (D,T): its derivative d/du;  (T,D): its derivative d/dv.
 *   A node on an element edge depends only on the source nodes of that grid line, and both neighbouring elements compute it by the same
 *   expression, so the result is again an ni x nj structured array.  A node shared between elements is written by the element above it
 *   (local index 0), the last node of a grid line by the last element.  Corner nodes are the source nodes, except that -0 may become +0.
 *   With TM_HO_EQUIDISTANT, or p = 1, the (T,T) contraction is skipped and the nodes are copied: the planes equal tm_export_soa's bit for
 *   bit.  Across block connections nothing is reconciled HERE: the two sides sum in their own index order and agree to rounding; "welded
 *   unstructured mesh" below merges them and reports by how much they differ.
 * Element record:
 *   J[a][b] = x_u*y_v - x_v*y_u at the element's own (p+1)^2 nodes (one-sided on element edges)
 *   orientation  o: the rule of tm_quality applied to the mesh of element corners -- sign of the sum of a = 0.5*((C.x-A.x)*(D.y-B.y) -
 *                (D.x-B.x)*(C.y-A.y)) over the elements, 0 (reported as +1) when |sum a| <= elements * 2^-53 * sum |a|
 *   per element  Jmin, Jmax of o*J over its nodes; invalid if Jmin <= 0 or any J is non-finite; otherwise its scaled Jacobian
 *                sj = Jmin/Jmax, the usual curved-element measure.  It is SAMPLED AT THE NODES: a positive sj is necessary for a valid
 *                (injective) element, not sufficient -- the Jacobian of a degree-p map is a polynomial of degree 2p-1 per direction and
 *                can dip below zero between the nodes.  The sufficient test is tm_ho_certify (next section).
 *   min_scaled_jacobian  min of sj over valid elements, (worst_block, worst_e, worst_f) its element, ties to the lowest (block, e, f);
 *                NaN and 0, 0, 0 when no element is valid
 *   min_jacobian / max_jacobian   the extremes of o*J over valid elements (NaN when there is none)
 *   hist[k]      valid elements by sj, the bins of tm_quality; sum hist == elements - invalid
 * The record has no summed field: every field is equal between device and host bit for bit (the orientation is decided from a sum and is
 * the same unless that sum lies within rounding of the zero tolerance).
 * tm_ho_quality_total: counts and hist summed, extremes combined, the worst element the one with the smallest value, orientation and
 * order the blocks' common one or 0; records with elements == 0 are left out.  Host only.
 * Order elevation in span for stacked blocks: "high-order hexahedra of stacked blocks" below.
 * Not served: re-projection of wall nodes onto the blade spline (the interpolant of the
 * on-spline nodes is used as it is); Gmsh and HOPR output; repairing invalid elements.  Interface nodes: "welded unstructured mesh". */
#define TM_HO_MAX_ORDER 8
enum { TM_HO_EQUIDISTANT = 0, TM_HO_GAUSS_LOBATTO = 1, TM_HO_PRESCRIBED = 2 };
typedef struct tm_ho_opt {               /* 16 bytes */
    int32_t order, distribution;
    const double* nodes;                 /* TM_HO_PRESCRIBED: [order + 1]; ignored otherwise */
} tm_ho_opt;
typedef struct tm_ho_quality {           /* 152 bytes */
    uint64_t elements, invalid;
    int32_t  orientation, order;
    double   min_scaled_jacobian;
    uint64_t worst_block, worst_e, worst_f;
    double   min_jacobian, max_jacobian;
    uint64_t hist[10];
} tm_ho_quality;

/* nodes [p+1], T and D [(p+1)*(p+1)], row = target node a; any output may be NULL.  Host only: no GPU touched */
int tm_ho_tables(const tm_ho_opt* opt, double* nodes, double* T, double* D);
/* TM_OK, or TM_E_SIZE with tm_last_error naming the first offender: a block whose ni-1 or nj-1 is not a multiple of p, then a
 * connection range whose start or end is not a multiple of p (element edges would not meet across the interface).  Host only */
int tm_ho_check(const tm_mesh_desc* mesh, const tm_ho_opt* opt);
/* Block `block` of a mesh given on the host, elevated on the device (kernel K13).  x, y: planes of ni*nj doubles with i fastest,
 * x[j*ni + i], the layout of tm_export_soa; both may be NULL for a report alone.  q may be NULL.  sj, when given, receives Ei*Ej values
 * as sj[f*Ei + e], NaN for invalid elements.  A block index past the mesh, a block without coordinates, x without y: TM_E_ARG. */
int tm_ho_elevate(const tm_mesh_desc* mesh, const tm_ho_opt* opt, uint64_t block, double* x, double* y, tm_ho_quality* q, double* sj);
/* the same definition evaluated on the host: no GPU touched, works in a process without a device.  Planes, sj and every field of the
 * record equal the device's bit for bit */
int tm_ho_elevate_host(const tm_mesh_desc* mesh, const tm_ho_opt* opt, uint64_t block, double* x, double* y, tm_ho_quality* q, double* sj);
/* The same kernel on the coordinates resident in the handle, behind its pending work on its stream; modifies neither the coordinates
 * nor any solver state.  The buffers (two planes, one pair per element, a few KB of partial records) are allocated on first use with the
 * HIP allocator, outside a caller-provided workspace, and freed by tm_smoother_destroy.  A block the handle does not own, a dead or
 * NULL handle: TM_E_ARG.  A block that fails the size rule: TM_E_SIZE.  Bit-identical to tm_ho_elevate on the downloaded coordinates. */
int tm_smoother_elevate(tm_smoother* s, const tm_ho_opt* opt, uint64_t block, double* x, double* y, tm_ho_quality* q, double* sj);
int tm_ho_quality_total(const tm_ho_quality* per_block, uint64_t n, tm_ho_quality* total);

/* ------------------------------------------------------------------ high-order elements: certificate (Bezier bounds of the Jacobian)
 * The record above samples J at the nodes.  The certificate bounds J on the WHOLE element: J of the degree-p interpolant of the source
 * nodes X[e*p+m][f*p+n] (u, v = 0 .. p) is a polynomial of degree 2p-1 per direction, and its Bernstein coefficients enclose it.  That
 * polynomial is the same for every node distribution, so the certificate depends on the order alone: `distribution` and `nodes` are
 * validated as in tm_ho_elevate and otherwise ignored.  All arithmetic IEEE fp64, nothing fused.
 * Tables, on the host in long double (from exact integers), every entry rounded once:
 *   M[i][m]  the Bernstein coefficient i of the Lagrange polynomial of node m/p, (p+1) x (p+1); rows 0 and p are exact unit vectors
 *   wu[k][i] = C(p-1,i) C(p,k-i) / C(2p-1,k)  (0 <= k-i <= p, else 0),  wv[l][j] = C(p,j) C(p-1,l-j) / C(2p-1,l)  (0 <= l-j <= p-1, else 0)
 * Control points: d[m][n] = X[e*p+m][f*p+n] - X[e*p][f*p] (the element's first corner: J does not see a translation, and the rounding
 *   of everything after is then relative to the element's extent, not to its distance from the origin), then per component
 *   W[m][j] = M[j][0]*d[m][0], then + M[j][n]*d[m][n] for n = 1 .. p;   C[i][j] = M[i][0]*W[0][j], then + M[i][m]*W[m][j] for m = 1 .. p.
 * Derivative coefficients on u, v in [0, p] (K13's units, no factor):
 *   xu[i][j] = C[i+1][j] - C[i][j] (i < p),  xv[i][j] = C[i][j+1] - C[i][j] (j < p), likewise yu, yv.
 * Coefficients of J, k, l = 0 .. 2p-1:
 *   B[k][l] = sum_i wu[k][i] * ( sum_j wv[l][j] * (xu[i][j]*yv[k-i][l-j] - yu[i][j]*xv[k-i][l-j]) ),
 *   i ascending over max(0,k-p) .. min(p-1,k), j ascending over max(0,l-p+1) .. min(p,l), both sums started from 0.
 *   The four corner coefficients are J at the element's corners; min B <= J <= max B on the patch.
 * Subdivision: a patch is split at its midpoint in u (along k), then each half in v (along l), by de Casteljau with 0.5*(a + b); the
 *   corners of the patches of level L are values of J at multiples of p/2^L.
 * Orientation o: K13's (0 counts as +1); the call runs K13's report on the block first to learn it and the nodal verdicts.
 * Guard: g = (G(p) * 2^-53) * R, R = (max|xu| + max|xv|) * (max|yu| + max|yv|) over the element's derivative coefficients -- that is
 *   S = max|xu|*max|yv| + max|xv|*max|yu| PLUS the cross products max|xu|*max|yu| + max|xv|*max|yv|.  The conversion rounds relative to the
 *   element's extent in both directions, so the error of a coefficient scales with R; on a thin cell at an angle to the axes (a boundary
 *   layer) R exceeds S by the aspect ratio, and S alone does not bound the error there.
 *   G(p) = 2 p (4p+14) L^2 + 18p + 4 with L = ||M||_inf the largest absolute row sum (fp64, rounded once): g bounds the rounding error of
 *   a coefficient at any level up to TM_HO_CERT_MAX_DEPTH, with no condition on the element's shape (DESIGN.md, section 4, K14 derives it).
 * Status of an element, breadth first for L = 0 .. max_depth (0 <= max_depth <= TM_HO_CERT_MAX_DEPTH = 4):
 *   a patch is INVALID if a corner has o*B <= 0 or any coefficient is non-finite (at level 0 also if K13's nodal record calls the
 *   element invalid), else PROVEN if min(o*B) > g, else undecided.  The first level with an invalid patch makes the element
 *   TM_HO_INVALID; otherwise the first level without an undecided patch makes it TM_HO_PROVEN; otherwise the undecided patches are split
 *   and the next level is judged; TM_HO_UNDECIDED if level max_depth still has one.  depth: that level.
 *   lo = min over the leaf patches (the proven patches of the levels above `depth`, every patch of level `depth`) of min(o*B), minus g;
 *   hi = the max likewise, plus g:  lo <= o*J <= hi on the whole element.  For a proven element lo/hi is a certified lower bound of
 *   the scaled Jacobian min J / max J that K13 samples.
 * Record: counts; hidden_invalid = invalid here but valid in K13's nodal record; decided_at[L] = proven and invalid elements decided
 *   at level L; min_scaled_bound = min of lo/hi over proven elements with its element (ties to the lowest (block, e, f); NaN, 0, 0, 0
 *   when none is proven); the lowest (e, f) that is not proven, has_unproven = 0 and zeros when all are.  No summed floating-point
 *   field: device and host agree bit for bit in every field, in status and in bounds.
 * tm_ho_certificate_total: counts summed, min_scaled_bound and the first unproven element from the lowest block, orientation, order
 *   and max_depth the blocks' common one or 0 (-1 for max_depth); records with elements == 0 are left out.  Host only.
 * Not served: repairing the elements the certificate rejects; adaptive (non-uniform) subdivision. */
#define TM_HO_CERT_MAX_DEPTH 4
enum { TM_HO_PROVEN = 0, TM_HO_INVALID = 1, TM_HO_UNDECIDED = 2 };
typedef struct tm_ho_certificate {      /* 152 bytes */
    uint64_t elements, proven, invalid, undecided, hidden_invalid;
    int32_t  orientation, order, max_depth, has_unproven;
    uint64_t decided_at[5];
    double   min_scaled_bound;
    uint64_t worst_block, worst_e, worst_f;
    uint64_t first_unproven_block, first_unproven_e, first_unproven_f;
} tm_ho_certificate;
/* M [(p+1)*(p+1)], wu [2p*p], wv [2p*(p+1)], G(p) and ||M||_inf; any output may be NULL.  Host only */
int tm_ho_certify_tables(const tm_ho_opt* opt, double* M, double* wu, double* wv, double* G, double* norm);
/* Block `block` of a mesh given on the host, certified on the device (K13's report, then kernel K14).  status, when given, receives
 * Ei*Ej bytes as status[f*Ei + e]; bounds 2*Ei*Ej doubles, bounds[2*(f*Ei + e)] = (lo, hi); cert may be NULL.  Errors as tm_ho_elevate;
 * a max_depth outside 0 .. TM_HO_CERT_MAX_DEPTH: TM_E_ARG. */
int tm_ho_certify(const tm_mesh_desc* mesh, const tm_ho_opt* opt, int32_t max_depth, uint64_t block, tm_ho_certificate* cert, uint8_t* status, double* bounds);
/* the same definition on the host: no GPU touched; every output equals the device's bit for bit */
int tm_ho_certify_host(const tm_mesh_desc* mesh, const tm_ho_opt* opt, int32_t max_depth, uint64_t block, tm_ho_certificate* cert, uint8_t* status, double* bounds);
/* The same kernels on the coordinates resident in the handle, behind its pending work on its stream; modifies neither the coordinates
 * nor any solver state; buffers as tm_smoother_elevate.  Errors as tm_smoother_elevate.  Bit-identical to tm_ho_certify on the download. */
int tm_smoother_certify(tm_smoother* s, const tm_ho_opt* opt, int32_t max_depth, uint64_t block, tm_ho_certificate* cert, uint8_t* status, double* bounds);
/* The (2p)^2 coefficients of element (e, f) as B[k*2p + l], NOT multiplied by o.  An element past the block: TM_E_ARG.  Host only */
int tm_ho_jacobian_bezier_host(const tm_mesh_desc* mesh, const tm_ho_opt* opt, uint64_t block, uint64_t e, uint64_t f, double* B);
int tm_ho_certificate_total(const tm_ho_certificate* per_block, uint64_t n, tm_ho_certificate* total);

/* ------------------------------------------------------------------ high-order hexahedra of stacked blocks
 * The reference's roadmap asks for "high order meshes" and "3D based on meshed 2d cuts"; this section serves the two together: the
 * layers of a stacked block are agglomerated into curved hexahedra of order p, in span exactly as in i and j.
 * Elements.
 *   - The order p is the same in i, j and span, 1 <= p <= TM_HO3_MAX_ORDER = 4.  Orders 5 .. 8 answer TM_E_ARG: the (p+1)^3 working set
 *     of an element -- fine nodes and the intermediate results of three contraction stages, three components each -- is held on chip
 *     by the kernel, and above p = 4 it no longer fits beside the K cut values of the nodes.
 *   - A stacked block of ni x nj nodes and nk layers qualifies iff (ni-1), (nj-1) and (nk-1) are multiples of p, ni, nj >= 2 and
 *     nk >= p+1.  Anything else: TM_E_SIZE.  It has Ei x Ej x Eg elements, Ei = (ni-1)/p, Ej = (nj-1)/p, Eg = (nk-1)/p.
 *   - Element (e, f, g) owns the fine nodes F[e*p+m][f*p+n][g*p+l], m, n, l = 0 .. p, at the parametric positions (u, v, w) = (m, n, l).
 *   - Span is parametrised by the layer INDEX, as i and j are by the node index.  The layers need not be ordered: a layer out of order
 *     shows up as invalid elements.
 * Fine nodes: exactly what tm_stack_block / tm_stack_block_surf return for the layer -- the same weight table, the same sum over the
 *   cuts c = 0 .. K-1, the same theta_c division and sincos, the same surface stage (K15).  The device path sees bit for bit what K11
 *   writes, which is the contract the 3-D quality report (K12) already has.
 * Tables: tm_ho_tables of the tm_ho_opt (nodes, T, D), unchanged.
 * Contraction.  All arithmetic IEEE fp64, nothing fused, the three components alike, every sum started at index 0 and continued in
 *   ascending order.  For (A, B, C) in {(T,T,T), (D,T,T), (T,D,T), (T,T,D)}:
 *     V[m][n][c] = sum_l C[c][l]*F[m][n][l];   W[m][b][c] = sum_n B[b][n]*V[m][n][c];   R[a][b][c] = sum_m A[a][m]*W[m][b][c]
 *   (T,T,T): the elevated node Y[e*p+a][f*p+b][g*p+c];  the other three: its derivatives d/du, d/dv, d/dw.
 *   - With TM_HO_EQUIDISTANT, or p = 1, the (T,T,T) contraction is skipped and the nodes are copied: the planes equal tm_stack_block's
 *     bit for bit.
 *   - Rows 0 and p of T are unit vectors, so a node on an element face, edge or corner depends only on the fine nodes of that face,
 *     edge or corner, and neighbouring elements compute the same value: the result is again an ni x nj x nk structured array.  A node
 *     shared between elements is written by the element above it in each direction, the last node of a grid line by the last element.
 *   - Consequence: layer k = g*p of the output equals tm_ho_elevate_host applied to fine layer k (x and y, or any two components),
 *     numerically equal -- only a -0 may become +0.
 * Element record.
 *   J = x_u*(y_v*z_w - y_w*z_v) - x_v*(y_u*z_w - y_w*z_u) + x_w*(y_u*z_v - y_v*z_u) at the element's own (p+1)^3 nodes
 *   orientation  o: sign of the sum of V over the hexahedra of element corners, V the exact trilinear volume of "3-D quality of stacked
 *                blocks" with x[a + 2b + 4c] the corner (a*p, b*p, c*p) of the element; 0 (reported as +1) when
 *                |sum V| <= elements * 2^-53 * sum |V|
 *   per element  Jmin, Jmax of o*J over its nodes; invalid if Jmin <= 0 or any J is non-finite; otherwise sj = Jmin/Jmax (for o = -1
 *                formed as Jmax/Jmin of the unoriented values, so that a mirrored block has the same bits)
 *   min_scaled_jacobian  min of sj over valid elements, (worst_block, worst_e, worst_f, worst_g) its element, ties to the lowest
 *                (block, g, f, e); NaN and zeros when no element is valid
 *   min_jacobian / max_jacobian, hist[k]: as in tm_ho_quality
 *   The record is SAMPLED AT THE NODES: a positive sj is necessary for a valid element, not sufficient.  The sufficient test is
 *   tm_stack_certify ("high-order hexahedra: certificate" below).
 *   No summed field: device and host agree bit for bit in every field (the orientation is decided from a sum and is the same unless
 *   that sum lies within rounding of the zero tolerance).
 * tm_ho3_quality_total: the rules of tm_ho_quality_total.  Host only.
 * Not served: orders above 4; different orders in-plane and in span; span nodes evaluated from the
 * spline weights instead of by agglomeration; cuts spread over ranks; re-projection onto the blade; Gmsh, HOPR and CGNS output.
 * Interface nodes: "welded unstructured mesh". */
#define TM_HO3_MAX_ORDER 4
typedef struct tm_ho3_quality {          /* 160 bytes */
    uint64_t elements, invalid;
    int32_t  orientation, order;
    double   min_scaled_jacobian;
    uint64_t worst_block, worst_e, worst_f, worst_g;
    double   min_jacobian, max_jacobian;
    uint64_t hist[10];
} tm_ho3_quality;
/* TM_OK, or TM_E_SIZE with tm_last_error naming the first offender: a block of the cut whose ni-1 or nj-1 is not a multiple of p, then
 * a connection range off the element grid (as tm_ho_check), then the layer count of `stack`.  Only sizes and topology are read from
 * `cut0` and only nlayers from `stack`.  An order above TM_HO3_MAX_ORDER: TM_E_ARG.  Host only */
int tm_ho3_check(const tm_mesh_desc* cut0, const tm_stack_opt* stack, const tm_ho_opt* opt);
/* Any 3-D block in PLOT3D order (planes of nk*nj*ni doubles, i fastest).  No GPU touched.  X, Y, Z: the elevated planes, the same shape;
 * all three NULL for a report alone.  q may be NULL.  sj, when given: Ei*Ej*Eg values as sj[(g*Ej + f)*Ei + e], NaN for invalid
 * elements.  `block` only labels the record. */
int tm_ho3_planes_host(const double* x, const double* y, const double* z, uint64_t ni, uint64_t nj, uint64_t nk, const tm_ho_opt* opt,
                       uint64_t block, double* X, double* Y, double* Z, tm_ho3_quality* q, double* sj);
/* Block `block` of the stack of K meshes given on the host, elevated on the device (kernel K16) straight from the K cuts: the fine 3-D
 * block is never stored.  surfaces: NULL unless stack->mapping is TM_STACK_REVOLUTION, then required (anything else TM_E_ARG).
 * x, y, z: the node layers [g_begin*p, (g_begin + g_count)*p] of the elevated block, g_count*p + 1 planes of ni*nj doubles, i fastest;
 * all three NULL for a report alone (g_count is then ignored and may be 0).  q and sj (either may be NULL) always cover the WHOLE block;
 * with both NULL only the window's elements are evaluated.  outside (may be NULL) is written with TM_STACK_REVOLUTION only, as by
 * tm_stack_block_surf.  Errors: those of tm_stack_block / tm_stack_block_surf, the size rule above (TM_E_SIZE), an order above
 * TM_HO3_MAX_ORDER, planes with an empty window or a window past Eg (TM_E_ARG).  Planes, sj and every field of the record equal
 * tm_ho3_planes_host applied to the planes tm_stack_block[_surf] returns, bit for bit. */
int tm_stack_elevate(const tm_mesh_desc* const* cuts, const tm_stack_opt* stack, const tm_stack_surfaces* surfaces, const tm_ho_opt* opt,
                     uint64_t block, uint64_t g_begin, uint64_t g_count, double* x, double* y, double* z, tm_ho3_quality* q, double* sj,
                     uint64_t* outside);
/* tm_stack_block[_surf]_host followed by the host definition, p+1 fine layers held at a time; no GPU touched */
int tm_stack_elevate_host(const tm_mesh_desc* const* cuts, const tm_stack_opt* stack, const tm_stack_surfaces* surfaces, const tm_ho_opt* opt,
                          uint64_t block, uint64_t g_begin, uint64_t g_count, double* x, double* y, double* z, tm_ho3_quality* q, double* sj,
                          uint64_t* outside);
/* The same kernel on the coordinates RESIDENT in K handles.  Ordered behind the pending work of every handle exactly as
 * tm_stack_smoothers is; modifies no handle.  Errors as tm_stack_smoothers[_surf], plus the cases above.  Bit-identical to
 * tm_stack_elevate on the downloaded coordinates. */
int tm_stack_smoothers_elevate(tm_smoother* const* cuts, const tm_stack_opt* stack, const tm_stack_surfaces* surfaces, const tm_ho_opt* opt,
                               uint64_t block, uint64_t g_begin, uint64_t g_count, double* x, double* y, double* z, tm_ho3_quality* q,
                               double* sj, uint64_t* outside);
int tm_ho3_quality_total(const tm_ho3_quality* per_block, uint64_t n, tm_ho3_quality* total);

/* ------------------------------------------------------------------ high-order hexahedra: certificate (Bezier bounds of the Jacobian)
 * The record above samples J at the (p+1)^3 nodes.  The certificate bounds J on the WHOLE hexahedron: J of the degree-p interpolant of the
 * fine nodes is a polynomial of degree 3p-1 per direction, and its (3p)^3 Bernstein coefficients enclose it.
 * Elements, the order rule (1 <= p <= TM_HO3_MAX_ORDER), the size rule and the fine nodes are those of the section above: the fine nodes are
 *   exactly what tm_stack_block[_surf] returns.  The certificate depends on the order alone: `distribution` and `nodes` are validated and
 *   otherwise ignored.  All arithmetic IEEE fp64, nothing fused.  N1 = p+1, N = 3p.
 * Tables, on the host in long double from exact integers, every entry rounded once:
 *   M[i][m]          tm_ho_certify_tables' M, unchanged
 *   w^{a,b}[k][i]  = C(a,i) C(b,k-i) / C(a+b,k)  (0 <= k-i <= b, else 0), k = 0 .. a+b, i = 0 .. a: the weights of the Bernstein product of a
 *                    degree-a and a degree-b polynomial.  wA packs w^{p,p}, w^{p-1,p}, w^{p,p-1}; wB packs w^{p-1,2p}, w^{p,2p-1} (the latter
 *                    serves v and w alike), each row-major with a+1 entries per row.
 * Control points, per component: d[m][n][l] = F[e*p+m][f*p+n][g*p+l] - F[e*p][f*p][g*p], then three stages, span first:
 *   V[m][n][k] = M[k][0]*d[m][n][0], then + M[k][l]*d[m][n][l] for l = 1 .. p;
 *   W[m][j][k] = M[j][0]*V[m][0][k], then + M[j][n]*V[m][n][k] for n = 1 .. p;
 *   C[i][j][k] = M[i][0]*W[0][j][k], then + M[i][m]*W[m][j][k] for m = 1 .. p.
 * Derivative coefficients on [0, p]^3 (K16's units, no factor):
 *   xu[i][j][k] = C[i+1][j][k] - C[i][j][k]  (p x N1 x N1),  xv[i][j][k] = C[i][j+1][k] - C[i][j][k]  (N1 x p x N1),
 *   xw[i][j][k] = C[i][j][k+1] - C[i][j][k]  (N1 x N1 x p), likewise y and z.
 * Jacobian J = Xu . (Xv x Xw), in two Bernstein products.  Every sum runs over its admissible index range in ascending order and starts
 * from 0 (s = 0, then s = s + weight * value); the sums are nested u outside, then v, then w inside.
 *   1. cofactors, (2p+1) x 2p x 2p coefficients each, for (f, g) = (y, z), (z, x), (x, y) giving cx, cy, cz:
 *        c[a][b][c] = sum_i w^{p,p}[a][i] * ( sum_j w^{p-1,p}[b][j] * ( sum_k w^{p,p-1}[c][k] * t ) ),
 *        t = fv[i][j][k]*gw[a-i][b-j][c-k] - gv[i][j][k]*fw[a-i][b-j][c-k]
 *        (cx = yv zw - zv yw, cy = zv xw - xv zw, cz = xv yw - yv xw);
 *        i over max(0,a-p) .. min(p,a), j over max(0,b-p) .. min(p-1,b), k over max(0,c-p+1) .. min(p,c).
 *   2. B[a][b][c] = sum_i w^{p-1,2p}[a][i] * ( sum_j w^{p,2p-1}[b][j] * ( sum_k w^{p,2p-1}[c][k] * t ) ),
 *        t = xu[i][j][k]*cx[a-i][b-j][c-k] + yu[i][j][k]*cy[a-i][b-j][c-k] + zu[i][j][k]*cz[a-i][b-j][c-k]   (left to right);
 *        i over max(0,a-2p) .. min(p-1,a), j over max(0,b-2p+1) .. min(p,b), k likewise with c.
 *   The eight corner coefficients are J at the element's corners; min B <= J <= max B on the patch.
 * Subdivision: a patch is split at its midpoint in u (index a), then each half in v, then each quarter in w, by de Casteljau with
 *   0.5*(a + b) along every line of the direction: eight children, child q = (u half) + 2 (v half) + 4 (w half).  The corners of the
 *   patches of level L are values of J at multiples of p/2^L.
 * Orientation o and the nodal verdict: K16's (0 counts as +1); the call runs K16's report on the block first.
 * Guard: g = (G3(p) * 2^-53) * R3,  R3 = (sx * sy) * sz,  sx = (max|xu| + max|xv|) + max|xw| over the element's derivative coefficients,
 *   sy and sz likewise.  G3(p) = 9 p (6p+20) L^3 + 99p + 52 with L = ||M||_inf (fp64, rounded once; the expression in long double, rounded
 *   once): g bounds the rounding error of a coefficient at any level up to TM_HO3_CERT_MAX_DEPTH with no condition on the element's shape
 *   (DESIGN.md, section 4, K17 derives it).  It is the only tolerance.
 * Status of an element, levels, lo / hi, hidden_invalid, decided_at, min_scaled_bound, the first unproven element and the tie rules: those of
 *   "high-order elements: certificate" above, with "patch corner" meaning the eight corners, 0 <= max_depth <= TM_HO3_CERT_MAX_DEPTH = 3 (at
 *   depth 3 an element has up to 512 leaf patches of (3p)^3 coefficients: one level less than in 2-D), elements ordered by (block, g, f, e).
 *   No summed floating-point field: device and host agree bit for bit in record, status and bounds.
 * tm_ho3_certificate_total: the rules of tm_ho_certificate_total.  Host only.
 * Not served: repairing the elements the certificate rejects; adaptive subdivision; orders above 4; cuts spread over ranks. */
#define TM_HO3_CERT_MAX_DEPTH 3
typedef struct tm_ho3_certificate {     /* 160 bytes */
    uint64_t elements, proven, invalid, undecided, hidden_invalid;
    int32_t  orientation, order, max_depth, has_unproven;
    uint64_t decided_at[4];
    double   min_scaled_bound;
    uint64_t worst_block, worst_e, worst_f, worst_g;
    uint64_t first_unproven_block, first_unproven_e, first_unproven_f, first_unproven_g;
} tm_ho3_certificate;
/* M [(p+1)^2]; wA [(2p+1)(p+1) + 2p*p + 2p(p+1)]; wB [3p*p + 3p(p+1)]; G3(p) and ||M||_inf; any output may be NULL.  Host only */
int tm_ho3_certify_tables(const tm_ho_opt* opt, double* M, double* wA, double* wB, double* G, double* norm);
/* The (3p)^3 coefficients of element (e, f, g) of any 3-D block in PLOT3D order as B[(a*3p + b)*3p + c], NOT multiplied by o.  An element
 * past the block: TM_E_ARG; the size rule: TM_E_SIZE.  Host only */
int tm_ho3_jacobian_bezier_host(const double* x, const double* y, const double* z, uint64_t ni, uint64_t nj, uint64_t nk, const tm_ho_opt* opt,
                                uint64_t e, uint64_t f, uint64_t g, double* B);
/* Any 3-D block in PLOT3D order (what tm_stack_block returned, or a file read back).  No GPU touched.  status, when given, receives
 * Ei*Ej*Eg bytes as status[(g*Ej + f)*Ei + e]; bounds 2 doubles (lo, hi) per element in the same order; cert may be NULL.  `block` only
 * labels the record.  A max_depth outside 0 .. TM_HO3_CERT_MAX_DEPTH: TM_E_ARG. */
int tm_ho3_certify_planes_host(const double* x, const double* y, const double* z, uint64_t ni, uint64_t nj, uint64_t nk, const tm_ho_opt* opt,
                               int32_t max_depth, uint64_t block, tm_ho3_certificate* cert, uint8_t* status, double* bounds);
/* Block `block` of the stack of K meshes given on the host, certified on the device: K16's report, then per window of span elements K11
 * into device planes and kernel K17 on them.  surfaces, outside and the errors as tm_stack_elevate.  Every output equals
 * tm_ho3_certify_planes_host applied to the planes tm_stack_block[_surf] returns, bit for bit. */
int tm_stack_certify(const tm_mesh_desc* const* cuts, const tm_stack_opt* stack, const tm_stack_surfaces* surfaces, const tm_ho_opt* opt,
                     int32_t max_depth, uint64_t block, tm_ho3_certificate* cert, uint8_t* status, double* bounds, uint64_t* outside);
/* tm_stack_block[_surf]_host followed by tm_ho3_certify_planes_host; no GPU touched */
int tm_stack_certify_host(const tm_mesh_desc* const* cuts, const tm_stack_opt* stack, const tm_stack_surfaces* surfaces, const tm_ho_opt* opt,
                          int32_t max_depth, uint64_t block, tm_ho3_certificate* cert, uint8_t* status, double* bounds, uint64_t* outside);
/* The same kernels on the coordinates RESIDENT in K handles.  Ordered behind the pending work of every handle exactly as
 * tm_stack_smoothers is; modifies no handle.  Errors as tm_stack_smoothers_elevate.  Bit-identical to tm_stack_certify on the download. */
int tm_stack_smoothers_certify(tm_smoother* const* cuts, const tm_stack_opt* stack, const tm_stack_surfaces* surfaces, const tm_ho_opt* opt,
                               int32_t max_depth, uint64_t block, tm_ho3_certificate* cert, uint8_t* status, double* bounds, uint64_t* outside);
int tm_ho3_certificate_total(const tm_ho3_certificate* per_block, uint64_t n, tm_ho3_certificate* total);

/* ------------------------------------------------------------------ welded unstructured mesh (kernel K18)
 * Everything above hands out separate blocks: an interface carries its nodes twice, a junction three or four times.  This section gives
 * the blocks ONE node numbering across their connections, and from it the points and cells of a conforming unstructured mesh -- what the
 * reference's roadmap items "legacy vtk", "modern vtk formats" and "cgns - unstructured" all need first.  The high-order node grid of a
 * block is the block's own ni x nj index space (elements are agglomerated, nodes only relocated), so one numbering serves linear
 * quadrilaterals, Lagrange quadrilaterals of order p, stacked hexahedra and Lagrange hexahedra.  The numbering is a pure function of
 * sizes and connections; points and cells are gathers.
 * Definition.
 *   Flat index   node (i, j) of block b: n = off_b + j*ni_b + i, off_b the sum of ni*nj over the earlier blocks -- the plane order of
 *                tm_export_soa (i fastest).  N = nodes_in is their number.
 *   Links        a connection WITHOUT periodicity links, for t = 0 .. len-1, position start +- t of r[0] with start +- t of r[1] (minus when
 *                start > end).  Side and position give the node as everywhere in this header: TM_SIDE_I_MIN is j = 0 at i = position,
 *                TM_SIDE_I_MAX j = nj-1, TM_SIDE_J_MIN i = 0 at j = position, TM_SIDE_J_MAX i = ni-1.
 *   Classes      the transitive closure of the links.  A junction of four corners is one class although no connection joins all four;
 *                a block may be connected to itself.  An unlinked node is a class of one.
 *   Owner, id    the owner of a class is its smallest flat index; map[n] = the number of owners with a smaller flat index than the
 *                owner of n (first-occurrence order); nodes_out = the number of classes.
 *   Periodic     connections weld nothing.  They yield the pairs (map[a_t], map[b_t]), connection after connection, t ascending
 *                (tm_weld_periodic_pairs), to which the connection's translation belongs.
 *   Points       a welded node has the coordinates of its owner, bit for bit; nothing is averaged.  With nk layers the welded planes are
 *                layer-major: value k*nodes_out + id.  max_gap = max over layers k and nodes n of max_c |coord_c(k, n) - coord_c(k, owner(n))|,
 *                gap_node = the smallest k*N + n at which it occurs (0 when max_gap is 0; NaN differences never count).  A diagnostic: a
 *                wrong connection shows as a gap of the size of the mesh, a good one as the rounding the two sides differ by.
 *                periodic_gap = max over the periodic pairs, every layer and components d = 0, 1 of |P_d[map[a]] + periodicity[d] - P_d[map[b]]|
 *                on the welded planes P (meaningful where components 0, 1 are the plane of the cut; 0 without periodic connections).
 *   Cells        element (e, f) of block b at order p, 1 <= p <= TM_HO_MAX_ORDER, lists map[off_b + (f*p + b')*ni + e*p + a] for its local
 *                nodes (a, b') in the order of VTK's Lagrange quadrilateral: corners (0,0), (p,0), (p,p), (0,p); edges b' = 0, a = p, b' = p,
 *                a = 0, each ascending; the interior with a fastest.  At p = 1 that is VTK_QUAD.  Elements run e fastest, then f, blocks
 *                in order.  With nk >= 2 layers: hexahedra of order p <= TM_HO3_MAX_ORDER, id = (g*p + c)*nodes_out + map[...], local nodes
 *                in the order of VTK 9's Lagrange hexahedron (corners of c = 0, then c = p; edges of c = 0, of c = p, the four vertical
 *                edges; faces a = 0, a = p, b' = 0, b' = p, c = 0, c = p; interior), elements ordered e fastest, then f, then g.
 *   Ids are int32_t: a mesh of more than 2^31 - 1 nodes, or nk * nodes_out > 2^31 - 1, answers TM_E_ARG before anything is read.
 * Errors of every call: a connection whose two ranges differ in length or whose range leaves its side: TM_E_MISMATCH; a block with ni < 2
 *   or nj < 2: TM_E_SIZE; a block index past the mesh, a side that does not exist, more than 65535 blocks or connections: TM_E_ARG.
 *   Cells of order p: tm_ho_check (tm_ho3_check with nk >= 2) is the precondition and its answer is returned.
 * Device and host agree exactly in map, info, planes and cells: integers, copies, |a - b| and max are all that is computed.
 * Not served: .vtu, CGNS, Gmsh and HOPR writers; gluing periodic sides; cuts or blocks spread over ranks (a handle with rank hooks
 *   answers TM_E_UNSUPPORTED); averaging the two sides of an interface.  Boundary patches: "boundary of the welded mesh" below. */
typedef struct tm_weld_info {            /* 88 bytes */
    uint64_t nodes_in, nodes_out;
    uint64_t classes_2, classes_3, classes_4, classes_5_up;   /* classes of that many nodes */
    uint64_t max_class;                                       /* 1 when nothing is welded */
    uint64_t periodic_pairs;
    uint64_t gap_node;
    double   max_gap, periodic_gap;
} tm_weld_info;
/* map: N ids; info may be NULL.  Only sizes and connections are read: blocks[b].xy may be NULL.  max_gap, gap_node and periodic_gap
 * are written as 0 (tm_weld_points fills them).  On the device: a lock-free union-find over the perimeter nodes (the class root is the
 * smallest index, so the result does not depend on execution order), then an exclusive prefix sum of the owner flags over all N nodes
 * as reduce / scan of partials / downsweep in separate launches. */
int tm_weld_map(const tm_mesh_desc* mesh, int32_t* map, tm_weld_info* info);
/* the same definition on the host: no GPU touched */
int tm_weld_map_host(const tm_mesh_desc* mesh, int32_t* map, tm_weld_info* info);
/* Welded planes.  map: what tm_weld_map returned for this mesh.  planes[c*nblocks + b]: component c (ncomp = 1 .. 3) of block b, nk
 * layers (nk <= 1: one) of ni*nj doubles with i fastest -- the planes of tm_export_soa / tm_ho_elevate (nk = 1) or of tm_stack_block /
 * tm_stack_elevate.  out[c]: nk * nodes_out doubles.  info (may be NULL): nodes_in, nodes_out, periodic_pairs, max_gap, gap_node and
 * periodic_gap are written, the class counts are left as they are.  A NULL pointer, ncomp outside 1 .. 3: TM_E_ARG. */
int tm_weld_points(const tm_mesh_desc* mesh, const int32_t* map, int32_t ncomp, uint64_t nk, const double* const* planes, double* const* out,
                   tm_weld_info* info);
int tm_weld_points_host(const tm_mesh_desc* mesh, const int32_t* map, int32_t ncomp, uint64_t nk, const double* const* planes, double* const* out,
                        tm_weld_info* info);
/* Map and welded points of the coordinates RESIDENT in a handle, behind its pending work on its stream like tm_smoother_export_soa: the
 * interleaved coordinates are read in place (no export pass in between); modifies neither the coordinates nor any solver state.
 * map (N ids) may be NULL; X, Y: nodes_out doubles each -- N is always enough.  Every field of info is written.  A dead or NULL handle,
 * NULL X or Y: TM_E_ARG; a handle with rank hooks: TM_E_UNSUPPORTED.  Equal to tm_weld_map + tm_weld_points on the downloaded coordinates. */
int tm_smoother_weld(tm_smoother* s, int32_t* map_or_null, double* X, double* Y, tm_weld_info* info);
/* cells: ids per element as above, (p+1)^2 per quadrilateral (nk <= 1) or (p+1)^3 per hexahedron (nk >= 2 layers).  map and nodes_out:
 * tm_weld_map's.  Sizes are checked before anything is read. */
int tm_weld_cells(const tm_mesh_desc* mesh, const int32_t* map, uint64_t nodes_out, int32_t order, uint64_t nk, int32_t* cells);
int tm_weld_cells_host(const tm_mesh_desc* mesh, const int32_t* map, uint64_t nodes_out, int32_t order, uint64_t nk, int32_t* cells);
/* pairs: 2 * periodic_pairs ids.  Host only: the perimeter is small */
int tm_weld_periodic_pairs(const tm_mesh_desc* mesh, const int32_t* map, int32_t* pairs);

/* ------------------------------------------------------------------ boundary of the welded mesh (kernel K19)
 * The welded mesh above has cells and no boundary.  This section lists its boundary faces -- edges of the plane mesh, quadrilaterals of
 * the stacked one -- over the SAME welded ids, grouped into patches that a flow solver reads: the conditions of the description (inlet,
 * outlet, wall), the two sides of every periodic connection as matched faces, whatever is left (the reference's O4H template leaves the
 * blade there: its "TODO: add wall boundary condition"), and with layers hub and shroud.  Like the numbering, the face lists are a pure
 * function of sizes, connections and conditions; the measures of the patches are sums over the welded points.
 * Definition.
 *   Segments     at order p a side of block b has E = (length - 1) / p segments, segment e covering positions e*p .. (e+1)*p of the side.
 *                tm_ho_check (tm_ho3_check with nk >= 2) is the precondition and its answer is returned.
 *   Coverage     a range (of a connection or a condition) covers a segment when both end positions of the segment lie inside it.  A range
 *                that covers some but not all of the p fine edges of a segment is off the element grid: TM_E_MISMATCH, naming the range
 *                (connections are refused by the precondition already; this is the rule for conditions).
 *   Interior     a segment covered by a connection WITHOUT periodicity is interior.  Every other segment is a boundary face.
 *   Patches      in this order: the nbcs conditions in order (kind = their TM_BC_* value, source = index of the condition, also when no
 *                face falls to them); per periodic connection in order two patches, the side of r[0] then the side of r[1] (kind
 *                TM_PATCH_PERIODIC, source = index of the connection, partner = the other patch, translation = the connection's for the
 *                side of r[0] and its negative for the side of r[1]: own face + translation = partner's face); one patch
 *                TM_PATCH_UNASSIGNED; with nk >= 2 TM_PATCH_HUB (layer 0) and TM_PATCH_SHROUD (layer nk-1).  A boundary segment belongs to
 *                the patch of the first periodic connection range that covers it (connections in order, r[0] before r[1]), otherwise to
 *                the first condition that covers it, otherwise it is unassigned.
 *   Face order   patch-major: patches[q].face_begin and .faces form a CSR over the face list.  Inside a condition patch or the unassigned
 *                patch: block, then side 0 .. 3 (the TM_SIDE_* value), then e ascending.  Inside a periodic patch: the element index t along
 *                the connection's own pair order (pairs t*p .. (t+1)*p), ascending, so that face t of one side is the partner of face t
 *                of the other.  With layers the span element g = 0 .. (nk-1)/p - 1 is slowest inside every lateral patch; the caps list
 *                the plane elements in the order of tm_weld_cells (e fastest, then f, blocks in order).
 *   Local nodes  the block sense of a side is counter-clockwise in index space: TM_SIDE_I_MIN (j = 0) i ascending, TM_SIDE_J_MAX
 *                (i = ni-1) j ascending, TM_SIDE_I_MAX (j = nj-1) i descending, TM_SIDE_J_MIN (i = 0) j descending; a = 0 .. p runs along it.
 *                Plane faces are VTK Lagrange curves: a = 0, then a = p, then a = 1 .. p-1 (VTK_LINE at p = 1).  Lateral faces of a stacked
 *                mesh are VTK Lagrange quadrilaterals over (a, c), c the span, in the order given for cells above; id = (g*p + c)*nodes_out
 *                + map[...].  Cap faces are the same quadrilateral over (a, b'): on the hub a runs along j and b' along i, on the shroud a
 *                along i and b' along j; shroud ids are offset by (nk-1)*nodes_out.
 *   Orientation  block_orientation[b] = +-1 (0 and a NULL array count as +1): tm_mesh_quality's orientation of the block for a plane mesh,
 *                tm_stack_quality's for a stacked one.  A block with -1 lists a -> p - a on its curves and lateral faces, and on its caps the
 *                two directions are exchanged.  With these values every normal points OUT of the mesh: for a curve the tangent turned by
 *                -90 degrees, for a quadrilateral the right-hand rule of its ring.  Node (a, c) of periodic face t is then the image of
 *                node (p - a, c) of its partner.
 *   origin       four values per face: block, side, e, g.  Caps: side 4 (hub) / 5 (shroud), e = f*Ei + e the block's own element index,
 *                g = 0 / (nk-1)/p - 1.  Plane faces: g = 0.
 *   Measures     per patch the sums over the fine sub-faces of its faces (p per curve, p*p per quadrilateral), every term in IEEE fp64,
 *                nothing fused.  Plane, fine edge A -> B: n = (yB - yA, -(xB - xA)), length = sqrt(dx*dx + dy*dy), moment = xA*yB - xB*yA;
 *                sum moment / 2 over a closed boundary is the enclosed area.  Stacked, fine quadrilateral A, B, C, D in ring order:
 *                n = 0.5 * (C - A) x (D - B), measure = |n|, moment = 0.25*(A + B + C + D) . n; sum moment / 3 is the volume when the faces
 *                are planar.  Host and device form identical terms and differ in the order of the sums only: each patch value agrees
 *                within 2 (n-1) 2^-53 sum |t| over its n terms.  The device result is the same from run to run (no floating-point atomics).
 *   Diagnostics  of the plane boundary, from the end nodes of the segments: loops = connected components, irregular_nodes = boundary
 *                nodes whose degree is not 2.
 * Not served: gluing periodic sides; telling wall from hub inside `unassigned`; blocks spread over ranks; .vtu / CGNS writers (they
 *   now need a writer only). */
enum { TM_PATCH_PERIODIC = 16, TM_PATCH_UNASSIGNED = 17, TM_PATCH_HUB = 18, TM_PATCH_SHROUD = 19 };   /* kinds beside TM_BC_* */
typedef struct tm_weld_patch {           /* 88 bytes */
    int32_t  kind;                       /* TM_BC_* or TM_PATCH_* */
    int32_t  source;                     /* index of the condition / the periodic connection; -1 otherwise */
    int32_t  partner;                    /* the other patch of a periodic connection; -1 otherwise */
    int32_t  _pad;
    uint64_t face_begin, faces;
    double   translation[2];             /* periodic patches; 0 otherwise */
    double   measure, normal[3], moment; /* tm_weld_faces_measure */
} tm_weld_patch;
typedef struct tm_weld_boundary_info {   /* 56 bytes */
    uint64_t patches, faces, nodes_per_face;
    uint64_t lateral_faces, cap_faces;   /* cap_faces: hub and shroud together; 0 for a plane mesh */
    uint64_t loops, irregular_nodes;
} tm_weld_boundary_info;
/* Host only; the perimeter is small.  info may be NULL; patches: info->patches records (nbcs + 2 * periodic connections + 1, + 2 with
 * nk >= 2) with kind, source, partner, translation and the CSR, measures zeroed -- NULL only counts. */
int tm_weld_boundary_plan(const tm_mesh_desc* mesh, int32_t order, uint64_t nk, tm_weld_boundary_info* info, tm_weld_patch* patches_or_null);
/* faces: info.faces * info.nodes_per_face ids; face_patch: the patch of every face; origin: 4 values per face.  map and nodes_out:
 * tm_weld_map's.  Sizes are checked before anything is read; errors as tm_weld_cells, and more than 2^31 - 1 faces: TM_E_ARG.  On the
 * device the ids are expanded by the kernels (k_weld_faces_lateral over the host's segment table, k_weld_faces_caps over all plane
 * elements); face_patch and origin are integers of the plan and are written by the host in both. */
int tm_weld_boundary_faces(const tm_mesh_desc* mesh, const int32_t* map, uint64_t nodes_out, int32_t order, uint64_t nk,
                           const int32_t* block_orientation, int32_t* faces, int32_t* face_patch_or_null, int32_t* origin_or_null);
int tm_weld_boundary_faces_host(const tm_mesh_desc* mesh, const int32_t* map, uint64_t nodes_out, int32_t order, uint64_t nk,
                                const int32_t* block_orientation, int32_t* faces, int32_t* face_patch_or_null, int32_t* origin_or_null);
/* Measures of ANY face list over welded planes (points[c]: component c, npoints doubles, as tm_weld_points wrote them): dim = 2 curves of
 * order 1 .. TM_HO_MAX_ORDER over components 0, 1 (ncomp >= 2); dim = 3 quadrilaterals of order 1 .. TM_HO3_MAX_ORDER (ncomp = 3).
 * face_patch must not decrease (patch-major) and stay below npatches; ids lie in 0 .. npoints-1: TM_E_ARG otherwise, checked before
 * anything is launched.  Writes measure, normal and moment of patches[0 .. npatches-1] and nothing else of them.  On the device: a gather
 * through the ids, wave -> workgroup -> one partial per (workgroup, patch), and a finalize launch that sums the partials in fixed order. */
int tm_weld_faces_measure(int32_t dim, int32_t order, uint64_t nfaces, const int32_t* faces, const int32_t* face_patch, uint64_t npatches,
                          uint64_t npoints, int32_t ncomp, const double* const* points, tm_weld_patch* patches);
int tm_weld_faces_measure_host(int32_t dim, int32_t order, uint64_t nfaces, const int32_t* faces, const int32_t* face_patch, uint64_t npatches,
                               uint64_t npoints, int32_t ncomp, const double* const* points, tm_weld_patch* patches);
/* Boundary of the coordinates RESIDENT in a handle, behind its pending work; modifies nothing.  Defined as tm_smoother_weld followed by
 * tm_weld_boundary_faces and tm_weld_faces_measure on its map, X, Y -- the welded points stay on the device.  faces / face_patch (may be
 * NULL) / patches sized by tm_weld_boundary_plan(mesh, order, 0).  A NULL block_orientation is taken by the rule of tm_smoother_quality.
 * A dead handle, NULL patches: TM_E_ARG; rank hooks: TM_E_UNSUPPORTED. */
int tm_smoother_weld_boundary(tm_smoother* s, int32_t order, const int32_t* block_orientation_or_null, int32_t* faces, int32_t* face_patch,
                              tm_weld_patch* patches);

/* ------------------------------------------------------------------ wall distance of the welded mesh (kernel K20)
 * The distance of every welded node to the nearest wall face: the per-node field that Spalart-Allmaras, SST and wall functions read
 * from a mesh.  On a blade passage the nearest wall of a node near a periodic side is the NEIGHBOURING blade -- the same wall shifted by
 * the pitch -- so a query is also made under images: the translations K19 hands out with its periodic patches, or rotations about x.
 * Definition (csrc/tm_wall_distance.hpp holds it as code; every expression order below is fixed, nothing is fused).
 *   Input        dim = 2 or 3; points[c]: component c, npoints doubles, as tm_weld_points wrote them; wall faces of order 1 over the same
 *                ids: 2 ids per face (edge A -> B) for dim = 2, 4 ids in ring order A, B, C, D for dim = 3; 1 .. 16 images.
 *   Images       an image maps the QUERY, not the wall: P' = (x - t0, (c*y + s*z) - t1, (-s*y + c*z) - t2), formed once per point and image;
 *                the distance is defined from this rounded P'.  dim = 2: z, t2 and s are ignored, c must be 1 and P'_y = y - t1.  Image 0
 *                must be the identity {0, 0, 0, 1, 0}.
 *   Primitives   a 2-D face is one segment; a 3-D face is the triangles (A, B, C) and (A, C, D), primitives 2f and 2f + 1.  The distance is
 *                to these LINEAR faces: with curved elements the wall is still the fine mesh the equidistant nodes lie on.
 *   Segment      a = B - A, L = a.a, iL = 1 / L (once per face), p = P' - A, t = p.a; t <= 0: d2 = p.p; t >= L: d2 = |P' - B|^2; otherwise
 *                r = t * iL, q = p - r*a, d2 = q.q.  A = B falls into the first branch.  Sums run left to right over the components.
 *   Triangle     closest point by Voronoi region, tested in this order with ab = B - A, ac = C - A, bc = C - B, ap = P' - A, bp = P' - B,
 *                cp = P' - C, d1 = ab.ap, d2 = ac.ap, d3 = ab.bp, d4 = ac.bp, d5 = ab.cp, d6 = ac.cp, tb = bc.bp:
 *                vertex A (d1 <= 0, d2 <= 0): ap.ap; vertex B (d3 >= 0, d4 <= d3): bp.bp; edge AB (d1*d4 - d3*d2 <= 0, d1 >= 0, d3 <= 0):
 *                q = ap - (d1 * iLab) ab; vertex C (d6 >= 0, d5 <= d6): cp.cp; edge AC (d5*d2 - d1*d6 <= 0, d2 >= 0, d6 <= 0):
 *                q = ap - (d2 * iLac) ac; edge BC (d3*d6 - d5*d4 <= 0, 0 <= tb <= bc.bc): q = bp - (tb * iLbc) bc; otherwise the interior,
 *                d2 = (ap.n)^2 with n the unit normal: ab x ac, each component a difference of two error-free products (two fma), divided by its
 *                length once per triangle.  No division and no square root per pair.  A triangle with ab x ac = 0 (collinear) is replaced by (A', B', B') of its longest edge, which
 *                the vertex and edge regions of A'B' serve for every query: the distance to that edge, never 0/0.
 *   Error        |d2 - exact d2| <= 32 * 2^-53 * rho2, rho2 = the largest squared distance from P' to the nodes of the face + its longest
 *                squared edge, independent of the aspect ratio; derived for triangles whose largest angle sine is at least 2^-20
 *                (DESIGN section 4, K20).
 *   Result       per point the key (d2, face, image) is minimised lexicographically over all faces and images -- the smallest d2, then the
 *                smallest face index, then the smallest image index; a NaN d2 never wins.  distance = sqrt(d2), face = index into the given
 *                face list, image = index of the image.  A point with a NaN coordinate (or that no pair serves): NaN, -1, -1.  The minimum
 *                does not depend on the order of evaluation, so host, device, culled and not culled give the same three outputs bit for bit.
 *   Record       points, faces, primitives, images, groups (runs of 64 consecutive primitives); on_wall: points with distance exactly 0;
 *                nan_points; nearest_via_image: points whose image is not 0; max_distance with max_point, the smallest id at the maximum
 *                (0 and 0 when no point has a distance); pairs_evaluated: point-primitive evaluations made (host: points x primitives x
 *                images).  Host and device agree in every field but pairs_evaluated.
 * Errors: a NULL input or distance, an id outside 0 .. npoints-1, dim other than 2 or 3, nfaces = 0, more than 2^31 - 1 faces or points,
 *   nimages outside 1 .. 16, an image 0 that is not the identity, c != 1 with dim = 2: TM_E_ARG, before anything is launched.
 * Not served: distance to curved high-order faces; cell-centre queries; blocks spread over ranks; telling blade from hub inside
 *   `unassigned`; signed distance; Eikonal or PDE wall distance. */
typedef struct tm_wall_image {           /* 40 bytes */
    double t[3];
    double c, s;
} tm_wall_image;
typedef struct tm_wall_info {            /* 88 bytes */
    uint64_t points, faces, primitives, images, groups;
    uint64_t on_wall, nan_points, nearest_via_image;
    uint64_t max_point;
    uint64_t pairs_evaluated;
    double   max_distance;
} tm_wall_info;
enum { TM_WALL_NO_CULL = 1 };            /* evaluate every pair; same results */
/* distance: npoints doubles; face / image (may be NULL): npoints int32 each; info may be NULL.  On the device: one launch gathers the
 * faces into a primitive table with the bounding box of every group, one launch takes a point per lane and walks the groups wave by
 * wave -- a group is evaluated when any lane cannot rule it out by box bound > best + guard (guard = 40 * 2^-53 * rho2 of lane and group:
 * the error bound above plus the rounding of the box bound) -- and one launch combines the per-workgroup records in fixed order. */
int tm_wall_distance(int32_t dim, uint64_t nfaces, const int32_t* faces, uint64_t npoints, const double* const* points, uint64_t nimages,
                     const tm_wall_image* images, uint32_t flags, double* distance, int32_t* face_or_null, int32_t* image_or_null,
                     tm_wall_info* info_or_null);
/* the same definition as plain loops over all pairs: no GPU touched; flags are ignored */
int tm_wall_distance_host(int32_t dim, uint64_t nfaces, const int32_t* faces, uint64_t npoints, const double* const* points, uint64_t nimages,
                          const tm_wall_image* images, uint32_t flags, double* distance, int32_t* face_or_null, int32_t* image_or_null,
                          tm_wall_info* info_or_null);
/* Host only.  From tm_weld_boundary_plan(mesh, 1, nk): the faces of all patches whose kind bit is set in kinds_mask (bit k for kind k:
 * wall 1 << 0, unassigned 1 << 17, hub 1 << 18, shroud 1 << 19), patch-major, as indices into K19's face list; and the images: image 0,
 * then +T and -T for each distinct periodic translation of the plan (T and -T count as one) in first-occurrence order, t2 = 0, c = 1,
 * s = 0.  *nfaces and *nimages are written always; face_index / images may be NULL to count.  More than 16 images: TM_E_ARG. */
int tm_wall_select(const tm_mesh_desc* mesh, uint64_t nk, uint32_t kinds_mask, uint64_t* nfaces, int32_t* face_index_or_null, uint64_t* nimages,
                   tm_wall_image* images_or_null);
/* Wall distance of the coordinates RESIDENT in a handle, behind its pending work; modifies nothing.  Defined as tm_smoother_weld ->
 * tm_weld_boundary_faces (order 1) -> tm_wall_select -> tm_wall_distance on the welded X, Y: the points stay on the device, only the
 * outputs cross.  distance / face / image: nodes_out values; face is an index into K19's face list of the plan.  A NULL
 * block_orientation is taken by the rule of tm_smoother_quality.  No face selected, a dead handle, NULL distance: TM_E_ARG; rank hooks:
 * TM_E_UNSUPPORTED. */
int tm_smoother_wall_distance(tm_smoother* s, uint32_t kinds_mask, uint32_t flags, const int32_t* block_orientation_or_null, double* distance,
                              int32_t* face_or_null, int32_t* image_or_null, tm_wall_info* info_or_null);

/* ------------------------------------------------------------------ faces of the welded mesh (kernel K21)
 * A cell-centred finite-volume solver reads FACES with an owner and a neighbour cell, interior faces first in upper-triangular order,
 * then the boundary patch by patch, and judges a mesh by face non-orthogonality, skewness, closedness and negative volumes.  This section
 * gives the welded mesh that view at order 1 (the fine cells), over the SAME welded ids, and its metrics.  The lists are a pure function
 * of sizes and connections; the metrics are sums over the welded points (csrc/tm_fv.hpp holds every expression as code, in a fixed order,
 * nothing fused).
 * Definition.
 *   Cells        the cells of tm_weld_cells at order 1 in its order: cell (e, f) of block b, Ei = ni-1, Ej = nj-1, is cell0_b + f*Ei + e;
 *                with nk >= 2 layers cell0_b + (g*Ej + f)*Ei + e, g = 0 .. nk-2, cell0_b counting the hexahedra of the earlier blocks.
 *   Local sides  0 .. 3: the TM_SIDE_* value of the side of the cell (I_MIN the edge j = f, I_MAX j = f+1, J_MIN i = e, J_MAX i = e+1);
 *                with layers 4 is the side towards layer g and 5 the side towards layer g+1.  A cell has 4 (6) of them.
 *   Face shown   the face a cell shows on a side is the face the rules of "boundary of the welded mesh" give, at order 1, for a block that
 *                consists of this one cell and has the block's block_orientation: the ring counter-clockwise in index space (reversed for
 *                -1), lateral faces quadrilaterals over (a, c), side 4 by the hub rule and side 5 by the shroud rule, ids
 *                layer*nodes_out + map[...].  A boundary face of tm_weld_boundary_faces is therefore its owner's face on that side, and
 *                every face's normal (the tangent turned by -90 degrees; the right-hand rule of the ring) points OUT of the cell that shows it.
 *   Neighbour    across a side: inside the block the adjacent cell; across layers the cell of the same block one layer down / up; on a
 *                block side the cell behind the partner segment of the first connection WITHOUT periodicity that covers the segment
 *                (connections in order, r[0] before r[1]), in the same layer; otherwise none -- the side is a boundary face.  Periodic
 *                connections glue nothing.  A cell that is its own neighbour (a ring one cell around), or a segment whose partner does not
 *                name it back: TM_E_MISMATCH, naming block and side.
 *   Interior     one face per pair of sides that face each other: owner = the smaller cell, neighbour = the larger, the face is the
 *                OWNER's (its normal points owner -> neighbour).  Sorted by (owner, neighbour, owner's local side) ascending: two cells
 *                that share two faces (a ring two cells around) keep both.  ninternal = (faces_per_cell * cells - boundary faces) / 2.
 *   Boundary     the list of tm_weld_boundary_faces at order 1 in its order, as faces ninternal + t; the owner follows from `origin`.
 *   cell_faces   per cell and local side the face index.  The cell is the owner of that face iff owner[face] == cell.
 *   More than 2^31 - 1 faces: TM_E_ARG before anything is read.
 *   Face         area vector S: plane edge A -> B (yB - yA, -(xB - xA)); quadrilateral 0.5 (C - A) x (D - B) -- the terms of
 *                tm_weld_faces_measure, so the reversed ring gives exactly -S.  Centre Cf: the midpoint 0.5 (A + B); for a quadrilateral
 *                with m = 0.25 (((A + B) + C) + D) and the four triangles (m, P_k, P_k+1), w_k = |0.5 (P_k - m) x (P_k+1 - m)|:
 *                Cf = m + (sum w_k ((P_k - m) + (P_k+1 - m)) / 3) / sum w_k (m itself when sum w_k = 0).
 *   Cell         over its faces k in local side order, sign_k = +1 where the cell owns face k, else -1, mean = (sum Cf_k) / faces,
 *                dim = 2 or 3: v_k = sign_k (S_k . (Cf_k - mean)) / dim (the pyramid on face k with apex mean); volume V = sum v_k; centre =
 *                mean + (sum v_k * beta (Cf_k - mean)) / V with beta = 2/3 (dim 2) or 3/4 (dim 3) -- the V-weighted mean of the pyramid
 *                centroids (mean itself when V = 0); closedness = max_c |sum sign_k S_k,c| / max_c sum |S_k,c| (0 when the latter is 0).
 *   Interior face  d = C_nb - C_own (cell centres): cos = (d . S) / (|d| |S|), the non-orthogonality;
 *                skewness = |Cf - C_own - ((S . (Cf - C_own)) / (S . d)) d| / |d|: the distance of the face centre from the point where the
 *                line of centres meets the face's plane, over |d|.  This is THIS definition, not any particular solver's normalisation.
 *   Boundary face  the same cos with d = Cf - C_own; no skewness.
 *   Record       tm_fv_info below.  Extremes carry the smallest index at a tie and a NaN never wins one, so every field but total_volume is
 *                independent of the order of evaluation; an index is 0 when nothing qualifies.  Host and device form identical terms:
 *                every per-cell and per-face value and every extreme agree bit for bit; total_volume, summed in another order, agrees
 *                within 2 (n-1) 2^-53 sum |V|.  The device result is the same from run to run (no floating-point atomics).
 * Not served: high-order faces; gluing periodic sides; blocks spread over ranks; repair of bad cells; any solver's own checkMesh. */
typedef struct tm_fv_plan {              /* 40 bytes */
    uint64_t cells, internal_faces, boundary_faces, nodes_per_face, faces_per_cell;
} tm_fv_plan;
typedef struct tm_fv_info {              /* 144 bytes */
    uint64_t cells, internal_faces, boundary_faces;
    uint64_t min_volume_cell, max_volume_cell;
    uint64_t negative_cells, first_negative_cell;     /* cells with V <= 0 and the smallest of them */
    uint64_t max_closedness_cell;
    uint64_t min_cos_face;                            /* over all faces */
    uint64_t nonorthogonal_faces;                     /* interior faces with cos < cos 70 degrees */
    uint64_t inverted_faces;                          /* faces with cos <= 0 */
    uint64_t max_skewness_face;                       /* over the interior faces */
    double   min_volume, max_volume, total_volume, max_closedness, min_cos, max_skewness;
} tm_fv_info;
typedef struct tm_fv_fields {            /* 56 bytes; optional outputs of tm_fv_metrics, any may be NULL; vectors are component-major planes */
    double* volume;                      /* cells */
    double* centre;                      /* dim * cells */
    double* closedness;                  /* cells */
    double* area;                        /* dim * faces: S */
    double* face_centre;                 /* dim * faces: Cf */
    double* cos;                         /* faces */
    double* skewness;                    /* internal faces */
} tm_fv_fields;
/* Host only, closed form: the counts of the lists below for nk layers (nk <= 1: the plane mesh). */
int tm_weld_faces_plan(const tm_mesh_desc* mesh, uint64_t nk, tm_fv_plan* plan);
/* faces: (internal + boundary) * nodes_per_face ids; owner: one per face; neighbour: one per internal face; cell_faces (may be NULL):
 * faces_per_cell per cell.  map and nodes_out: tm_weld_map's; block_orientation as for tm_weld_boundary_faces.  On the device: the host
 * builds the table of the block-side segments (the perimeter is small); k_fv_count takes a cell per thread and counts its neighbours above
 * itself; the counts are scanned by K18's launches; k_fv_interior sorts the owned neighbours with a fixed network and writes owner,
 * neighbour, ring and both cell_faces slots -- plain stores to distinct addresses; k_fv_boundary adds K19's faces. */
int tm_weld_faces(const tm_mesh_desc* mesh, const int32_t* map, uint64_t nodes_out, uint64_t nk, const int32_t* block_orientation, int32_t* faces,
                  int32_t* owner, int32_t* neighbour, int32_t* cell_faces_or_null);
int tm_weld_faces_host(const tm_mesh_desc* mesh, const int32_t* map, uint64_t nodes_out, uint64_t nk, const int32_t* block_orientation, int32_t* faces,
                       int32_t* owner, int32_t* neighbour, int32_t* cell_faces_or_null);
/* Metrics of ANY such lists over welded planes (points[c]: component c, npoints doubles): dim = 2 edges with 4 faces per cell, dim = 3
 * quadrilaterals with 6.  Ids inside 0 .. npoints-1, owners inside the cells and not decreasing over the internal faces, neighbour >
 * owner, cell_faces naming faces of which the cell is owner or neighbour: TM_E_ARG otherwise, checked before anything is launched.  On the
 * device: one pass per cell through cell_faces, one pass per face, the record through the shared wave reduction. */
int tm_fv_metrics(int32_t dim, uint64_t ncells, uint64_t ninternal, uint64_t nboundary, const int32_t* faces, const int32_t* owner,
                  const int32_t* neighbour, const int32_t* cell_faces, uint64_t npoints, const double* const* points, const tm_fv_fields* fields_or_null,
                  tm_fv_info* info);
int tm_fv_metrics_host(int32_t dim, uint64_t ncells, uint64_t ninternal, uint64_t nboundary, const int32_t* faces, const int32_t* owner,
                       const int32_t* neighbour, const int32_t* cell_faces, uint64_t npoints, const double* const* points,
                       const tm_fv_fields* fields_or_null, tm_fv_info* info);
/* The record of the coordinates RESIDENT in a handle, behind its pending work; modifies nothing.  Defined as tm_smoother_weld ->
 * tm_weld_faces -> tm_fv_metrics on the welded X, Y: lists and points stay on the device, only the record crosses.  A NULL
 * block_orientation is taken by the rule of tm_smoother_quality.  A dead handle, NULL info: TM_E_ARG; rank hooks: TM_E_UNSUPPORTED. */
int tm_smoother_fv_report(tm_smoother* s, const int32_t* block_orientation_or_null, tm_fv_info* info);

/* ------------------------------------------------------------------ elliptic smoothing of stacked blocks (K22)
 * Jacobi relaxation of the 3-D Winslow equations on ONE stored block with its six faces held: the only stage that moves a node of a
 * stacked block.  Planes X, Y, Z in PLOT3D order, element (k*nj + j)*ni + i (what tm_stack_block returns for all layers, or a file read
 * back).  P(di,dj,dk) is a neighbour of node P; interior nodes have 1 <= i <= ni-2, 1 <= j <= nj-2, 1 <= k <= nk-2; every other node is
 * copied bit for bit by every sweep, so a node shared by two blocks stays identical on both sides.  ni, nj or nk < 2: TM_E_SIZE.  A block
 * without interior nodes is valid: no sweep is made, it comes back unchanged with sweeps_done = 0.
 *
 * One sweep, everything read from the input state of the sweep, IEEE fp64, nothing fused, sums left to right as written, per component
 * where a vector is meant:
 *   r1 = 0.5*(P(1,0,0) - P(-1,0,0)), r2 along j, r3 along k;  s1 = P(1,0,0) + P(-1,0,0), s2, s3 alike
 *   gab = (ra.x*rb.x + ra.y*rb.y) + ra.z*rb.z
 *   a11 = g22*g33 - g23*g23   a22 = g11*g33 - g13*g13   a33 = g11*g22 - g12*g12
 *   a12 = g13*g23 - g12*g33   a13 = g12*g23 - g13*g22   a23 = g12*g13 - g23*g11
 *   m12 = 0.25*(((P(1,1,0) - P(1,-1,0)) - P(-1,1,0)) + P(-1,-1,0)), m13 over (i, k), m23 over (j, k) alike
 *   num = (((a11*s1 + a22*s2) + a33*s3) + 2*((a12*m12 + a13*m13) + a23*m23)) + (((a11*f1)*r1 + (a22*f2)*r2) + (a33*f3)*r3)
 *   den = 2*((a11 + a22) + a33), inv = 1/den (one correctly rounded division per node), new = num*inv, out = P + omega*(new - P)
 * A node is frozen (out = P, counted) when den is not finite, is not > 0, or a component of num is not finite; den is twice the sum of
 * the principal 2 x 2 minors of the metric, so apart from overflow that is where r1, r2, r3 span less than a plane.  J = (r1.x*(r2.y*r3.z
 * - r2.z*r3.y) + r1.y*(r2.z*r3.x - r2.x*r3.z)) + r1.z*(r2.x*r3.y - r2.y*r3.x) is used by the record only.  19 points: the eight cube
 * corners are not read.
 *
 * Control field (f1, f2, f3), one double per node each.  TM_S3_LAPLACE: no field -- the second bracket of num is NOT FORMED (not
 * multiplied by 0), so a Laplace result does not depend on the field code.  TM_S3_THOMAS_MIDDLECOFF: formed once from the INPUT block
 * before the first sweep, then frozen.  Along a grid line at its node t (1 <= t <= n-2): d1 = 0.5*(r(t+1) - r(t-1)), d2 = (r(t+1) - r(t))
 * - (r(t) - r(t-1)), phi = -(d1.d2)/(d1.d1), 0 where d1.d1 is 0 or not finite.  f1 takes lines along i on the faces j = 0, j = nj-1,
 * k = 0, k = nk-1 and carries them inside by the boolean sum in (j, k), u = j/(nj-1), v = k/(nk-1):
 *   f1 = ((((1-u)*F_j0 + u*F_j1) + (1-v)*F_k0) + v*F_k1) - (((((1-u)*(1-v))*E00 + (u*(1-v))*E10) + ((1-u)*v)*E01) + (u*v)*E11)
 * with E the values on the four edge lines at the same i (Euv at u, v in {0, 1}).  f2: lines along j, u = i/(ni-1), v = k/(nk-1); f3:
 * lines along k, u = i/(ni-1), v = j/(nj-1).  The field is 0 on every node that is not interior.  TM_S3_PRESCRIBED: the caller's planes.
 *
 * Stopping: `sweeps` sweeps; with tol > 0 the call ends once sqrt(last_sum_sq / interior) <= tol, tested behind every 8th sweep and
 * behind the last -- the only host read-back inside a call.  sweeps = 0 returns the input and sweeps_done = 0.
 * 0 < omega <= 1, tol >= 0, a known algorithm, planes for TM_S3_PRESCRIBED, no NULL: TM_E_ARG otherwise.
 *
 * On the device (csrc/tm_smooth3d.hip): the whole block is held -- two states and the field; what does not fit: TM_E_MEMORY.
 * k_s3_control_faces and k_s3_control_blend form the field; k_s3_sweep takes an (i, j) tile per workgroup and marches along k with
 * the planes k-1, k, k+1 of the tile and a one-node rim in LDS, ping-pong between the two states; the record is combined in a fixed
 * order.  Host and device agree bit for bit in the planes, the field and every record field but the two sums; those agree within
 * 2 (n-1) 2^-53 sum and are the same from run to run. */
#define TM_S3_LAPLACE 0
#define TM_S3_THOMAS_MIDDLECOFF 1
#define TM_S3_PRESCRIBED 2
typedef struct tm_smooth3d_opt {   /* 56 bytes */
    int32_t algorithm;             /* TM_S3_* */
    int32_t _pad;
    uint64_t sweeps;
    double omega;                  /* 0 < omega <= 1 */
    double tol;                    /* 0: run all sweeps */
    const double* f1;              /* TM_S3_PRESCRIBED: nodes doubles each, read at interior nodes; ignored otherwise */
    const double* f2;
    const double* f3;
} tm_smooth3d_opt;
typedef struct tm_smooth3d_info {  /* 136 bytes; all counts over interior nodes */
    uint64_t nodes, interior, sweeps_done;
    uint64_t frozen;                                      /* of the last sweep */
    uint64_t first_neg, first_pos, first_zero_or_nan;     /* sign of J in the input of the first sweep */
    uint64_t last_neg, last_pos, last_zero_or_nan;        /* ... of the last sweep */
    uint64_t last_max_node;                               /* flat index; ~0 when no sweep was made or every update is a NaN */
    double first_sum_sq, last_sum_sq;                     /* sum of |out - P|^2 = (dx*dx + dy*dy) + dz*dz of the first / last sweep */
    double last_max_update;                               /* largest |out - P| by its square, the smallest flat index at a tie; a NaN never wins */
    double control_max[3];                                /* max |f| over the interior */
} tm_smooth3d_info;
int tm_smooth3d_planes(uint64_t ni, uint64_t nj, uint64_t nk, double* x, double* y, double* z /* in/out */, const tm_smooth3d_opt* opt,
                       tm_smooth3d_info* info);
/* the same definition on the CPU: no GPU touched */
int tm_smooth3d_planes_host(uint64_t ni, uint64_t nj, uint64_t nk, double* x, double* y, double* z, const tm_smooth3d_opt* opt,
                            tm_smooth3d_info* info);
/* The Thomas-Middlecoff field of a block: f1, f2, f3, nodes doubles each. */
int tm_smooth3d_control(uint64_t ni, uint64_t nj, uint64_t nk, const double* x, const double* y, const double* z, double* f1, double* f2,
                        double* f3);
int tm_smooth3d_control_host(uint64_t ni, uint64_t nj, uint64_t nk, const double* x, const double* y, const double* z, double* f1, double* f2,
                             double* f3);
/* All layers of `block` stacked from the K resident handles (K11) into a device buffer, smoothed there; only the planes (nlayers * nj * ni
 * doubles each) and the record cross to the host.  No handle is modified.  Errors: those of tm_stack_smoothers, and the ones above. */
int tm_stack_smoothers_smooth(tm_smoother* const* cuts, const tm_stack_opt* opt, uint64_t block, const tm_smooth3d_opt* smooth, double* x,
                              double* y, double* z, tm_smooth3d_info* info);
int tm_stack_smoothers_smooth_surf(tm_smoother* const* cuts, const tm_stack_opt* opt, const tm_stack_surfaces* surfaces, uint64_t block,
                                   const tm_smooth3d_opt* smooth, double* x, double* y, double* z, tm_smooth3d_info* info);

/* ------------------------------------------------------------------ host-only planning (no GPU needed)
 * The perimeter-row table the device kernels consume, exported as CSR so it can be compared with
 * the reference's assembled rows (smooth.zig:421-921).  Only sizes/topology are read from `mesh`
 * (coordinates may be NULL).  Arrays are malloc'ed by the library; free with tm_plan_free. */
typedef struct tm_plan_rows {
    uint64_t nrows;          /* number of perimeter rows of the whole mesh                         */
    int64_t* row;            /* [nrows] global row id, ascending                                   */
    int32_t* kind;           /* [nrows] BlockBoundaryPointKind                                     */
    int32_t* ncols;          /* [nrows]                                                            */
    int64_t* cols;           /* [nrows*9] global column ids, ascending                             */
    double* coef_x;          /* [nrows*9] x-system coefficients (NaN for `smoothed` rows: dynamic) */
    double* coef_y;          /* [nrows*9] y-system coefficients                                    */
    double* rhs;             /* [nrows*2] static rhs (NaN where it is taken from the coordinates)  */
    int32_t* slot;           /* [nrows*9] smoothed rows: StencilData index (smooth.zig:175-185) per column */
} tm_plan_rows;
int tm_plan_build(const tm_mesh_desc* mesh, tm_plan_rows* out);
void tm_plan_free(tm_plan_rows* rows);

/* Rank-local view of a partitioned mesh (host-only): which rows a rank owns, which remote rows it keeps copies of
 * (ghost rows, appended after the owned rows in every rank-local vector) and the halo exchange lists.
 * Every rank computes the same tables from the global topology, so no set-up communication is needed.
 * The halo is two rows deep: the remote rows the rank's perimeter rows read (the reference couples blocks through
 * smooth.zig:618-693, 994-1105: interface row, first interior row of either side, junction neighbours) -- listed in
 * ghost_row_* with their own columns -- AND the remote rows those read, so that a rank can evaluate the former one sweep
 * ahead and a PAIR of relaxation sweeps needs one exchange. */
typedef struct tm_plan_local_info {
    int64_t n_owned, n_ghost, n_send;
    int32_t npeers, nowned_blocks;
    int64_t* owned_blocks;   /* [nowned_blocks] global block ids, ascending                      */
    int64_t* local_start;    /* [nowned_blocks] rank-local index of node (0,0) of each of them   */
    int64_t* ghost_gid;      /* [n_ghost] global row ids, grouped by owner rank then ascending   */
    int32_t* send_ids;       /* [n_send] rank-local indices of the rows packed for the peers     */
    int64_t* send_gid;       /* [n_send] their global row ids                                    */
    int32_t* peer_rank;      /* [npeers]                                                         */
    int64_t* send_offset;    /* [npeers] rows; peer k gets send_ids[send_offset[k] .. +send_count[k]) */
    int64_t* send_count;
    int64_t* recv_offset;    /* [npeers] rows into the ghost segment                             */
    int64_t* recv_count;
    int64_t* send_first;     /* [npeers] first rank-local row of peer k's send list                            */
    int32_t direct_send;     /* 1: every peer's send list is one ascending run of local rows -- a handle then sends
                                straight from the vector (tm_smoother_exchange_plan offsets = send_first), no pack kernel */
    int32_t _pad;
    int64_t n_ghost_rows;    /* ghost rows this rank can evaluate itself (the depth-1 part of the halo)                 */
    int64_t* ghost_row_gid;  /* [n_ghost_rows]                                                                           */
    int32_t* ghost_row_kind; /* [n_ghost_rows] BlockBoundaryPointKind of the row, or 5 = interior node of the remote block */
    int64_t* ghost_row_cols; /* [n_ghost_rows * 9] global ids of its columns, -1 padded                                  */
} tm_plan_local_info;
int tm_plan_local(const tm_mesh_desc* mesh, const int32_t* owner, int32_t rank, int32_t nranks, tm_plan_local_info* out);
void tm_plan_local_free(tm_plan_local_info* info);

/* ------------------------------------------------------------------ device-level entry points
 * Same kernels on caller-provided DEVICE pointers and stream, for callers that keep blocks in
 * HBM (bench.py, the multi-GPU driver).  No allocation, no synchronisation. */
int tm_dev_tfi_block(double* d_xy, uint64_t ni, uint64_t nj,
                     const double* d_x_i_min, const double* d_x_i_max, const double* d_x_j_min, const double* d_x_j_max,
                     const double* d_s1, const double* d_s2, const double* d_t1, const double* d_t2, void* stream);
/* One fused Jacobi elliptic sweep of a single block with fixed boundary (Laplace control function):
 * d_out = d_in + omega * D^-1 (b - A(d_in) d_in) on interior nodes, boundary nodes copied;
 * d_partials[2*nwg] receives per-workgroup sums of (dx^2, dy^2); returns nwg through *nwg. */
int tm_dev_relax_sweep(const double* d_in, double* d_out, uint64_t ni, uint64_t nj, double omega,
                       double* d_partials, uint64_t partials_capacity, uint64_t* nwg, void* stream);
uint64_t tm_dev_relax_partials_needed(uint64_t ni, uint64_t nj);

#ifdef __cplusplus
}
#endif
#endif /* TM_HIP_H */
