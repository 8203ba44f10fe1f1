// Device-resident smoother handle (internal).  One handle = one rank's share of a mesh.
#pragma once
#include "../../include/tm_hip.h"
#include <cstdlib>
#include "tm_edge_tables.hpp"
#include "tm_kernels.h"
#include "tm_krylov.hpp"
#include "tm_multigrid.hpp"
#include "tm_plan.hpp"
#include <cmath>
#include <atomic>
#include <memory>
#include <string>
#include <functional>
#include <vector>

namespace tmh {

struct TmError : std::runtime_error {
    int code;
    TmError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
void hip_check(hipError_t e, const char* what);
// per-iteration log sink (tm_set_log), process-wide like the reference's std.log
extern std::atomic<int> g_multirank_handles;   // live handles with comm hooks in this process
extern tm_log_fn g_log_sink;
extern void* g_log_ctx;

// Bump allocator over either library-owned hipMalloc chunks or a caller-provided workspace.
class DeviceArena {
   public:
    DeviceArena() = default;
    ~DeviceArena();
    void use_workspace(void* base, uint64_t bytes);   // carve from caller memory
    void measure_only();                              // only count bytes (tm_smoother_workspace_bytes)
    void* alloc(uint64_t bytes);
    template <class T>
    T* alloc_n(uint64_t n) { return static_cast<T*>(alloc(n * sizeof(T))); }
    uint64_t used() const { return used_; }
    bool measuring() const { return measure_; }

   private:
    std::vector<void*> owned_;
    char* base_ = nullptr;
    uint64_t cap_ = 0, used_ = 0;
    bool external_ = false, measure_ = false;
};

struct QualityDev;
struct HoDev;
struct WeldDev;
struct HcDev;

struct Smoother {
    Smoother() = default;
    ~Smoother();
    Smoother(const Smoother&) = delete;
    Smoother& operator=(const Smoother&) = delete;
    Topology topo;
    std::vector<PlanRow> all_rows;
    LocalPlan lp;
    tm_solver_opt opt{};
    tm_control_fn cf{};
    tm_comm_hooks hooks{};
    bool has_hooks = false;
    std::vector<int32_t> owner;
    hipStream_t stream = nullptr;
    DeviceArena arena;

    int64_t n_owned = 0, n_local = 0, n_ghost = 0, dof_global = 0;
    // vectors, double2[n_local]
    double2 *X = nullptr, *U = nullptr, *r = nullptr, *r_hat = nullptr, *p = nullptr, *v = nullptr, *s = nullptr, *t = nullptr;
    double2 *PQ = nullptr, *tmpA = nullptr, *tmpB = nullptr;
    // multigrid preconditioner (TM_INNER_MG_BICGSTAB): preconditioned search directions, two scratch vectors, one hierarchy per owned block
    double2 *p_hat = nullptr, *s_hat = nullptr, *mg_w0 = nullptr, *mg_w1 = nullptr;
    std::vector<BlockMG> mg;
    bool use_mg = false;
    bool mg_perimeter_step = false;   // the preconditioner applies the perimeter rows to the interior corrections (precondition())
    bool mg_dirichlet = false;   // ... and hands the perimeter values to the cycles as Dirichlet data (precondition())
    // the cycles of a multi-block mesh run side by side: one stream per block (at most 8), forked from and joined to the handle's stream by events
    std::vector<hipStream_t> mg_streams;
    std::vector<hipEvent_t> mg_join;
    hipEvent_t mg_fork = nullptr;
    int mg_perimeter_sweeps = 2;   // passes of the perimeter rows behind the cycles: the first on (e_I, 0), the others Jacobi sweeps on the perimeter system
    void precondition(const double2* in, double2* out);
    void precondition_probe_host(const double* f, double* z, double* f_after);   // tm_smoother_precondition_probe
    double2* M = nullptr;           // X^(k+1) of a fused pair of relax sweeps (perimeter + first-interior ring only)
    double2* M2 = nullptr;          // coupled triples: X^(k+2) on the perimeter and in the zone next to sides whose perimeter rows move
    bool fuse_pairs = false;
    bool relax2_store_nt = true;     // K2x2 result stores streaming (nt) or plain: by the rank's footprint against the Infinity Cache (decide_schedule())
    bool pair_sync_events = false;   // TM_PAIR_SYNC=events when the handle was created: multi-rank sweep pairs ordered by events, not device counters
    size_t inside_lds = 0;          // dynamic LDS of the interior pass of a multi-rank sweep pair (occupancy cap, see decide_schedule())
    // perimeter rows (run tables: tm_edge_tables.cpp)
    EdgeRowsDev edge;
    std::vector<double> h_rhs;   // host copy of the static rhs (refilled on upload), lp.rows order; never resized after create (rhs_tables point into it)
    // per run table, in the order they were built: the device right-hand sides and, per position in run order, where the pair comes
    // from -- a slot of h_rhs, a ghost row's static rhs (lp.ghost_rows / ghost_rows2) or the zero pair of an interior row
    struct RhsTable {
        double* dev = nullptr;
        std::vector<const double*> src;
    };
    std::vector<RhsTable> rhs_tables;
    // relax mode: the perimeter rows that are not `fixed` (the only ones a sweep has to evaluate), and per owned block which
    // sides carry such rows (moving_sides)
    EdgeRowsDev edge_nf;
    EdgeRowsDev edge_nf_g;          // the same + the depth-1 ghost rows (multi-rank sweep pairs; empty otherwise)
    std::vector<int> dyn_mask;
    std::vector<const int32_t*> border_ids;   // per owned block: device list of the K2x2 border tiles
    std::vector<int> border_n;
    void prefill_fixed();   // perimeter of X -> perimeter of U and M
    // reductions: the partial-sum buffers, their sums and the Krylov scalar block live in the lazy scalar queue (tm_krylov.hpp)
    LazyScalarQueue lsq;
    double*& partials = lsq.partials;
    double*& red = lsq.red;
    KrylovScalars*& S = lsq.S;
    KrylovScalars* h_S = nullptr;   // pinned
    // pipelined convergence poll (poll_done): two pinned copies of the scalar block in flight alternately
    bool pipelined_poll = false, poll_open = false;
    KrylovScalars* h_poll[2] = {nullptr, nullptr};
    hipEvent_t ev_poll[2] = {nullptr, nullptr};
    uint64_t poll_it[2] = {0, 0}, poll_iters = 0;
    int poll_slot = 0;
    int poll_done(uint64_t it, bool final);
    StallWatch stall;   // stagnation watch of the inner solve (poll_done)
    double* h_red = nullptr;        // pinned
    // the two-kernel Krylov iteration of a large mesh runs its kernels on overlapping 62-column strips (apply_tile<.., OV>): their own
    // partial-row layout (more strips per block than the 64-column tiling)
    bool vk_overlap = false;
    std::vector<int> poff_ov;
    int poff_edge_ov = 0, nwg_apply_ov = 0;
    std::vector<int> poff;          // partial-row offset of each owned block's K2 launch
    int poff_edge = 0, nwg_apply = 0, nwg_vec = 0;
    std::vector<int> poff2, rows2;  // same for the fused two-sweep launches, and their rows per workgroup
    int poff2_edge = 0, nwg_apply2 = 0;
    struct FixedWallPlan { std::vector<int> poff, rows; int nwg = 0; };   // ... and for a depth of the fixed-wall pass (K2x3 / K2x4)
    FixedWallPlan plan3, plan4;     // three sweeps per pass (all perimeter rows fixed, or coupled triples); four (where fuse_quads holds)
    bool fuse_triples = false;
    bool fuse_quads = false;        // fuse_triples, every block 9 x 9 or larger; TM_FUSE_4=0 at creation: the schedule of triples alone, same binary
    static constexpr int64_t QUAD_MIN_NODES = 8000000;         // nodes per launch from which a quad beats a triple per sweep (measured)
    // Coupled triples (single process): K2x3 with a frozen perimeter stores everything but the nodes within two of a side whose
    // perimeter rows move; three perimeter-row passes evaluate the perimeter and that zone level by level (rows within 4 / 3 / 2 nodes)
    bool triples_coupled = false;
    EdgeRowsDev edge_L[3];          // zone rows (zone_rows): level 1: distance <= 4, level 2: <= 3, level 3: <= 2
    bool levels_fused = false;               // the three level passes of a coupled triple in one launch (k_edge_levels3; TM_LEVELS_FUSED=0: three launches)
    FusedLevelsDev fused_levels;
    bool pipelined_single = false;   // single process, coupled blocks: perimeter-row passes on the chain's queue beside the interior pass
    // halo exchange
    int32_t* d_send_ids = nullptr;
    double2* d_send_buf = nullptr;
    int64_t n_send = 0;
    // white control function
    bool white = false;
    ConnShifts white_le{};
    // a per-node (P,Q) field exists: every kind but laplace.  `white` above = White's O4H algorithm runs on it; the prescribed and the
    // Thomas-Middlecoff field are frozen over the outer iterations and change only through the three calls below
    bool has_field = false;
    bool thomas_middlecoff() const { return cf.kind == TM_CF_THOMAS_MIDDLECOFF; }
    TmFieldBlock* tmf_table = nullptr;   // K10 (tm_control.hip): block table and edge scratch, carved from the arena (Thomas-Middlecoff handles)
    double* tmf_scratch = nullptr;
    int tmf_nwg_edges = 0, tmf_nwg_blend = 0;
    void tm_field_launch();                            // PQ of every owned block from the resident coordinates (asynchronous)
    void set_control_function_host(const double* pq);  // tm_smoother_set_control_function
    void update_control_function();                    // tm_smoother_update_control_function
    uint64_t outer_done = 0;
    // measurement: HIP event pairs around K2 launches
    int profile = 0;                // 0 = off, k > 0 = every k-th launch of the dominant kernel is bracketed
    std::vector<hipEvent_t> ev_start, ev_stop;
    size_t ev_used = 0;
    uint64_t prof_launches = 0;     // event pairs that count as a launch of the dominant kernel (the parts of a split K2x2 pass count once)
    uint64_t prof_timed = 0;        // ... of which carried an event pair
    uint64_t prof_open = 0;         // launches inside the group bracket that is open (see profiled)
    uint64_t prof_phase = 0;        // position within the bracketed / unbracketed alternation
    void profile_close(hipStream_t on);
    void profile_read(double* ms_total, uint64_t* launches, uint64_t* timed);

    void create(const tm_mesh_desc* mesh, const tm_solver_opt* o, const tm_control_fn* c, const tm_comm_hooks* h, void* strm,
                bool measure);
    void upload(const tm_mesh_desc* mesh);
    void download(const tm_mesh_desc* mesh);
    void iterate(uint64_t iterations, tm_stats* stats);
    bool iterate_until(uint64_t max_iterations, double tol, tm_stats* stats);          // true = the scaled residual reached tol
    bool iterate_until_update(uint64_t max_iterations, double tol, tm_stats* stats);   // true = the update of the last outer iteration was <= tol
    double stop_tol = 0.0;          // > 0: a Picard iteration whose start residual is already <= stop_tol returns without solving
    void apply_host(const double* in_xy, double* out_xy, int scaled);
    // the reference's assembled system for the current coordinates (tm_smoother_assemble_csr) and A in through it, in CSR order
    // (tm_smoother_apply_reference_order); single-process handles
    uint64_t assemble_csr_host(int32_t* Ap, int32_t* Ai, double* Ax_x, double* Ax_y, uint64_t nnz_capacity);
    void apply_reference_host(const double* in_xy, double* out_xy);
    struct AssembledCsr {            // device copy, built on demand, dropped by the next iterate / upload
        int32_t *p = nullptr, *i = nullptr;
        double *vx = nullptr, *vy = nullptr;
        uint64_t nnz = 0;
        std::vector<int32_t> h_p, h_i;
    } csr;
    void csr_build_pattern();
    void csr_fill_values();
    void csr_release();              // frees the device copy -- unless the handle keeps it for its lifetime (ref != nullptr)
    void csr_free();
    void rhs_host(double* rhs_xy);
    void residual_host(const double* xy, double* r_xy);   // tm_smoother_residual
    void control_function_host(double* pq);
    void export_soa_host(int64_t block, double* x, double* y, double* p, double* q);
    void* export_buf = nullptr;     // scratch planes of export_soa_host (hipMalloc, grown on demand)
    size_t export_bytes = 0;
    // mesh quality report of the resident coordinates (tm_quality.hip): reads X only; its buffers (a few KB of records, one cell plane
    // for the field) are hipMalloc'ed on first use OUTSIDE the arena, so a caller-provided workspace is sized as before
    QualityDev* qdev = nullptr;
    void quality_host(tm_quality* per_block, tm_quality* total);
    void quality_field_host(int64_t block, double* out);
    // high-order elevation of an owned block from the resident coordinates (tm_highorder.hip): reads X only; buffers as for the quality report
    HoDev* hodev = nullptr;
    void elevate_host(const tm_ho_opt* opt, int64_t block, double* x, double* y, tm_ho_quality* q, double* sj);
    // certificate of an owned block's elements from the resident coordinates (tm_highorder_cert.hip): K13's report through hodev, then K14
    HcDev* hcdev = nullptr;
    void certify_host(const tm_ho_opt* opt, int max_depth, int64_t block, tm_ho_certificate* cert, uint8_t* status, double* bounds);
    // welded map and points of the resident coordinates (tm_weld.hip, K18): reads X only; buffers as for the quality report
    WeldDev* welddev = nullptr;
    void weld_host(int32_t* map, double* x, double* y, tm_weld_info* info);
    void weld_tables(std::vector<tm_block>& tb, std::vector<tm_connection>& tc, std::vector<tm_condition>& tq, std::vector<const double2*>& blocks_x);
    // boundary faces and patch measures of the resident coordinates (tm_weld_boundary.hip, K19): the welded planes stay on the device
    void weld_boundary_host(int order, const int32_t* block_orientation, int32_t* faces, int32_t* face_patch, tm_weld_patch* patches);
    // wall distance of the resident coordinates (tm_wall_distance.hip, K20): welded planes and outputs stay on the device until the end
    void wall_distance_host(uint32_t kinds_mask, uint32_t flags, const int32_t* block_orientation, double* distance, int32_t* face, int32_t* image,
                            tm_wall_info* info);
    // finite-volume record of the resident coordinates (tm_fv.hip, K21): welded planes, face lists and fields stay on the device
    void fv_report_host(const int32_t* block_orientation, tm_fv_info* info);

    // building blocks
    void exchange(double2* vec, hipStream_t on = nullptr);   // start (and, without a split hook, finish) the halo exchange of `vec`; on = the handle's stream unless given
    void exchange_finish(hipStream_t on = nullptr);          // split hooks: make the stream wait for the transfer started by exchange()
    // second stream of a multi-rank relax handle: halo exchanges and perimeter rows of a sweep pair run here, beside the interior pass
    hipStream_t side = nullptr;
    hipEvent_t ev_to_side = nullptr, ev_to_main = nullptr, ev_inside[2] = {nullptr, nullptr};
    void fence(hipStream_t from, hipStream_t to, hipEvent_t ev);
    // How the two queues of a pipelined pass (interior pass on the handle's stream, chain on `side`) are ordered against each other.
    // Counters in device memory + one-wave announce / wait kernels need the two streams on DIFFERENT hardware queues (a waiter whose
    // producer sits behind it in the same in-order queue never sees it start); HIP does not promise that, so the handle finds out: once,
    // when `side` is created, one announce-and-wait round in both directions with a limit of milliseconds (queue_self_test).  Events
    // (barrier packets, ~10 us per hop, no assumption) are used when the test fails, when TM_PAIR_SYNC=events asks for them, and when
    // several multi-rank handles share the process.
    enum { ORDER_UNDECIDED = -1, ORDER_COUNTERS = 0, ORDER_EVENTS_REQUESTED = 1, ORDER_EVENTS_SHARED_PROCESS = 2, ORDER_EVENTS_SELF_TEST = 3 };
    int queue_ordering = ORDER_UNDECIDED;
    void ensure_side();              // creates `side` and its events, runs the self-test (first use)
    bool queue_self_test();          // true = the two streams ran side by side
    bool use_counters();             // the decision for the pass being enqueued
    bool transport_warm = false;     // the first exchange of a handle runs alone and synchronised (connections are set up inside it)
    void warm_transport();
    void relax_pairs_pipelined(uint64_t npairs, bool want_partials_last);
    uint32_t* sync_flags = nullptr;   // device counters of the cross-queue dependencies of a sweep pair (k_queue_signal / k_queue_wait)
    uint32_t* h_flags = nullptr;      // pinned
    bool flags_pending = false;
    bool counted = false;             // this handle is one of g_multirank_handles
    bool exchange_pending = false;
    // step >= 0: the Krylov scalar update that consumes the fused dot products follows the reduction (one launch without hooks)
    void apply(const double2* in, double2* out, int mode, int dot, const double2* aux, const double2* xk, double omega, int step = -1);
    void reduce(int nwg);   // partials -> red (+ all-reduce)
    int apply_rows = 0;             // K2 rows per chunk of this handle (0 = per-block rule)
    bool fuse_s = false;            // k_apply_vk<VK_S> / k_xr_update_vs instead of k_s_update + apply + k_xr_update
    bool fuse_p = false;            // k_apply_vk<VK_P> instead of k_p_update + apply; p and v alternate with p_alt, v_alt
    bool fuse2 = false;             // two kernels per iteration: k_apply_vk<VK_R> + k_apply_vk<VK_S2>; r alternates with r_alt
    double2 *p_alt = nullptr, *v_alt = nullptr, *r_alt = nullptr;
    void apply_virtual(int kind, const double2* in, const double2* in2, const double2* in3, double2* pout, double2* out, const double2* in4 = nullptr,
                       double2* rout = nullptr, double2* uio = nullptr);
    // TM_PARTIALS_GUARD (see alloc_reductions): a guard region behind lsq.part_buf[0..2] and behind red, compared by check_guards
    static constexpr uint64_t GUARD_DOUBLES = 2048 * MAX_PARTIALS;
    static constexpr int GUARD_BYTE = 0xA5;
    bool partials_guard = false;
    double* guard[4] = {nullptr, nullptr, nullptr, nullptr};
    void check_guards();
    void white_launch(int update);
    void sync();
    void ensure_tmp();

    // GMRES(30) (TM_INNER_GMRES; csrc/tm_gmres.hip): the m + 1 basis vectors, the device-resident Hessenberg / rotation state, a pinned copy
    double2* gm_V = nullptr;
    GmresScalars* gm_S = nullptr;
    GmresScalars* h_gm = nullptr;

    // TM_INNER_REFERENCE_GMRES: the reference's own route on the device -- the ASSEMBLED, unscaled system of every outer iteration (csr, kept
    // for the handle's lifetime), GMRES(30) left-preconditioned with ILU(0) or the diagonal, the reference's stop test (picard_reference).
    // Single-process handles only.
    struct ReferenceSolve;
    ReferenceSolve* ref = nullptr;
    void reference_create();
    double2* ref_b = nullptr;        // the unscaled right-hand side
    // TM_OPT_REFINE (refine_solution): double-double residual, correction and 1 / a_ii of the assembled system (ref_b: its right-hand side);
    // the figures of tm_smoother_refine_report
    double2 *rf_r = nullptr, *rf_d = nullptr, *rf_dinv = nullptr;
    uint32_t refine_steps = 0;        // steps of the last outer iteration (both components advance together)
    double refine_rel[2] = {0.0, 0.0};   // ||d|| / ||x|| of its last step
    double refine_rtol = 0.0;         // stop test of the corrections, relative to ||D^-1 r||
    uint64_t refine_iterations = 0;   // inner iterations spent in corrections over the handle's life
    bool refine() const { return (opt.flags & TM_OPT_REFINE) != 0; }
    uint64_t inner_counts[2] = {0, 0};   // inner iterations of the last outer iteration per component (tm_smoother_inner_counts)

   private:
    // create(), step by step
    struct Selection;
    bool reference() const { return opt.inner == TM_INNER_REFERENCE_GMRES; }
    double2* vec() { return arena.alloc_n<double2>(static_cast<uint64_t>(n_local)); }
    void resolve_options(const tm_mesh_desc* mesh, const tm_solver_opt* o, const tm_control_fn* c, const tm_comm_hooks* h, bool measure);
    void plan_mesh(const tm_mesh_desc* mesh, const tm_comm_hooks* h, bool measure);
    void alloc_vectors(const tm_mesh_desc* mesh, bool measure);
    void decide_schedule();
    void* upload_table(const void* src, uint64_t bytes);   // arena memory holding a host table (the sizing call only counts it)
    RunTable make_table(const Selection& sel, EdgeRowsDev& e);
    void build_row_tables();
    uint64_t size_launches();
    void alloc_reductions(uint64_t npart);
    void finish_create(const tm_mesh_desc* mesh);
    int picard_bicgstab(tm_stats& st);
    int picard_gmres(tm_stats& st);
    int picard_reference(tm_stats& st);
    void begin_outer();                 // what every picard_* starts with: the control function's update, the exchange of X
    void finish_outer(tm_stats& st);    // ... and ends with: residual and copy-back, X becomes the new frozen field
    BicgVectors bicg_vectors() { return {r, p, v, s, t, use_mg ? p_hat : p, use_mg ? s_hat : s, r_hat, n_owned, nwg_vec}; }
    GmresSpace gmres_space() { return {gm_S, gm_V, n_local, r, n_owned, partials, red, stream}; }
    bool gmres_poll();                  // the flags of both components, after everything enqueued so far
    void refine_solution();
    uint64_t correct_bicgstab(const double2* rhs, double2* d);
    uint64_t correct_gmres(const double2* rhs, double2* d);
    int picard_solve(tm_stats& st) {
        const uint64_t before = st.inner_iterations;
        if (opt.inner == TM_INNER_REFERENCE_GMRES) return picard_reference(st);
        const int rc = opt.inner == TM_INNER_GMRES ? picard_gmres(st) : picard_bicgstab(st);
        inner_counts[0] = inner_counts[1] = st.inner_iterations - before;   // both components advance together
        return rc;
    }
    void relax_sweeps(uint64_t n, tm_stats& st);
    void relax_pair(bool want_partials);
    FixedWallPlan plan_fixed_walls(int depth, bool beside_chain) const;
    // the owned blocks as the fused-sweep kernels take them; mid == nullptr / dyn, borders false: K2x3 / K2x4 use none of them
    std::vector<Relax2Block> relax_blocks(const double2* in, double2* mid, double2* out, bool dyn, bool borders, const std::vector<int>& poff) const;
    void relax_fixed_walls(int depth, bool want_partials);
    void relax_triples_coupled(uint64_t ntriples, bool want_partials_last);
    void profiled(const std::function<void()>& launch, bool counts = true, hipStream_t on = nullptr);
    void relax2_launch(int subset, bool counts, int dot, hipStream_t on = nullptr, const QueueWait* wait = nullptr);
};

// Defaults of the inner solve that depend on the size of the system (tm_solver_opt.rtol == 0, max_inner == 0).
// The stop test bounds the scaled RESIDUAL; the distance of the Picard iterate from the exact-solve iterate -- what north_star's
// 1e-10 RMS is about -- is conditioning x residual, and cond(D^-1 A) of the frozen Winslow system grows like the node count.
// Measured with the diagonal-only BiCGStab against the sparse-LU oracle on perturbed n^2 blocks (tests/test_gpu_parity_ladder.py,
// tools/dev/picard_ladder.py): rms error ~ 4e-17 .. 1e-16 x nodes x (rtol / 1e-14) -- 2e-11 at 1025^2,
// 6.5e-11 at 2049^2 and 6e-10 at 4096^2 with rtol 1e-14.  Hence rtol = 7.5e-9 / nodes, between 1e-16 and 1e-14: every size lands
// at <= 3e-11, for 0-40 % more inner iterations on the large meshes (the recurrence residual keeps falling; no stagnation seen down
// to 1e-16).  The iteration cap grows with the mesh too: BiCGStab with the diagonal alone needs ~3-5 sqrt(nodes) iterations.
// Will a handle with these options ever run sweep TRIPLES across ranks (the only schedule that needs the depth-3 halo)?  A pure function of
// the options (and of TM_TRIPLES_COUPLED in the environment), identical on every rank of a job.
inline bool triples_wanted(const tm_solver_opt& o, const tm_control_fn& c) {
    if (o.inner != TM_INNER_RELAX || c.kind != TM_CF_LAPLACE || (o.flags & TM_OPT_SINGLE_SWEEP)) return false;
    if (const char* e = std::getenv("TM_TRIPLES_COUPLED")) return std::atoi(e) != 0;
    return true;
}
// the library's own transport: non-negative = the depth its tables were built for (0: depth 2, 1: depth 3 where the topology has it); -1 = foreign hooks
int rccl_hooks_allow_triples(const tm_comm_hooks* h);

// TM_INNER_AUTO: the multigrid-preconditioned solve from this many nodes in the largest block on (include/tm_hip.h)
constexpr uint64_t AUTO_MG_MIN_BLOCK_NODES = 100000;
constexpr uint64_t AUTO_MG_MIN_LONE_BLOCK_NODES = 1000;   // ... and from this many when no connection couples the blocks (tm_smoother.cpp)
// ... unless the cells' aspect ratio VARIES inside a block (standard deviation of log(g11/g22) over the block's nodes above this): the cycle
// smooths with point Jacobi and coarsens a block by one rule, so boundary-layer clustering (the reference's O-grids: 1.4-1.8; the
// uniform synthetic blocks: 0.3) leaves it a poor preconditioner -- T106 / LS89 refined to 0.9 / 1.3 M nodes: 14.5 / 21 s against
// 5.5 / 12 s with the plain solve (tools/dev/o4h_auto_probe.py)
constexpr double AUTO_MG_MAX_ASPECT_SPREAD = 1.0;

inline double default_rtol(double nodes) {
    const double r = 7.5e-9 / (nodes > 1.0 ? nodes : 1.0);
    return r > 1e-14 ? 1e-14 : (r < 1e-16 ? 1e-16 : r);
}
inline uint64_t default_max_inner(double nodes) {
    const double k = 12.0 * std::sqrt(nodes > 1.0 ? nodes : 1.0);
    return k > 10000.0 ? static_cast<uint64_t>(k) : 10000u;   // the reference caps at 1000 (BiCGStab.zig:19) -- with its far looser stop test
}

}  // namespace tmh

struct tm_smoother {
    tmh::Smoother impl;
};
