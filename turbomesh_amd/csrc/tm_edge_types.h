// Descriptors of the perimeter-row kernels (K4/K5, k_edge_levels3) shared by the host planning (tm_edge_tables.cpp, pure C++)
// and the device code (tm_kernels.h includes this file).  No HIP header here.
#pragma once
#include <cstdint>

// ---- K4/K5 perimeter rows.  The rows of an interface are REGULAR: along a connection the row id, every column id and the
// four metric neighbours advance by constant strides while kind, column count, stencil slots and static coefficients stay
// the same (smooth.zig:518-616 fixes the column order per connection, not per point).  The host therefore compresses the
// per-row table of tm_plan into RUNS; a workgroup serves one stretch of one run, reads the run's descriptor through the
// scalar cache and computes its indices arithmetically, so the only vector loads of a row are the VALUES it gathers --
// one level of memory latency instead of two (index tables -> values), which is what a perimeter-row pass costs when it
// runs beside a bandwidth-saturating interior pass.  Irregular rows (connection end points, junctions) are runs of one.
struct EdgeRun {
    int32_t first, count;            // positions [first, first + count) of the run's rows in `rhs` (run order)
    int32_t row0, row_stride;        // local vector index of row k: row0 + k * row_stride
    int32_t col0[9], col_stride[9];  // its columns, ascending GLOBAL id order (the reference's CSR order)
    int32_t met0[4], met_stride[4];  // smoothed rows: im1_j, ip1_j, i_jm1, i_jp1
    int8_t kind, ncols, self;        // BlockBoundaryPointKind (5 = interior node of a remote block), #columns, diagonal position
    uint8_t flags;                   // bit0 periodic, bit1 swap (Q,P), bit2 / bit3: rhs_x / rhs_y = the row's current value (ghost copies), bit4: kind 5 row of an OWNED node (its displacement enters DOT_DELTA)
    int8_t slot[9];                  // smoothed rows: stencil slot per column
    int8_t _pad[3];
    double cx[9], cy[9];             // static x / y system coefficients
    double per[2];                   // periodicity of the row's connection
};
static_assert(sizeof(EdgeRun) == 296, "EdgeRun is read by the kernels through the scalar cache: its layout is fixed");
struct EdgeRowsDev {
    int nrows = 0;                      // rows in all runs
    int nwg = 0;                        // workgroups of a launch (= partial-sum rows it writes)
    const EdgeRun* runs = nullptr;
    const int32_t* wg_run = nullptr;    // [nwg] run served by workgroup w
    const int32_t* wg_k0 = nullptr;     // [nwg] first point of the run it serves
    const double* rhs = nullptr;        // [nrows*2] static right-hand side, run order
};
constexpr int EDGE_BLOCK = 128;
// The three level passes of a coupled sweep triple in ONE launch (Smoother::relax_triples_coupled): the rows of level 3 are cut into
// strips along their grid lines; a workgroup owns one strip and evaluates -- redundantly, with the very run descriptors of the three
// level tables -- every level-1 and level-2 row its strip depends on (the closure is computed on the host), level by level with a barrier
// in between.  What a workgroup reads at level l it wrote itself at level l - 1 (or nobody writes it at all), so no workgroup waits for
// another; neighbouring strips store the same bits where their closures overlap.  One kernel boundary instead of three on the
// latency-critical chain.  A task = up to 64 consecutive points of one run, taken by one wave (the descriptor stays wave-uniform).
struct LevelTask {
    int32_t run, k0, count;
};
struct FusedLevelsDev {
    int nstrips = 0;
    const LevelTask* tasks = nullptr;   // all strips, level by level
    const int32_t* off = nullptr;       // [nstrips * 4]: tasks of level l of strip s are off[4 s + l] .. off[4 s + l + 1]
};
constexpr int LEVELS_BLOCK = 512;   // (1024: no faster -- 2048^2 rank 11.9 against 10.8-11.8 us per sweep -- and twice the LDS)
