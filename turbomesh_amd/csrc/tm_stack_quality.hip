// K12  stack_quality: the 3-D quality report of a stacked block (include/tm_hip.h, "3-D quality of stacked blocks") in one pass over the
//      K cuts -- negative / degenerate hexahedra across layers, scaled Jacobian with its worst cell and histogram, aspect, spanwise growth,
//      volumes -- without the 3-D block ever being stored.  gfx950, wave64.  The per-cell arithmetic is tm_quality3d.h, shared with the
//      host loop; the node positions are formed with K11's expression (tm_stack.hip), so the report sees bit for bit the block K11 writes.
//
// Layout.  A workgroup of 256 threads holds a tile of SQ_TILE x SQ_TILE = 16 x 16 nodes, thread t node (i0 + t/16, j0 + t%16): the K cut
// values of the node are loaded once (16 B per lane, 16 lanes = 256 contiguous bytes along j, all K loads in flight together) and stay in
// registers under compile-time indices (K is a template parameter, the loops over it are unrolled).  The workgroup then MARCHES over the
// layers.  At layer k every thread
//   1. forms its node's position (2 K multiply-adds; one sincos with the cylindrical mapping) and the k-edge to its own previous position,
//   2. publishes the position in LDS; barrier; reads the positions of its i- and j-neighbour and forms its i-edge and j-edge,
//   3. publishes the three edge lengths; barrier; reads what the cell below still lacks -- the fourth position of the layer, one i-edge,
//      one j-edge and three k-edges of the neighbours -- and evaluates the eight corners, the volume and the aspect of cell (i, j, k-1).
// The layer below is carried in registers (4 positions, 4 edge lengths), so a cell costs 14 LDS reads of 8 B and the two LDS buffers
// alternate with no third barrier: a buffer is rewritten two barriers after its last read.  Every edge length is ONE square root -- by
// the thread that holds the edge's lower node -- shared through LDS by the four cells and the growth pair that use it.
// Tiles overlap by one node row and column: a tile owns SQ_OWN x SQ_OWN = 15 x 15 cell columns (88 % of the lanes evaluate a cell they
// own; the seam nodes are loaded and positioned twice).  Extremes are idempotent, so the overlap only matters for counts and sums:
// cells are counted by their owner alone.  Lanes past the block repeat its last row / column; what they compute is masked.
//
// Reductions: in-lane over the march, in-wave by shuffles, across the 4 waves through LDS, one Q3Acc record per workgroup; the histogram
// by integer LDS atomics.  k_stack_quality_finalize (one launch, one wave) combines the records in fixed order and picks the
// orientation's candidate set (q3_finish).  No floating-point atomics anywhere: the result does not depend on scheduling.
//
// Traffic: 16 K bytes per node read (x 1.14 for the seams), one 264 B record per workgroup written; nothing else touches HBM.
// Compiler's resource usage (cross-compile, -Rpass-analysis=kernel-resource-usage): DESIGN.md section 4, K12.
#include "tm_quality3d.h"
#include "tm_stack_dev.hpp"
#include "tm_dispatch.hpp"
#include "tm_records.hpp"

#include <cstring>

namespace tmh {

constexpr int SQ_TILE = 16, SQ_OWN = SQ_TILE - 1, SQ_THREADS = SQ_TILE * SQ_TILE, SQ_WAVES = SQ_THREADS / 64;

__device__ __forceinline__ unsigned long long sq_shfl(unsigned long long v, int off) { return __shfl_down(v, off, 64); }

// table: per layer K weights followed by s[k] (row pitch K + 1), all nk layers.  Node layers [k0, k1] are marched, i.e. the cell layers
// [k0, k1).  partials: one record per workgroup, or null when only the field is wanted; field: per-cell min of o*s, element
// ((k - k0)*(nj-1) + j)*(ni-1) + i, or null.
template <int K, int MAP>
__global__ __launch_bounds__(SQ_THREADS) void k_stack_quality(StackCuts cuts, StackSurf surf, const double* __restrict__ table, int k0, int k1, int ni, int nj,
                                                              Q3Acc* __restrict__ partials, double* __restrict__ field, int orientation) {
    constexpr bool REV = MAP == TM_STACK_REVOLUTION;
    static_assert(TM_STACK_MAX_KNOTS <= SQ_THREADS, "one thread stages one knot");
    __shared__ double sh_u[REV ? 2 : 1][REV ? TM_STACK_MAX_KNOTS : 1];
    __shared__ double sh[2][6][SQ_THREADS];   // per buffer: x, y, z, then the lengths of the node's i-, j- and k-edge; one column per thread
    __shared__ unsigned sh_hist[20];
    __shared__ Q3Acc sh_acc[SQ_WAVES];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int ti = t / SQ_TILE, tj = t % SQ_TILE;
    if (t < 20) sh_hist[t] = 0;   // ordered before the first atomic by the barriers of the first layer

    const int i0 = static_cast<int>(blockIdx.y) * SQ_OWN, j0 = static_cast<int>(blockIdx.x) * SQ_OWN;
    const int i = i0 + ti < ni ? i0 + ti : ni - 1, j = j0 + tj < nj ? j0 + tj : nj - 1;   // lanes past the block repeat its last row / column
    const bool own_cell = ti < SQ_OWN && tj < SQ_OWN && i0 + ti + 1 < ni && j0 + tj + 1 < nj;
    // the threads that hold the i-, j- and ij-neighbour; the tile's last row / column (which own no cell) point at themselves
    const int t_i = ti < SQ_OWN ? t + SQ_TILE : t, t_j = tj < SQ_OWN ? t + 1 : t, t_ij = (ti < SQ_OWN ? SQ_TILE : 0) + (tj < SQ_OWN ? 1 : 0) + t;

    double2 v[K];
    {
        const size_t o = static_cast<size_t>(i) * nj + j;
#pragma unroll
        for (int c = 0; c < K; ++c) v[c] = cuts.xy[c][o];
    }
    if (MAP == TM_STACK_CYLINDRICAL) {
#pragma unroll
        for (int c = 0; c < K; ++c) v[c].y = v[c].y / cuts.radius[c];
    }
    // K15 (tm_stack.hip): cut after cut the knots pass through LDS, two buffers alternating, one barrier per cut; the node then holds
    // (x_c, theta_c) in v[c] and r_c in rc[c], formed by K11's very expressions
    double rc[REV ? K : 1];
    if (REV) {
#pragma unroll
        for (int c = 0; c < K; ++c) {
            stack_surf_stage(sh_u[c & 1], surf, c, t);
            __syncthreads();
            double xs, rs;
            stack_surf_node(sh_u[c & 1], surf, c, v[c].x, &xs, &rs);
            v[c].x = xs;
            rc[c] = rs;
            v[c].y = v[c].y / cuts.radius[c];
        }
    }

    Q3Acc acc;
    q3_init(acc);
    // the layer below: positions of the nodes (i,j), (i+1,j), (i,j+1), (i+1,j+1); i-edges at j and j+1; j-edges at i and i+1; own k-edge
    Q3Point p00{0, 0, 0}, p10 = p00, p01 = p00, p11 = p00;
    double li0_p = 0.0, li1_p = 0.0, lj0_p = 0.0, lj1_p = 0.0, lk_p = 0.0;
    const unsigned long long cells_per_layer = static_cast<unsigned long long>(ni - 1) * (nj - 1);
    const unsigned long long cell_in_layer = static_cast<unsigned long long>(j) * (ni - 1) + i;

    for (int k = k0; k <= k1; ++k) {
        const double* __restrict__ w = table + static_cast<size_t>(k) * (K + 1);   // wave-uniform
        // K11's expression, operation for operation
        double ax = w[0] * v[0].x, ay = w[0] * v[0].y, ar = REV ? w[0] * rc[0] : 0.0;
#pragma unroll
        for (int c = 1; c < K; ++c) {
            ax = ax + w[c] * v[c].x;
            ay = ay + w[c] * v[c].y;
            if (REV) ar = ar + w[c] * rc[c];
        }
        const double s = REV ? ar : w[K];
        Q3Point c00;
        c00.x = ax;
        if (MAP == TM_STACK_CYLINDRICAL || REV) {
            double sn, cs;
            sincos(ay, &sn, &cs);
            c00.y = s * sn;
            c00.z = s * cs;
        } else {
            c00.y = ay;
            c00.z = s;
        }
        const double lk = k > k0 ? q3_edge(p00, c00) : 0.0;
        double(*b)[SQ_THREADS] = sh[k & 1];
        b[0][t] = c00.x;
        b[1][t] = c00.y;
        b[2][t] = c00.z;
        __syncthreads();
        const Q3Point c10{b[0][t_i], b[1][t_i], b[2][t_i]}, c01{b[0][t_j], b[1][t_j], b[2][t_j]};
        const double li0 = q3_edge(c00, c10), lj0 = q3_edge(c00, c01);
        b[3][t] = li0;
        b[4][t] = lj0;
        b[5][t] = lk;
        __syncthreads();
        const Q3Point c11{b[0][t_ij], b[1][t_ij], b[2][t_ij]};
        const double li1 = b[3][t_j], lj1 = b[4][t_i];
        if (k > k0) {
            // cell (i, j, k-1): corner a + 2b + 4c = node (i+a, j+b, k-1+c)
            const Q3Point x[8] = {p00, p10, p01, p11, c00, c10, c01, c11};
            const double li[4] = {li0_p, li1_p, li0, li1};
            const double lj[4] = {lj0_p, lj1_p, lj0, lj1};
            const double lkk[4] = {lk, b[5][t_i], b[5][t_j], b[5][t_ij]};
            const Q3Cell cell = q3_cell(x, li, lj, lkk);
            if (own_cell) {
                const unsigned long long id = static_cast<unsigned long long>(k - 1) * cells_per_layer + cell_in_layer;
                if (partials) {
                    const int bin = q3_count_cell(cell, id, acc);
                    if (bin >= 0) atomicAdd(&sh_hist[bin], 1u);
                }
                if (field) field[id - static_cast<unsigned long long>(k0) * cells_per_layer] = q3_field_value(cell, orientation);
            }
            if (k > k0 + 1) q_growth(lk_p, lk, acc.gk);   // every lane holds a node of the block (clamped lanes repeat a real one)
        }
        p00 = c00;
        p10 = c10;
        p01 = c01;
        p11 = c11;
        li0_p = li0;
        li1_p = li1;
        lj0_p = lj0;
        lj1_p = lj1;
        lk_p = lk;
    }
    if (!partials) return;

    // in-wave, fixed tree
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        acc.deg += sq_shfl(acc.deg, off);
        acc.jle0 += sq_shfl(acc.jle0, off);
        acc.jge0 += sq_shfl(acc.jge0, off);
        q_take_min(acc.smin, acc.imin, __shfl_down(acc.smin, off, 64), sq_shfl(acc.imin, off));
        q_take_max(acc.smax, acc.imax, __shfl_down(acc.smax, off, 64), sq_shfl(acc.imax, off));
        double u;
        u = __shfl_down(acc.aspect, off, 64);
        if (u > acc.aspect) acc.aspect = u;
        u = __shfl_down(acc.gk, off, 64);
        if (u > acc.gk) acc.gk = u;
        u = __shfl_down(acc.vmin, off, 64);
        if (u < acc.vmin) acc.vmin = u;
        u = __shfl_down(acc.vmax, off, 64);
        if (u > acc.vmax) acc.vmax = u;
        acc.vsum += __shfl_down(acc.vsum, off, 64);
        acc.vabs += __shfl_down(acc.vabs, off, 64);
    }
    if (lane == 0) sh_acc[wave] = acc;   // hist is zero in every lane: the bins are in sh_hist
    __syncthreads();
    if (t == 0) {
        Q3Acc r = sh_acc[0];
        for (int wv = 1; wv < SQ_WAVES; ++wv) q3_combine(r, sh_acc[wv]);
        for (int h = 0; h < 20; ++h) r.hist[h / 10][h % 10] = sh_hist[h];
        partials[static_cast<size_t>(blockIdx.y) * gridDim.x + blockIdx.x] = r;
    }
}

// one wave combines the records in the fixed order of records_reduce_wave, so the sums are the same on every run
__global__ __launch_bounds__(64) void k_stack_quality_finalize(const Q3Acc* __restrict__ partials, long long nrec, uint64_t block, uint64_t ni, uint64_t nj,
                                                               uint64_t nk, tm_quality3d* __restrict__ out) {
    __shared__ Q3Acc sh[64];
    records_reduce_wave<Q3Acc, q3_init, q3_combine>(partials, 0ll, nrec, sh);
    if (threadIdx.x == 0) q3_finish(sh[0], block, ni, nj, nk, out);
}

static dim3 stack_quality_grid(int ni, int nj) { return dim3((nj - 1 + SQ_OWN - 1) / SQ_OWN, (ni - 1 + SQ_OWN - 1) / SQ_OWN); }

template <int K>
static void stack_quality_launch_k(const StackCuts& cuts, const StackSurf& surf, int mapping, const double* table, int k0, int k1, int ni, int nj, Q3Acc* partials,
                                   double* field, int orientation, hipStream_t st) {
    const dim3 grid = stack_quality_grid(ni, nj), block(SQ_THREADS);
    if (mapping == TM_STACK_REVOLUTION)
        hipLaunchKernelGGL((k_stack_quality<K, TM_STACK_REVOLUTION>), grid, block, 0, st, cuts, surf, table, k0, k1, ni, nj, partials, field, orientation);
    else if (mapping == TM_STACK_CYLINDRICAL)
        hipLaunchKernelGGL((k_stack_quality<K, TM_STACK_CYLINDRICAL>), grid, block, 0, st, cuts, surf, table, k0, k1, ni, nj, partials, field, orientation);
    else
        hipLaunchKernelGGL((k_stack_quality<K, TM_STACK_PLANAR>), grid, block, 0, st, cuts, surf, table, k0, k1, ni, nj, partials, field, orientation);
}

static hipError_t launch_stack_quality(int K, const StackCuts& cuts, const StackSurf& surf, int mapping, const double* table, int k0, int k1, int ni, int nj, Q3Acc* partials,
                                       double* field, int orientation, hipStream_t st) {
    if (K < 2 || K > TM_STACK_MAX_CUTS) return hipErrorInvalidValue;
    dispatch_int<2, TM_STACK_MAX_CUTS>(K, [&](auto k) { stack_quality_launch_k<k()>(cuts, surf, mapping, table, k0, k1, ni, nj, partials, field, orientation, st); });
    return hipGetLastError();
}

static void stack_quality_check_sizes(const StackPlan& p, uint64_t ni, uint64_t nj) {
    stack_check_cells(p, ni, nj);
    if (p.nlayers >= (uint64_t{1} << 31) || ni * nj >= (uint64_t{1} << 31)) throw TmError(TM_E_SIZE, "block size or layer count out of range");
}

// The report of the whole stack: table up, K12 and its finalize on `st`, the record back; returns when it has arrived.
// `sf` (TM_STACK_REVOLUTION): the meridional tables go up on `st` like the weight table.
static void stack_quality_run(const StackPlan& p, StackCuts& cuts, uint64_t block, uint64_t ni, uint64_t nj, tm_quality3d* out, hipStream_t st,
                              const SurfPlan* sf = nullptr) {
    const int K = p.ncuts;
    stack_fill_radii(p, cuts);
    StackSurfDev sd;
    if (sf) stack_surf_upload(p, *sf, cuts, sd, st);
    const dim3 grid = stack_quality_grid(static_cast<int>(ni), static_cast<int>(nj));
    const size_t nrec = static_cast<size_t>(grid.x) * grid.y;   // the records buffer is sized from the very grid that writes it
    const std::vector<double> table = stack_weight_table(p, 0, p.nlayers);
    DevBuf d_table, d_rec(sizeof(Q3Acc) * nrec, "stack quality records"), d_out(sizeof(tm_quality3d), "stack quality result");
    d_table.upload(table.data(), table.size(), st, "stack weights");
    HIPCHK(launch_stack_quality(K, cuts, sd.surf, p.mapping, d_table.as<double>(), 0, static_cast<int>(p.nlayers) - 1, static_cast<int>(ni), static_cast<int>(nj), d_rec.as<Q3Acc>(),
                                nullptr, 0, st));
    hipLaunchKernelGGL(k_stack_quality_finalize, dim3(1), dim3(64), 0, st, d_rec.as<Q3Acc>(), static_cast<long long>(nrec), block, ni, nj, p.nlayers, d_out.as<tm_quality3d>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_out.p, sizeof(tm_quality3d), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));   // `table` and the device buffers live until here
}

// per-cell min of o*s of the cell layers [k_begin, k_begin + k_count)
static void stack_quality_field_run(const StackPlan& p, StackCuts& cuts, uint64_t ni, uint64_t nj, uint64_t k_begin, uint64_t k_count, int orientation,
                                    double* host_field, hipStream_t st, const SurfPlan* sf = nullptr) {
    const int K = p.ncuts;
    stack_fill_radii(p, cuts);
    StackSurfDev sd;
    if (sf) stack_surf_upload(p, *sf, cuts, sd, st);
    const size_t cells = static_cast<size_t>(k_count) * (ni - 1) * (nj - 1);
    const std::vector<double> table = stack_weight_table(p, 0, p.nlayers);
    DevBuf d_table, d_field(sizeof(double) * cells, "stack quality cells");
    d_table.upload(table.data(), table.size(), st, "stack weights");
    HIPCHK(launch_stack_quality(K, cuts, sd.surf, p.mapping, d_table.as<double>(), static_cast<int>(k_begin), static_cast<int>(k_begin + k_count), static_cast<int>(ni),
                                static_cast<int>(nj), nullptr, d_field.as<double>(), orientation, st));
    HIPCHK(hipMemcpyAsync(host_field, d_field.p, sizeof(double) * cells, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
}

}  // namespace tmh

using namespace tmh;

// sf: the filled meridional plan of the _surf entry points, null for the plain ones (`p` then comes from stack_plan)
static void stack_quality_host_cuts(const tm_mesh_desc* const* cuts, const StackPlan& p, const SurfPlan* sf, uint64_t block, tm_quality3d* out) {
    uint64_t ni = 0, nj = 0;
    stack_check_cuts(cuts, p.ncuts, block, &ni, &nj);
    stack_quality_check_sizes(p, ni, nj);
    DevBuf in;
    StackCuts dc{};
    stack_upload_cuts(cuts, p.ncuts, block, ni, nj, in, dc);
    stack_quality_run(p, dc, block, ni, nj, out, nullptr, sf);
}
// want_field false: the report into *out; true: the orientation from the report, then the cell layers [k_begin, k_begin + k_count) into field
static void stack_quality_smoothers(tm_smoother* const* cuts, const StackPlan& p, const SurfPlan* sf, uint64_t block, tm_quality3d* out, bool want_field,
                                    uint64_t k_begin, uint64_t k_count, double* field) {
    StackCuts dc{};
    uint64_t ni = 0, nj = 0;
    stack_resident_cuts(cuts, p, block, dc, &ni, &nj);
    stack_quality_check_sizes(p, ni, nj);
    if (want_field && (k_count < 1 || k_begin >= p.nlayers - 1 || k_count > p.nlayers - 1 - k_begin))
        throw TmError(TM_E_ARG, "the window of cell layers is empty or reaches past nlayers - 1");
    std::vector<std::unique_ptr<StackEvent>> events;
    const hipStream_t st = stack_order_behind(cuts, p.ncuts, events);
    tm_quality3d q;
    stack_quality_run(p, dc, block, ni, nj, want_field ? &q : out, st, sf);   // synchronises st: the other handles' coordinates have been read when it returns
    if (want_field) stack_quality_field_run(p, dc, ni, nj, k_begin, k_count, q.orientation, field, st, sf);
}

extern "C" int tm_stack_quality(const tm_mesh_desc* const* cuts, const tm_stack_opt* opt, uint64_t block, tm_quality3d* out) {
    return guarded([&]() {
        if (!out) throw TmError(TM_E_ARG, "null argument");
        stack_quality_host_cuts(cuts, stack_plan(opt), nullptr, block, out);
        return TM_OK;
    });
}

extern "C" int tm_stack_smoothers_quality(tm_smoother* const* cuts, const tm_stack_opt* opt, uint64_t block, tm_quality3d* out) {
    return guarded([&]() {
        if (!cuts || !out) throw TmError(TM_E_ARG, "null argument");
        stack_quality_smoothers(cuts, stack_plan(opt), nullptr, block, out, false, 0, 0, nullptr);
        return TM_OK;
    });
}

extern "C" int tm_stack_smoothers_quality_field(tm_smoother* const* cuts, const tm_stack_opt* opt, uint64_t block, uint64_t k_begin, uint64_t k_count,
                                                double* min_scaled_jacobian) {
    return guarded([&]() {
        if (!cuts || !min_scaled_jacobian) throw TmError(TM_E_ARG, "null argument");
        stack_quality_smoothers(cuts, stack_plan(opt), nullptr, block, nullptr, true, k_begin, k_count, min_scaled_jacobian);
        return TM_OK;
    });
}

extern "C" int tm_stack_quality_surf(const tm_mesh_desc* const* cuts, const tm_stack_opt* opt, const tm_stack_surfaces* surfaces, uint64_t block,
                                     tm_quality3d* out) {
    return guarded([&]() {
        if (!out) throw TmError(TM_E_ARG, "null argument");
        SurfPlan sf;
        const StackPlan p = stack_plan_surf(opt, surfaces, sf);
        stack_quality_host_cuts(cuts, p, &sf, block, out);
        return TM_OK;
    });
}

extern "C" int tm_stack_smoothers_quality_surf(tm_smoother* const* cuts, const tm_stack_opt* opt, const tm_stack_surfaces* surfaces, uint64_t block,
                                               tm_quality3d* out) {
    return guarded([&]() {
        if (!cuts || !out) throw TmError(TM_E_ARG, "null argument");
        SurfPlan sf;
        const StackPlan p = stack_plan_surf(opt, surfaces, sf);
        stack_quality_smoothers(cuts, p, &sf, block, out, false, 0, 0, nullptr);
        return TM_OK;
    });
}

extern "C" int tm_stack_smoothers_quality_field_surf(tm_smoother* const* cuts, const tm_stack_opt* opt, const tm_stack_surfaces* surfaces, uint64_t block,
                                                     uint64_t k_begin, uint64_t k_count, double* min_scaled_jacobian) {
    return guarded([&]() {
        if (!cuts || !min_scaled_jacobian) throw TmError(TM_E_ARG, "null argument");
        SurfPlan sf;
        const StackPlan p = stack_plan_surf(opt, surfaces, sf);
        stack_quality_smoothers(cuts, p, &sf, block, nullptr, true, k_begin, k_count, min_scaled_jacobian);
        return TM_OK;
    });
}
