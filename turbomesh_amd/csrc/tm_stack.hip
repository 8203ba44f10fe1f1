// K11  stack_planes: K smoothed 2-D cuts of one block -> the layers of a 3-D block (include/tm_hip.h, "3-D from 2-D cuts").  gfx950, wave64.
//      layer k, node (i,j):  v = sum_c A[k][c] v_c(i,j), c = 0 .. K-1 in that order, nothing fused; planes X, Y, Z with i fastest.
//
// Layout.  32 x 32 tiles like K8, one node per thread (1024 threads).  Loads: every thread first issues its K loads -- node
// (i0 + ty, j0 + tx) of every cut, coalesced along j, 16 B per lane, all K in flight together -- then the cuts pass one after the other
// through a padded LDS tile (double2 [32][33], two of them alternating so that one barrier per cut is enough) and come back transposed
// into the SAME registers: the thread ends up holding the K values of node (i0 + tx, j0 + ty).  K is a template parameter, the loops
// over it are unrolled, so the K values live in registers under compile-time indices.  Stores: a loop over the window's layers; the
// weight row of a layer (and s[k]) is read from a small table under a wave-uniform index -- scalar loads, not per lane -- and X, Y, Z
// are stored coalesced along i.  The cylindrical mapping divides once per cut (theta_c = y_c / z[c], before the layer loop) and takes one
// sincos per output.
//
// Traffic per node: 16 K bytes read, 24 k_count bytes written, each byte once: plain coalesced loads and stores, the three output
// streams dominate.  Compiler's resource usage (cross-compile, -Rpass-analysis=kernel-resource-usage): see DESIGN.md section 4, K11.
#include "tm_stack_dev.hpp"
#include "tm_dispatch.hpp"

#include <algorithm>
#include <cstring>

namespace tmh {

constexpr int STACK_TILE = 32, STACK_THREADS = STACK_TILE * STACK_TILE;

// table: per layer of the window K weights followed by s[k] (row pitch K + 1)
//
// K15 (MAP == TM_STACK_REVOLUTION; include/tm_hip.h, "cuts on stream surfaces of revolution").  As cut c passes through the tile, the
// first N_c threads also stage its knots in LDS (two buffers alternating like the tiles: the same one barrier per cut covers both); right
// behind the transposed read every thread locates its node's u among them (surf_locate: fixed steps, no branch on the data), gathers the
// interval's 64 B of coefficients from the table (16 KB per cut at the most: L2) and evaluates x_c and r_c by Horner (tm_stack_surface.hpp,
// shared with the host); theta_c = v / rref_c.  The thread then holds three values per cut, (x_c, theta_c) in v[c] and r_c in rc[c], and
// the layer loop sums three rows.  Nodes outside a table: ballot and popcount per wave and cut, LDS counters, one global integer atomic
// per workgroup and cut.  Lanes past the block run along (they hold node (0,0)) and are masked out of the counts and the stores.
template <int K, int MAP>
__global__ __launch_bounds__(STACK_THREADS) void k_stack_planes(StackCuts cuts, StackSurf surf, const double* __restrict__ table, int nk, int ni, int nj,
                                                                double* __restrict__ X, double* __restrict__ Y, double* __restrict__ Z,
                                                                unsigned long long* __restrict__ outside) {
    constexpr bool REV = MAP == TM_STACK_REVOLUTION;
    __shared__ double2 tile[2][STACK_TILE][STACK_TILE + 1];   // +1: the transposed read walks a column
    __shared__ double sh_u[REV ? 2 : 1][REV ? TM_STACK_MAX_KNOTS : 1];
    __shared__ unsigned sh_out[REV ? K : 1];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int i0 = blockIdx.y * STACK_TILE, j0 = blockIdx.x * STACK_TILE;
    double2 v[K];
    double rc[REV ? K : 1];
    {
        const int i = i0 + ty, j = j0 + tx;
        const bool in = i < ni && j < nj;
        const size_t o = in ? static_cast<size_t>(i) * nj + j : 0;   // lanes past the block read node (0,0); their values are never stored
#pragma unroll
        for (int c = 0; c < K; ++c) v[c] = cuts.xy[c][o];
    }
    const int i = i0 + tx, j = j0 + ty;
    const bool valid = i < ni && j < nj;
    if (REV && static_cast<int>(threadIdx.x) < K) sh_out[threadIdx.x] = 0;   // ordered before the first atomic by the first cut's barrier
#pragma unroll
    for (int c = 0; c < K; ++c) {
        tile[c & 1][ty][tx] = v[c];
        if (REV) stack_surf_stage(sh_u[c & 1], surf, c, static_cast<int>(threadIdx.x));
        __syncthreads();   // tile[c & 1] is written again two cuts later: every thread has passed the next barrier, i.e. read it, by then
        v[c] = tile[c & 1][tx][ty];
        if (REV) {
            double xs, rs;
            const bool out = stack_surf_node(sh_u[c & 1], surf, c, v[c].x, &xs, &rs);
            v[c].x = xs;
            rc[c] = rs;
            v[c].y = v[c].y / cuts.radius[c];
            if (outside) {
                const unsigned long long m = __ballot(out && valid);
                if ((threadIdx.x & 63) == 0 && m) atomicAdd(&sh_out[c], static_cast<unsigned>(__popcll(m)));
            }
        }
    }
    if (REV && outside) {
        __syncthreads();
        if (static_cast<int>(threadIdx.x) < K && sh_out[threadIdx.x]) atomicAdd(&outside[threadIdx.x], static_cast<unsigned long long>(sh_out[threadIdx.x]));
    }
    if (!valid) return;   // no barrier below
    if (MAP == TM_STACK_CYLINDRICAL) {
#pragma unroll
        for (int c = 0; c < K; ++c) v[c].y = v[c].y / cuts.radius[c];
    }
    const size_t plane = static_cast<size_t>(ni) * nj;
    size_t o = static_cast<size_t>(j) * ni + i;
    for (int k = 0; k < nk; ++k, o += plane) {
        const double* __restrict__ w = table + static_cast<size_t>(k) * (K + 1);   // wave-uniform
        double ax = w[0] * v[0].x, ay = w[0] * v[0].y, ar = REV ? w[0] * rc[0] : 0.0;
#pragma unroll
        for (int c = 1; c < K; ++c) {
            ax = ax + w[c] * v[c].x;
            ay = ay + w[c] * v[c].y;
            if (REV) ar = ar + w[c] * rc[c];
        }
        const double s = REV ? ar : w[K];
        X[o] = ax;
        if (MAP == TM_STACK_CYLINDRICAL || REV) {
            double sn, cs;
            sincos(ay, &sn, &cs);
            Y[o] = s * sn;
            Z[o] = s * cs;
        } else {
            Y[o] = ay;
            Z[o] = s;
        }
    }
}

template <int K>
static void stack_launch_k(const StackCuts& cuts, const StackSurf& surf, int mapping, const double* table, int nk, int ni, int nj, double* X, double* Y, double* Z,
                           unsigned long long* outside, hipStream_t st) {
    const dim3 grid((nj + STACK_TILE - 1) / STACK_TILE, (ni + STACK_TILE - 1) / STACK_TILE), block(STACK_THREADS);
    if (mapping == TM_STACK_REVOLUTION)
        hipLaunchKernelGGL((k_stack_planes<K, TM_STACK_REVOLUTION>), grid, block, 0, st, cuts, surf, table, nk, ni, nj, X, Y, Z, outside);
    else if (mapping == TM_STACK_CYLINDRICAL)
        hipLaunchKernelGGL((k_stack_planes<K, TM_STACK_CYLINDRICAL>), grid, block, 0, st, cuts, surf, table, nk, ni, nj, X, Y, Z, outside);
    else
        hipLaunchKernelGGL((k_stack_planes<K, TM_STACK_PLANAR>), grid, block, 0, st, cuts, surf, table, nk, ni, nj, X, Y, Z, outside);
}

hipError_t launch_stack_planes(int K, const StackCuts& cuts, const StackSurf& surf, int mapping, const double* table, int nk, int ni, int nj, double* X, double* Y,
                               double* Z, unsigned long long* outside, hipStream_t st) {
    if (K < 2 || K > TM_STACK_MAX_CUTS) return hipErrorInvalidValue;
    dispatch_int<2, TM_STACK_MAX_CUTS>(K, [&](auto k) { stack_launch_k<k()>(cuts, surf, mapping, table, nk, ni, nj, X, Y, Z, outside, st); });
    return hipGetLastError();
}

// The window's table to the device, the kernel on `st`, the three planes back to the host; returns when they have arrived.
// `sf` (TM_STACK_REVOLUTION): the meridional tables go up on `st` like the weight table; outside[c], when asked for, comes back with the planes.
static void stack_run(const StackPlan& p, StackCuts& cuts, uint64_t k_begin, uint64_t k_count, uint64_t ni, uint64_t nj, double* x, double* y, double* z,
                      hipStream_t st, const SurfPlan* sf = nullptr, uint64_t* outside = nullptr) {
    const int K = p.ncuts;
    if (k_count >= (uint64_t{1} << 31)) throw TmError(TM_E_SIZE, "layer window out of range");
    stack_fill_radii(p, cuts);
    StackSurfDev sd;
    DevBuf d_outside;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the counters are copied out as they are");
    if (sf) stack_surf_upload(p, *sf, cuts, sd, st);
    if (sf && outside) {
        d_outside.grow(sizeof(unsigned long long) * TM_STACK_MAX_CUTS, "stack outside counts");
        HIPCHK(hipMemsetAsync(d_outside.p, 0, sizeof(unsigned long long) * TM_STACK_MAX_CUTS, st));
    }
    const std::vector<double> table = stack_weight_table(p, k_begin, k_count);
    const size_t n = static_cast<size_t>(ni) * nj * k_count;
    DevBuf d_table, d_out(sizeof(double) * 3 * n, "stack planes");
    d_table.upload(table.data(), table.size(), st, "stack weights");
    double* out = d_out.as<double>();
    HIPCHK(launch_stack_planes(K, cuts, sd.surf, p.mapping, d_table.as<double>(), static_cast<int>(k_count), static_cast<int>(ni), static_cast<int>(nj), out, out + n,
                               out + 2 * n, d_outside.as<unsigned long long>(), st));
    if (d_outside.p) HIPCHK(hipMemcpyAsync(outside, d_outside.p, sizeof(uint64_t) * K, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(x, out, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(y, out + n, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(z, out + 2 * n, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));   // `table` and the device buffers live until here
}

void stack_surf_upload(const StackPlan& p, const SurfPlan& sf, StackCuts& cuts, StackSurfDev& d, hipStream_t st) {
    const size_t nknots = (sf.knots.size() + 3) / 4 * 4;   // the coefficients start on a 32 B boundary: they are read as double4
    d.host.assign(nknots + sf.coef.size(), 0.0);
    std::copy(sf.knots.begin(), sf.knots.end(), d.host.begin());
    std::copy(sf.coef.begin(), sf.coef.end(), d.host.begin() + nknots);
    d.surf.knots = d.dev.upload(d.host.data(), d.host.size(), st, "stack meridional tables");
    d.surf.coef = d.surf.knots + nknots;
    for (int c = 0; c < TM_STACK_MAX_CUTS; ++c) {
        d.surf.first[c] = c < p.ncuts ? sf.first[c] : 0;
        d.surf.nknots[c] = c < p.ncuts ? sf.nknots[c] : 2;
        if (c < p.ncuts) cuts.radius[c] = sf.rref[c];
    }
}

StackPlan stack_plan_any(const tm_stack_opt* opt, const tm_stack_surfaces* surfaces, SurfPlan& sf, const SurfPlan** used) {
    if (!opt) throw TmError(TM_E_ARG, "null stack options, span or layers");
    const bool rev = opt->mapping == TM_STACK_REVOLUTION;
    if (!rev && surfaces) throw TmError(TM_E_ARG, "meridional tables go with TM_STACK_REVOLUTION only");
    *used = rev ? &sf : nullptr;
    return rev ? stack_plan_surf(opt, surfaces, sf) : stack_plan(opt);
}

void stack_upload_cuts(const tm_mesh_desc* const* cuts, int ncuts, uint64_t block, uint64_t ni, uint64_t nj, DevBuf& in, StackCuts& dc) {
    require_gfx950();
    const size_t n = static_cast<size_t>(ni) * nj;
    in.grow(sizeof(double2) * n * ncuts, "stack cuts");
    for (int c = 0; c < ncuts; ++c) {
        dc.xy[c] = in.as<double2>() + n * c;
        HIPCHK(hipMemcpy(in.as<double2>() + n * c, cuts[c]->blocks[block].xy, sizeof(double2) * n, hipMemcpyHostToDevice));
    }
}

std::vector<double> stack_weight_table(const StackPlan& p, uint64_t k_begin, uint64_t k_count, size_t extra) {
    const int K = p.ncuts;
    std::vector<double> table(static_cast<size_t>(k_count) * (K + 1) + extra);
    for (uint64_t k = 0; k < k_count; ++k) {
        std::memcpy(&table[k * (K + 1)], &p.weights[(k_begin + k) * K], sizeof(double) * K);
        table[k * (K + 1) + K] = p.layers[k_begin + k];
    }
    return table;
}

void stack_resident_cuts(tm_smoother* const* cuts, const StackPlan& p, uint64_t block, StackCuts& dc, uint64_t* ni, uint64_t* nj) {
    for (int c = 0; c < p.ncuts; ++c)
        if (!cuts[c] || !smoother_is_live(cuts[c])) throw TmError(TM_E_ARG, "a cut is not a live handle");
    const Smoother& s0 = cuts[0]->impl;
    for (int c = 1; c < p.ncuts; ++c)
        if (cuts[c]->impl.topo.nblocks() != s0.topo.nblocks()) throw TmError(TM_E_SIZE, "InconsistentSize: the handles differ in block count");
    if (block >= static_cast<uint64_t>(s0.topo.nblocks())) throw TmError(TM_E_ARG, "block index past the mesh");
    const int64_t b = static_cast<int64_t>(block);
    for (int c = 0; c < p.ncuts; ++c) {
        const Smoother& s = cuts[c]->impl;
        if (s.topo.ni[b] != s0.topo.ni[b] || s.topo.nj[b] != s0.topo.nj[b]) throw TmError(TM_E_SIZE, "InconsistentSize: the handles differ in the size of the block");
        const auto it = std::lower_bound(s.lp.owned_blocks.begin(), s.lp.owned_blocks.end(), b);
        if (it == s.lp.owned_blocks.end() || *it != b) throw TmError(TM_E_ARG, "block is not owned by every handle");
        dc.xy[c] = s.X + s.lp.local_start[it - s.lp.owned_blocks.begin()];
    }
    *ni = static_cast<uint64_t>(s0.topo.ni[b]);
    *nj = static_cast<uint64_t>(s0.topo.nj[b]);
}

hipStream_t stack_order_behind(tm_smoother* const* cuts, int ncuts, std::vector<std::unique_ptr<StackEvent>>& events) {
    const hipStream_t st = cuts[0]->impl.stream;
    for (int c = 1; c < ncuts; ++c) {
        if (cuts[c]->impl.stream == st) continue;
        events.push_back(std::make_unique<StackEvent>());
        HIPCHK(hipEventRecord(events.back()->e, cuts[c]->impl.stream));
        HIPCHK(hipStreamWaitEvent(st, events.back()->e, 0));
    }
    return st;
}

}  // namespace tmh

using namespace tmh;

// sf: the filled meridional plan of the _surf entry points, null for the plain ones (`p` then comes from stack_plan)
static void stack_block(const tm_mesh_desc* const* cuts, const StackPlan& p, const SurfPlan* sf, uint64_t block, uint64_t k_begin, uint64_t k_count, double* x, double* y,
                        double* z, uint64_t* outside) {
    stack_check_window(p, k_begin, k_count);
    uint64_t ni = 0, nj = 0;
    stack_check_cuts(cuts, p.ncuts, block, &ni, &nj);
    DevBuf in;
    StackCuts dc{};
    stack_upload_cuts(cuts, p.ncuts, block, ni, nj, in, dc);
    stack_run(p, dc, k_begin, k_count, ni, nj, x, y, z, nullptr, sf, outside);
}
static void stack_smoothers(tm_smoother* const* cuts, const StackPlan& p, const SurfPlan* sf, uint64_t block, uint64_t k_begin, uint64_t k_count, double* x, double* y,
                            double* z, uint64_t* outside) {
    stack_check_window(p, k_begin, k_count);
    StackCuts dc{};
    uint64_t ni = 0, nj = 0;
    stack_resident_cuts(cuts, p, block, dc, &ni, &nj);
    std::vector<std::unique_ptr<StackEvent>> events;
    const hipStream_t st = stack_order_behind(cuts, p.ncuts, events);
    stack_run(p, dc, k_begin, k_count, ni, nj, x, y, z, st, sf, outside);   // synchronises st: the other handles' coordinates have been read when it returns
}

extern "C" int tm_stack_block(const tm_mesh_desc* const* cuts, const tm_stack_opt* opt, uint64_t block, uint64_t k_begin, uint64_t k_count, double* x,
                              double* y, double* z) {
    return guarded([&]() {
        if (!x || !y || !z) throw TmError(TM_E_ARG, "null argument");
        stack_block(cuts, stack_plan(opt), nullptr, block, k_begin, k_count, x, y, z, nullptr);
        return TM_OK;
    });
}

extern "C" int tm_stack_smoothers(tm_smoother* const* cuts, const tm_stack_opt* opt, uint64_t block, uint64_t k_begin, uint64_t k_count, double* x,
                                  double* y, double* z) {
    return guarded([&]() {
        if (!cuts || !x || !y || !z) throw TmError(TM_E_ARG, "null argument");
        stack_smoothers(cuts, stack_plan(opt), nullptr, block, k_begin, k_count, x, y, z, nullptr);
        return TM_OK;
    });
}

extern "C" int tm_stack_block_surf(const tm_mesh_desc* const* cuts, const tm_stack_opt* opt, const tm_stack_surfaces* surfaces, uint64_t block, uint64_t k_begin,
                                   uint64_t k_count, double* x, double* y, double* z, uint64_t* outside) {
    return guarded([&]() {
        if (!x || !y || !z) throw TmError(TM_E_ARG, "null argument");
        SurfPlan sf;
        const StackPlan p = stack_plan_surf(opt, surfaces, sf);
        stack_block(cuts, p, &sf, block, k_begin, k_count, x, y, z, outside);
        return TM_OK;
    });
}

extern "C" int tm_stack_smoothers_surf(tm_smoother* const* cuts, const tm_stack_opt* opt, const tm_stack_surfaces* surfaces, uint64_t block, uint64_t k_begin,
                                       uint64_t k_count, double* x, double* y, double* z, uint64_t* outside) {
    return guarded([&]() {
        if (!cuts || !x || !y || !z) throw TmError(TM_E_ARG, "null argument");
        SurfPlan sf;
        const StackPlan p = stack_plan_surf(opt, surfaces, sf);
        stack_smoothers(cuts, p, &sf, block, k_begin, k_count, x, y, z, outside);
        return TM_OK;
    });
}
