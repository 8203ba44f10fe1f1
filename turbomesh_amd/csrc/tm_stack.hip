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

#include <algorithm>
#include <cstring>

namespace tmh {

constexpr int STACK_TILE = 32, STACK_THREADS = STACK_TILE * STACK_TILE;

// table: per layer of the window K weights followed by s[k] (row pitch K + 1)
template <int K, int MAP>
__global__ __launch_bounds__(STACK_THREADS) void k_stack_planes(StackCuts cuts, const double* __restrict__ table, int nk, int ni, int nj, double* __restrict__ X,
                                                                double* __restrict__ Y, double* __restrict__ Z) {
    __shared__ double2 tile[2][STACK_TILE][STACK_TILE + 1];   // +1: the transposed read walks a column
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int i0 = blockIdx.y * STACK_TILE, j0 = blockIdx.x * STACK_TILE;
    double2 v[K];
    {
        const int i = i0 + ty, j = j0 + tx;
        const bool in = i < ni && j < nj;
        const size_t o = in ? static_cast<size_t>(i) * nj + j : 0;   // lanes past the block read node (0,0); their values are never stored
#pragma unroll
        for (int c = 0; c < K; ++c) v[c] = cuts.xy[c][o];
    }
#pragma unroll
    for (int c = 0; c < K; ++c) {
        tile[c & 1][ty][tx] = v[c];
        __syncthreads();   // tile[c & 1] is written again two cuts later: every thread has passed the next barrier, i.e. read it, by then
        v[c] = tile[c & 1][tx][ty];
    }
    const int i = i0 + tx, j = j0 + ty;
    if (i >= ni || j >= nj) return;   // no barrier below
    if (MAP == TM_STACK_CYLINDRICAL) {
#pragma unroll
        for (int c = 0; c < K; ++c) v[c].y = v[c].y / cuts.radius[c];
    }
    const size_t plane = static_cast<size_t>(ni) * nj;
    size_t o = static_cast<size_t>(j) * ni + i;
    for (int k = 0; k < nk; ++k, o += plane) {
        const double* __restrict__ w = table + static_cast<size_t>(k) * (K + 1);   // wave-uniform
        double ax = w[0] * v[0].x, ay = w[0] * v[0].y;
#pragma unroll
        for (int c = 1; c < K; ++c) {
            ax = ax + w[c] * v[c].x;
            ay = ay + w[c] * v[c].y;
        }
        const double s = w[K];
        X[o] = ax;
        if (MAP == TM_STACK_CYLINDRICAL) {
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
static void stack_launch_k(const StackCuts& cuts, int mapping, const double* table, int nk, int ni, int nj, double* X, double* Y, double* Z, hipStream_t st) {
    const dim3 grid((nj + STACK_TILE - 1) / STACK_TILE, (ni + STACK_TILE - 1) / STACK_TILE), block(STACK_THREADS);
    if (mapping == TM_STACK_CYLINDRICAL)
        hipLaunchKernelGGL((k_stack_planes<K, TM_STACK_CYLINDRICAL>), grid, block, 0, st, cuts, table, nk, ni, nj, X, Y, Z);
    else
        hipLaunchKernelGGL((k_stack_planes<K, TM_STACK_PLANAR>), grid, block, 0, st, cuts, table, nk, ni, nj, X, Y, Z);
}

static hipError_t launch_stack_planes(int K, const StackCuts& cuts, int mapping, const double* table, int nk, int ni, int nj, double* X, double* Y, double* Z,
                                      hipStream_t st) {
    switch (K) {
#define TM_STACK_CASE(n) \
    case n: stack_launch_k<n>(cuts, mapping, table, nk, ni, nj, X, Y, Z, st); break;
        TM_STACK_CASE(2) TM_STACK_CASE(3) TM_STACK_CASE(4) TM_STACK_CASE(5) TM_STACK_CASE(6) TM_STACK_CASE(7) TM_STACK_CASE(8) TM_STACK_CASE(9)
        TM_STACK_CASE(10) TM_STACK_CASE(11) TM_STACK_CASE(12) TM_STACK_CASE(13) TM_STACK_CASE(14) TM_STACK_CASE(15) TM_STACK_CASE(16)
#undef TM_STACK_CASE
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// The window's table to the device, the kernel on `st`, the three planes back to the host; returns when they have arrived.
static void stack_run(const StackPlan& p, StackCuts& cuts, uint64_t k_begin, uint64_t k_count, uint64_t ni, uint64_t nj, double* x, double* y, double* z,
                      hipStream_t st) {
    const int K = p.ncuts;
    if (k_count >= (uint64_t{1} << 31)) throw TmError(TM_E_SIZE, "layer window out of range");
    stack_fill_radii(p, cuts);
    std::vector<double> table(static_cast<size_t>(k_count) * (K + 1));
    for (uint64_t k = 0; k < k_count; ++k) {
        std::memcpy(&table[k * (K + 1)], &p.weights[(k_begin + k) * K], sizeof(double) * K);
        table[k * (K + 1) + K] = p.layers[k_begin + k];
    }
    const size_t n = static_cast<size_t>(ni) * nj * k_count;
    StackBuf d_table(sizeof(double) * table.size(), "stack weights"), d_out(sizeof(double) * 3 * n, "stack planes");
    HIPCHK(hipMemcpyAsync(d_table.p, table.data(), sizeof(double) * table.size(), hipMemcpyHostToDevice, st));
    double* out = d_out.as<double>();
    HIPCHK(launch_stack_planes(K, cuts, p.mapping, d_table.as<double>(), static_cast<int>(k_count), static_cast<int>(ni), static_cast<int>(nj), out, out + n, out + 2 * n, st));
    HIPCHK(hipMemcpyAsync(x, out, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(y, out + n, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(z, out + 2 * n, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));   // `table` and the device buffers live until here
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

extern "C" int tm_stack_block(const tm_mesh_desc* const* cuts, const tm_stack_opt* opt, uint64_t block, uint64_t k_begin, uint64_t k_count, double* x,
                              double* y, double* z) {
    return guarded([&]() {
        if (!x || !y || !z) throw TmError(TM_E_ARG, "null argument");
        const StackPlan p = stack_plan(opt);
        stack_check_window(p, k_begin, k_count);
        uint64_t ni = 0, nj = 0;
        stack_check_cuts(cuts, p.ncuts, block, &ni, &nj);
        require_gfx950_stack();
        const size_t n = static_cast<size_t>(ni) * nj;
        StackBuf in(sizeof(double2) * n * p.ncuts, "stack cuts");
        StackCuts dc{};
        for (int c = 0; c < p.ncuts; ++c) {
            dc.xy[c] = in.as<double2>() + n * c;
            HIPCHK(hipMemcpy(in.as<double2>() + n * c, cuts[c]->blocks[block].xy, sizeof(double2) * n, hipMemcpyHostToDevice));
        }
        stack_run(p, dc, k_begin, k_count, ni, nj, x, y, z, nullptr);
        return TM_OK;
    });
}

extern "C" int tm_stack_smoothers(tm_smoother* const* cuts, const tm_stack_opt* opt, uint64_t block, uint64_t k_begin, uint64_t k_count, double* x,
                                  double* y, double* z) {
    return guarded([&]() {
        if (!cuts || !x || !y || !z) throw TmError(TM_E_ARG, "null argument");
        const StackPlan p = stack_plan(opt);
        stack_check_window(p, k_begin, k_count);
        StackCuts dc{};
        uint64_t ni = 0, nj = 0;
        stack_resident_cuts(cuts, p, block, dc, &ni, &nj);
        std::vector<std::unique_ptr<StackEvent>> events;
        const hipStream_t st = stack_order_behind(cuts, p.ncuts, events);
        stack_run(p, dc, k_begin, k_count, ni, nj, x, y, z, st);   // synchronises st: the other handles' coordinates have been read when it returns
        return TM_OK;
    });
}
