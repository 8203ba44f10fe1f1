// K18 welding blocks into one conforming unstructured mesh.  gfx950, wave64.  Definitions: include/tm_hip.h, "welded unstructured mesh";
//     the index arithmetic is tm_weld.hpp, shared with the host definition (tm_weld_host.cpp).  Four stages:
//
// 1. Link.  The union-find lives on the PERIMETER SLOTS of the blocks (2 (ni + nj) - 4 per block, ascending with the flat index), not on
//    the nodes: an interior node is a class of its own and is never touched.  k_weld_init labels every slot with itself, k_weld_hook
//    takes one (connection, t) pair per thread straight from the connection table -- grid.y is the connection -- and hooks the larger of
//    the two roots under the smaller with atomicCAS; a failed CAS means the label of that root has DECREASED, so the thread finds the
//    roots again and its loop ends after finitely many of its own steps: nobody waits for anybody.  Labels only ever decrease, so the
//    root of a class is its smallest slot whatever the order of execution.  k_weld_compress points every slot at its root and counts the
//    class; k_weld_classes bins the classes.  Integer atomics only.
// 2. Number.  The owner flag of a node is computed, not stored: interior nodes own themselves, a perimeter node owns its class iff its
//    slot is a root.  Exclusive prefix sum of the flags over all N nodes in tiles of 2048: k_weld_count (one sum per tile), the sums
//    scanned in tiles of 1024 (k_weld_psum / k_weld_pscan: up to two levels, 2^31 nodes), k_weld_number (flags again, scan inside the
//    tile, ids of the owners into map).  Every launch ends before the next reads it: no look-back, no flag another workgroup spins on.
//    k_weld_slaves then gives the few non-owners the id of their root.
// 3. Points.  k_weld_gather (planes in flat order) / k_weld_gather_resident (the interleaved blocks of a handle, through K8's 32 x 32
//    LDS transpose so that loads run along j and stores along i) copy the owners' coordinates to their ids; k_weld_gap compares the
//    non-owners -- perimeter slots again -- with the welded planes and reduces (gap, index) per workgroup, k_weld_gap_final to one.
// 4. Cells.  A workgroup takes 2048 / npe whole elements and writes their ids with consecutive lanes on consecutive ids (a lane per
//    element would store 4 bytes at a stride of 4 npe); the local order table sits in LDS.
#include "tm_weld_dev.hpp"
#include "tm_stack_dev.hpp"

#include <algorithm>
#include <cstring>

namespace tmh {

constexpr int WELD_THREADS = 256, WELD_WAVES = WELD_THREADS / 64;
constexpr int WELD_PER_THREAD = 8, WELD_TILE = WELD_THREADS * WELD_PER_THREAD;   // nodes per workgroup of the count / number / gather passes
constexpr int WELD_PTILE = 1024;                                                 // tile sums per workgroup of the scan of partials (4 per lane)
constexpr int WELD_MAX_NPE = 125;                                                // (4+1)^3 > (8+1)^2

// a node of the flat index space as (block, i, j), advanced without dividing
struct WeldWalk {
    WeldBlock B;
    int b, i, j;
};
__device__ __forceinline__ void walk_start(const WeldBlock* __restrict__ blocks, int nblocks, int n, WeldWalk& w) {
    w.b = weld_block_of(blocks, nblocks, n);
    w.B = blocks[w.b];
    const int l = n - w.B.off;
    w.j = l / w.B.ni;
    w.i = l - w.j * w.B.ni;
}
__device__ __forceinline__ void walk_next(const WeldBlock* __restrict__ blocks, int nblocks, WeldWalk& w) {
    if (++w.i < w.B.ni) return;
    w.i = 0;
    if (++w.j < w.B.nj) return;
    w.j = 0;
    if (++w.b < nblocks) w.B = blocks[w.b];   // past the last block only behind node N-1, which no caller evaluates
}
__device__ __forceinline__ int weld_owner(const WeldBlock& B, int i, int j, const int32_t* __restrict__ parent) {
    if (!weld_on_perimeter(B.ni, B.nj, i, j)) return 1;
    const int s = B.slot0 + weld_slot(B.ni, B.nj, i, j);
    return parent[s] == s ? 1 : 0;
}
// eight consecutive nodes strictly inside one row of a block: no perimeter node among them
__device__ __forceinline__ bool walk_all_interior(const WeldWalk& w) {
    return w.j > 0 && w.j < w.B.nj - 1 && w.i > 0 && w.i + WELD_PER_THREAD < w.B.ni;
}

__device__ __forceinline__ int weld_block_exscan(int v, int* sh, int& total) {   // sh[WELD_WAVES]; exclusive prefix of v over the workgroup
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < WELD_WAVES; ++w) {
        const int s = sh[w];
        if (w < wave) base += s;
        total += s;
    }
    __syncthreads();
    return base + inc - v;
}

// ------------------------------------------------------------------ 1. link
__global__ __launch_bounds__(WELD_THREADS) void k_weld_init(int32_t* __restrict__ parent, int32_t* __restrict__ count, int nslots) {
    const int s = static_cast<int>(blockIdx.x) * WELD_THREADS + static_cast<int>(threadIdx.x);
    if (s < nslots) {
        parent[s] = s;
        count[s] = 0;
    }
}

__device__ __forceinline__ int weld_find(const int32_t* parent, int x) {
    for (;;) {
        const int p = __atomic_load_n(parent + x, __ATOMIC_RELAXED);   // p <= x always
        if (p == x) return x;
        x = p;
    }
}
__device__ __forceinline__ int weld_slot_of(const WeldBlock* __restrict__ blocks, const tm_range& r, int t) {
    const WeldBlock B = blocks[r.block];
    int i, j;
    weld_side_node(B.ni, B.nj, r.side, static_cast<int>(weld_range_pos(r.start, r.end, t)), i, j);
    return B.slot0 + weld_slot(B.ni, B.nj, i, j);
}

__global__ __launch_bounds__(WELD_THREADS) void k_weld_hook(const WeldBlock* __restrict__ blocks, const tm_connection* __restrict__ conns, int32_t* parent) {
    const tm_connection& c = conns[blockIdx.y];
    if (c.has_periodicity) return;
    const int t = static_cast<int>(blockIdx.x) * WELD_THREADS + static_cast<int>(threadIdx.x);
    if (t >= static_cast<int>(weld_range_length(c.r[0].start, c.r[0].end))) return;   // both ranges have this length and stay on their sides (weld_plan)
    int a = weld_find(parent, weld_slot_of(blocks, c.r[0], t)), b = weld_find(parent, weld_slot_of(blocks, c.r[1], t));
    while (a != b) {
        if (a < b) {
            const int s = a;
            a = b;
            b = s;
        }
        const int old = atomicCAS(parent + a, a, b);   // root a under the smaller root b
        if (old == a) break;
        a = weld_find(parent, old);   // old < a: somebody hooked a meanwhile -- this thread's pair has come closer to its root
        b = weld_find(parent, b);
    }
}

__global__ __launch_bounds__(WELD_THREADS) void k_weld_compress(int32_t* parent, int32_t* __restrict__ count, int nslots) {
    const int s = static_cast<int>(blockIdx.x) * WELD_THREADS + static_cast<int>(threadIdx.x);
    if (s >= nslots) return;
    const int r = weld_find(parent, s);
    __atomic_store_n(parent + s, r, __ATOMIC_RELAXED);   // a reader on its way through s sees the old label or the root: both lead there
    atomicAdd(count + r, 1);
}

__global__ __launch_bounds__(WELD_THREADS) void k_weld_classes(const int32_t* __restrict__ parent, const int32_t* __restrict__ count, int nslots,
                                                               unsigned long long* __restrict__ counters) {
    __shared__ unsigned sh[5];
    if (threadIdx.x < 5) sh[threadIdx.x] = 0;
    __syncthreads();
    const int s = static_cast<int>(blockIdx.x) * WELD_THREADS + static_cast<int>(threadIdx.x);
    if (s < nslots && parent[s] == s) {
        const int n = count[s];
        if (n >= 2) {
            atomicAdd(&sh[n == 2 ? WELD_C2 : n == 3 ? WELD_C3 : n == 4 ? WELD_C4 : WELD_C5], 1u);
            atomicMax(&sh[WELD_MAX_CLASS], static_cast<unsigned>(n));
        }
    }
    __syncthreads();
    if (threadIdx.x < 4 && sh[threadIdx.x]) atomicAdd(counters + threadIdx.x, static_cast<unsigned long long>(sh[threadIdx.x]));
    if (threadIdx.x == 4 && sh[4]) atomicMax(counters + WELD_MAX_CLASS, static_cast<unsigned long long>(sh[4]));
}

// ------------------------------------------------------------------ 2. number
__global__ __launch_bounds__(WELD_THREADS) void k_weld_count(const WeldBlock* __restrict__ blocks, int nblocks, const int32_t* __restrict__ parent, int N,
                                                             int32_t* __restrict__ part) {
    __shared__ int sh[WELD_WAVES];
    const long long base = static_cast<long long>(blockIdx.x) * WELD_TILE + static_cast<long long>(threadIdx.x) * WELD_PER_THREAD;
    int cnt = 0;
    if (base < N) {
        WeldWalk w;
        walk_start(blocks, nblocks, static_cast<int>(base), w);
        if (base + WELD_PER_THREAD <= N && walk_all_interior(w)) {
            cnt = WELD_PER_THREAD;
        } else {
            for (int q = 0; q < WELD_PER_THREAD && base + q < N; ++q) {
                cnt += weld_owner(w.B, w.i, w.j, parent);
                walk_next(blocks, nblocks, w);
            }
        }
    }
    int total;
    (void)weld_block_exscan(cnt, sh, total);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// sums of WELD_PTILE values each
__global__ __launch_bounds__(WELD_THREADS) void k_weld_psum(const int32_t* __restrict__ in, int n, int32_t* __restrict__ out) {
    __shared__ int sh[WELD_WAVES];
    const int base = static_cast<int>(blockIdx.x) * WELD_PTILE + static_cast<int>(threadIdx.x) * 4;
    int v = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (base + q < n) v += in[base + q];
    int total;
    (void)weld_block_exscan(v, sh, total);
    if (threadIdx.x == 0) out[blockIdx.x] = total;
}
// exclusive prefix of `in` inside each tile of WELD_PTILE values, plus the tile's own offset (tile_off null: one tile, offset 0)
__global__ __launch_bounds__(WELD_THREADS) void k_weld_pscan(const int32_t* __restrict__ in, int n, const int32_t* __restrict__ tile_off, int32_t* __restrict__ out) {
    __shared__ int sh[WELD_WAVES];
    const int base = static_cast<int>(blockIdx.x) * WELD_PTILE + static_cast<int>(threadIdx.x) * 4;
    int x[4], v = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        x[q] = base + q < n ? in[base + q] : 0;
        v += x[q];
    }
    int total;
    int run = weld_block_exscan(v, sh, total) + (tile_off ? tile_off[blockIdx.x] : 0);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (base + q < n) out[base + q] = run;
        run += x[q];
    }
}

__global__ __launch_bounds__(WELD_THREADS) void k_weld_number(const WeldBlock* __restrict__ blocks, int nblocks, const int32_t* __restrict__ parent, int N,
                                                              const int32_t* __restrict__ tile_off, int32_t* __restrict__ map,
                                                              unsigned long long* __restrict__ counters) {
    __shared__ int sh[WELD_WAVES];
    const long long base = static_cast<long long>(blockIdx.x) * WELD_TILE + static_cast<long long>(threadIdx.x) * WELD_PER_THREAD;
    int flag[WELD_PER_THREAD], cnt = 0;
#pragma unroll
    for (int q = 0; q < WELD_PER_THREAD; ++q) flag[q] = 0;
    if (base < N) {
        WeldWalk w;
        walk_start(blocks, nblocks, static_cast<int>(base), w);
        if (base + WELD_PER_THREAD <= N && walk_all_interior(w)) {
#pragma unroll
            for (int q = 0; q < WELD_PER_THREAD; ++q) flag[q] = 1;
        } else {
#pragma unroll
            for (int q = 0; q < WELD_PER_THREAD; ++q) {
                if (base + q < N) {
                    flag[q] = weld_owner(w.B, w.i, w.j, parent);
                    walk_next(blocks, nblocks, w);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < WELD_PER_THREAD; ++q) cnt += flag[q];
    }
    int total;
    int run = weld_block_exscan(cnt, sh, total) + tile_off[blockIdx.x];
    if (base >= N) return;
    int id[WELD_PER_THREAD];
#pragma unroll
    for (int q = 0; q < WELD_PER_THREAD; ++q) {
        id[q] = flag[q] ? run : -1;   // non-owners: k_weld_slaves
        run += flag[q];
    }
    if (base + WELD_PER_THREAD <= N) {   // base is a multiple of 8: 32-byte aligned
        int4* dst = reinterpret_cast<int4*>(map + base);
        dst[0] = make_int4(id[0], id[1], id[2], id[3]);
        dst[1] = make_int4(id[4], id[5], id[6], id[7]);
    } else {
#pragma unroll
        for (int q = 0; q < WELD_PER_THREAD; ++q)
            if (base + q < N) map[base + q] = id[q];
    }
    if (base + WELD_PER_THREAD >= N) counters[WELD_NODES_OUT] = static_cast<unsigned long long>(run);   // the thread of node N-1: every owner counted
}

// block of a global perimeter slot
__device__ __forceinline__ int weld_block_of_slot(const WeldBlock* __restrict__ blocks, int nblocks, int s) {
    int lo = 0, hi = nblocks - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (blocks[mid].slot0 <= s) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
__device__ __forceinline__ int weld_flat_of_slot(const WeldBlock& B, int s) {
    int i, j;
    weld_slot_node(B.ni, B.nj, s - B.slot0, i, j);
    return B.off + j * B.ni + i;
}

// grid.y = block, grid.x over its perimeter: a non-owner takes the id of its root (an owner: written by k_weld_number, which has ended)
__global__ __launch_bounds__(WELD_THREADS) void k_weld_slaves(const WeldBlock* __restrict__ blocks, int nblocks, const int32_t* __restrict__ parent, int32_t* map) {
    const WeldBlock B = blocks[blockIdx.y];
    const int ls = static_cast<int>(blockIdx.x) * WELD_THREADS + static_cast<int>(threadIdx.x);
    if (ls >= weld_perimeter(B.ni, B.nj)) return;
    const int s = B.slot0 + ls, r = parent[s];
    if (r == s) return;
    map[weld_flat_of_slot(B, s)] = map[weld_flat_of_slot(blocks[weld_block_of_slot(blocks, nblocks, r)], r)];
}

// ------------------------------------------------------------------ 3. points
// planes in flat order, layer-major: component c of (layer k, node n) at src[c*src_stride + k*N + n]; grid.y = layer
__global__ __launch_bounds__(WELD_THREADS) void k_weld_gather(const WeldBlock* __restrict__ blocks, int nblocks, const int32_t* __restrict__ parent,
                                                              const int32_t* __restrict__ map, int N, int nodes_out, int ncomp, const double* __restrict__ src,
                                                              long long src_stride, double* __restrict__ out, long long out_stride) {
    const long long base = static_cast<long long>(blockIdx.x) * WELD_TILE + static_cast<long long>(threadIdx.x) * WELD_PER_THREAD;
    if (base >= N) return;
    const long long k = blockIdx.y;
    WeldWalk w;
    walk_start(blocks, nblocks, static_cast<int>(base), w);
    const bool inside = base + WELD_PER_THREAD <= N && walk_all_interior(w);
    for (int q = 0; q < WELD_PER_THREAD && base + q < N; ++q) {
        const bool own = inside || weld_owner(w.B, w.i, w.j, parent);
        if (!inside) walk_next(blocks, nblocks, w);
        if (!own) continue;
        const long long from = k * N + base + q, to = k * nodes_out + map[base + q];
        for (int c = 0; c < ncomp; ++c) out[c * out_stride + to] = src[c * src_stride + from];
    }
}

// one block of a handle: X[i*nj + j] interleaved; loads with the lanes along j, stores along i (k_soa_planes' transpose)
__global__ __launch_bounds__(WELD_THREADS) void k_weld_gather_resident(const double2* __restrict__ X, WeldBlock B, const int32_t* __restrict__ parent,
                                                                       const int32_t* __restrict__ map, double* __restrict__ ox, double* __restrict__ oy) {
    __shared__ double2 tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int i0 = blockIdx.y * 32, j0 = blockIdx.x * 32;
    // the ids of the four nodes this thread will store, -1 where it stores nothing: loaded beside the coordinates, not behind the barrier,
    // so that no store waits for a load of its own address
    int id[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int j = j0 + ty + 8 * r, i = i0 + tx;
        const bool in = i < B.ni && j < B.nj;
        const int m = in ? map[B.off + j * B.ni + i] : -1;
        id[r] = in && weld_owner(B, i, j, parent) ? m : -1;
    }
#pragma unroll
    for (int r = 0; r < 32; r += 8) {
        const int i = i0 + ty + r, j = j0 + tx;
        if (i < B.ni && j < B.nj) tile[ty + r][tx] = X[static_cast<size_t>(i) * B.nj + j];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (id[r] >= 0) {
            const double2 v = tile[tx][ty + 8 * r];
            ox[id[r]] = v.x;
            oy[id[r]] = v.y;
        }
    }
}

__device__ __forceinline__ void gap_take(WeldGap& a, double g, unsigned long long node) {
    if (g > a.gap || (g == a.gap && node < a.node)) {
        a.gap = g;
        a.node = node;
    }
}
__device__ __forceinline__ void gap_block_reduce(WeldGap a, WeldGap* sh, WeldGap* out) {   // sh[WELD_THREADS]
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int off = WELD_THREADS / 2; off > 0; off >>= 1) {
        if (static_cast<int>(threadIdx.x) < off) gap_take(sh[threadIdx.x], sh[threadIdx.x + off].gap, sh[threadIdx.x + off].node);
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = sh[0];
}

// grid.y = block, grid.x over its perimeter: the non-owners against the welded planes
__global__ __launch_bounds__(WELD_THREADS) void k_weld_gap(const WeldBlock* __restrict__ blocks, const int32_t* __restrict__ parent, const int32_t* __restrict__ map,
                                                           int N, int nodes_out, WeldSrc src, const double* __restrict__ out, long long out_stride,
                                                           WeldGap* __restrict__ partials) {
    __shared__ WeldGap sh[WELD_THREADS];
    const WeldBlock B = blocks[blockIdx.y];
    const int ls = static_cast<int>(blockIdx.x) * WELD_THREADS + static_cast<int>(threadIdx.x);
    WeldGap acc{0.0, 0ull};
    if (ls < weld_perimeter(B.ni, B.nj)) {
        const int s = B.slot0 + ls;
        if (parent[s] != s) {
            int i, j;
            weld_slot_node(B.ni, B.nj, ls, i, j);
            const int n = B.off + j * B.ni + i, id = map[n];
            for (long long k = 0; k < src.layers; ++k) {
                double g = 0.0;
                for (int c = 0; c < src.ncomp; ++c) {
                    double mine;
                    if (src.resident) {
                        const double2 v = src.resident[blockIdx.y][static_cast<size_t>(i) * B.nj + j];
                        mine = c == 0 ? v.x : v.y;
                    } else {
                        mine = src.planes[c * src.comp_stride + k * N + n];
                    }
                    const double d = fabs(mine - out[c * out_stride + k * nodes_out + id]);
                    if (d > g) g = d;
                }
                gap_take(acc, g, static_cast<unsigned long long>(k) * static_cast<unsigned long long>(N) + static_cast<unsigned long long>(n));
            }
        }
    }
    gap_block_reduce(acc, sh, partials + static_cast<size_t>(blockIdx.y) * gridDim.x + blockIdx.x);
}
__global__ __launch_bounds__(WELD_THREADS) void k_weld_gap_final(const WeldGap* __restrict__ partials, int n, WeldGap* __restrict__ result) {
    __shared__ WeldGap sh[WELD_THREADS];
    WeldGap acc{0.0, 0ull};
    for (int r = threadIdx.x; r < n; r += WELD_THREADS) gap_take(acc, partials[r].gap, partials[r].node);
    gap_block_reduce(acc, sh, result);
}

// ------------------------------------------------------------------ 4. cells
// one block: a workgroup takes `per_wg` whole elements (per_wg * npe <= WELD_TILE ids); out: the block's first id
__global__ __launch_bounds__(WELD_THREADS) void k_weld_cells(const int32_t* __restrict__ map, WeldBlock B, int p, int Ei, int Ej, int ncells, int npe, int per_wg,
                                                             const int32_t* __restrict__ local, int nodes_out, int32_t* __restrict__ out) {
    __shared__ int32_t sh_local[WELD_MAX_NPE];
    if (static_cast<int>(threadIdx.x) < npe) sh_local[threadIdx.x] = local[threadIdx.x];
    __syncthreads();
    const int el0 = static_cast<int>(blockIdx.x) * per_wg;
    const int here = ncells - el0 < per_wg ? ncells - el0 : per_wg;   // >= 1 by the grid
    int32_t* dst = out + static_cast<size_t>(el0) * npe;
    for (int idx = threadIdx.x; idx < here * npe; idx += WELD_THREADS) {
        const int k = idx / npe, q = idx - k * npe, el = el0 + k;
        const int e = el % Ei, fg = el / Ei, f = fg % Ej, g = fg / Ej;
        const int l = sh_local[q], a = l & 255, b = (l >> 8) & 255, c = l >> 16;
        dst[idx] = (g * p + c) * nodes_out + map[B.off + (f * p + b) * B.ni + e * p + a];   // <= layers * nodes_out - 1: fits (weld_layers)
    }
}

// ------------------------------------------------------------------ host driver
static unsigned weld_groups(int64_t n, int per) { return static_cast<unsigned>((n + per - 1) / per); }

void WeldDev::link(const WeldPlan& pl, hipStream_t st) {
    const int nslots = static_cast<int>(pl.slots);
    blocks.grow(sizeof(WeldBlock) * pl.blocks.size(), "weld block table");
    conns.grow(sizeof(tm_connection) * pl.conns.size(), "weld connection table");
    parent.grow(sizeof(int32_t) * nslots, "weld labels");
    count.grow(sizeof(int32_t) * nslots, "weld class counts");
    counters.grow(sizeof(unsigned long long) * WELD_COUNTERS, "weld counters");
    HIPCHK(hipMemcpyAsync(blocks.p, pl.blocks.data(), sizeof(WeldBlock) * pl.blocks.size(), hipMemcpyHostToDevice, st));
    if (!pl.conns.empty()) HIPCHK(hipMemcpyAsync(conns.p, pl.conns.data(), sizeof(tm_connection) * pl.conns.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(counters.p, 0, sizeof(unsigned long long) * WELD_COUNTERS, st));
    const dim3 over_slots(weld_groups(nslots, WELD_THREADS));
    hipLaunchKernelGGL(k_weld_init, over_slots, dim3(WELD_THREADS), 0, st, parent.as<int32_t>(), count.as<int32_t>(), nslots);
    HIPCHK(hipGetLastError());
    if (pl.max_pairs > 0) {   // the connection table as it stands: grid.y = connection (at most 65535: weld_plan)
        hipLaunchKernelGGL(k_weld_hook, dim3(weld_groups(pl.max_pairs, WELD_THREADS), static_cast<unsigned>(pl.conns.size())), dim3(WELD_THREADS), 0, st,
                           blocks.as<WeldBlock>(), conns.as<tm_connection>(), parent.as<int32_t>());
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_weld_compress, over_slots, dim3(WELD_THREADS), 0, st, parent.as<int32_t>(), count.as<int32_t>(), nslots);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_weld_classes, over_slots, dim3(WELD_THREADS), 0, st, parent.as<int32_t>(), count.as<int32_t>(), nslots, counters.as<unsigned long long>());
    HIPCHK(hipGetLastError());
}

static int weld_max_perimeter(const WeldPlan& pl) {
    int m = 0;
    for (const WeldBlock& b : pl.blocks) m = std::max(m, weld_perimeter(b.ni, b.nj));
    return m;
}

void WeldDev::number(const WeldPlan& pl, hipStream_t st) {
    const int N = static_cast<int>(pl.nodes), nb = pl.nblocks();
    const int t1 = static_cast<int>(weld_groups(N, WELD_TILE)), t2 = static_cast<int>(weld_groups(t1, WELD_PTILE));   // t1 <= 2^20, t2 <= 1024
    map.grow(sizeof(int32_t) * static_cast<size_t>(N), "weld map");
    part1.grow(sizeof(int32_t) * t1, "weld tile sums");
    off1.grow(sizeof(int32_t) * t1, "weld tile offsets");
    part2.grow(sizeof(int32_t) * t2, "weld tile sums, second level");
    off2.grow(sizeof(int32_t) * t2, "weld tile offsets, second level");
    const dim3 wg(WELD_THREADS);
    hipLaunchKernelGGL(k_weld_count, dim3(t1), wg, 0, st, blocks.as<WeldBlock>(), nb, parent.as<int32_t>(), N, part1.as<int32_t>());
    HIPCHK(hipGetLastError());
    if (t2 == 1) {
        hipLaunchKernelGGL(k_weld_pscan, dim3(1), wg, 0, st, part1.as<int32_t>(), t1, static_cast<const int32_t*>(nullptr), off1.as<int32_t>());
    } else {   // the tile sums span more than one tile themselves: their sums, scanned by one workgroup (t2 <= WELD_PTILE), come back as tile offsets
        hipLaunchKernelGGL(k_weld_psum, dim3(t2), wg, 0, st, part1.as<int32_t>(), t1, part2.as<int32_t>());
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_weld_pscan, dim3(1), wg, 0, st, part2.as<int32_t>(), t2, static_cast<const int32_t*>(nullptr), off2.as<int32_t>());
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_weld_pscan, dim3(t2), wg, 0, st, part1.as<int32_t>(), t1, off2.as<int32_t>(), off1.as<int32_t>());
    }
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_weld_number, dim3(t1), wg, 0, st, blocks.as<WeldBlock>(), nb, parent.as<int32_t>(), N, off1.as<int32_t>(), map.as<int32_t>(),
                       counters.as<unsigned long long>());
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_weld_slaves, dim3(weld_groups(weld_max_perimeter(pl), WELD_THREADS), nb), wg, 0, st, blocks.as<WeldBlock>(), nb, parent.as<int32_t>(),
                       map.as<int32_t>());
    HIPCHK(hipGetLastError());
}

void WeldDev::exscan(hipStream_t st, const int32_t* in, int n, int32_t* out_scan) {
    const int t1 = static_cast<int>(weld_groups(n, WELD_PTILE)), t2 = static_cast<int>(weld_groups(t1, WELD_PTILE));
    if (t2 > WELD_PTILE) throw TmError(TM_E_ARG, "more than 2^30 values to scan");
    part1.grow(sizeof(int32_t) * t1, "weld tile sums");
    off1.grow(sizeof(int32_t) * t1, "weld tile offsets");
    part2.grow(sizeof(int32_t) * t2, "weld tile sums, second level");
    off2.grow(sizeof(int32_t) * t2, "weld tile offsets, second level");
    const dim3 wg(WELD_THREADS);
    const int32_t* none = nullptr;
    if (t1 == 1) {
        hipLaunchKernelGGL(k_weld_pscan, dim3(1), wg, 0, st, in, n, none, out_scan);
        HIPCHK(hipGetLastError());
        return;
    }
    hipLaunchKernelGGL(k_weld_psum, dim3(t1), wg, 0, st, in, n, part1.as<int32_t>());
    HIPCHK(hipGetLastError());
    if (t2 == 1) {
        hipLaunchKernelGGL(k_weld_pscan, dim3(1), wg, 0, st, static_cast<const int32_t*>(part1.as<int32_t>()), t1, none, off1.as<int32_t>());
    } else {
        hipLaunchKernelGGL(k_weld_psum, dim3(t2), wg, 0, st, static_cast<const int32_t*>(part1.as<int32_t>()), t1, part2.as<int32_t>());
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_weld_pscan, dim3(1), wg, 0, st, static_cast<const int32_t*>(part2.as<int32_t>()), t2, none, off2.as<int32_t>());
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_weld_pscan, dim3(t2), wg, 0, st, static_cast<const int32_t*>(part1.as<int32_t>()), t1, static_cast<const int32_t*>(off2.as<int32_t>()),
                           off1.as<int32_t>());
    }
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_weld_pscan, dim3(t1), wg, 0, st, in, n, static_cast<const int32_t*>(off1.as<int32_t>()), out_scan);
    HIPCHK(hipGetLastError());
}

void WeldDev::read_map(const WeldPlan& pl, hipStream_t st, int32_t* host_map, tm_weld_info* info) {
    unsigned long long c[WELD_COUNTERS];
    HIPCHK(hipMemcpyAsync(c, counters.p, sizeof(c), hipMemcpyDeviceToHost, st));
    if (host_map) HIPCHK(hipMemcpyAsync(host_map, map.p, sizeof(int32_t) * static_cast<size_t>(pl.nodes), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (!info) return;
    std::memset(info, 0, sizeof(*info));
    info->nodes_in = static_cast<uint64_t>(pl.nodes);
    info->nodes_out = c[WELD_NODES_OUT];
    info->classes_2 = c[WELD_C2];
    info->classes_3 = c[WELD_C3];
    info->classes_4 = c[WELD_C4];
    info->classes_5_up = c[WELD_C5];
    info->max_class = c[WELD_MAX_CLASS] ? c[WELD_MAX_CLASS] : 1;
    info->periodic_pairs = static_cast<uint64_t>(pl.periodic_pairs);
}

void WeldDev::upload_map(const WeldPlan& pl, hipStream_t st, const int32_t* host_map) {
    map.grow(sizeof(int32_t) * static_cast<size_t>(pl.nodes), "weld map");
    HIPCHK(hipMemcpyAsync(map.p, host_map, sizeof(int32_t) * static_cast<size_t>(pl.nodes), hipMemcpyHostToDevice, st));
}

void WeldDev::gap_run(const WeldPlan& pl, hipStream_t st, const WeldSrc& s, int64_t nodes_out, WeldGap* host_gap) {
    const dim3 grid(weld_groups(weld_max_perimeter(pl), WELD_THREADS), pl.nblocks());
    const int npart = static_cast<int>(grid.x * grid.y);
    gaps.grow(sizeof(WeldGap) * npart, "weld gap records");
    gap.grow(sizeof(WeldGap), "weld gap record");
    hipLaunchKernelGGL(k_weld_gap, grid, dim3(WELD_THREADS), 0, st, blocks.as<WeldBlock>(), parent.as<int32_t>(), map.as<int32_t>(), static_cast<int>(pl.nodes),
                       static_cast<int>(nodes_out), s, out.as<double>(), static_cast<long long>(s.layers) * nodes_out, gaps.as<WeldGap>());
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_weld_gap_final, dim3(1), dim3(WELD_THREADS), 0, st, gaps.as<WeldGap>(), npart, gap.as<WeldGap>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(host_gap, gap.p, sizeof(WeldGap), hipMemcpyDeviceToHost, st));
}

void WeldDev::points_planes(const WeldPlan& pl, hipStream_t st, int ncomp, int64_t layers, int64_t nodes_out, const double* const* planes, double* const* host_out,
                            WeldGap* host_gap) {
    const int64_t N = pl.nodes;
    const int nb = pl.nblocks();
    if (layers > 65535) throw TmError(TM_E_ARG, "more than 65535 layers");
    const size_t src_stride = static_cast<size_t>(layers) * N, out_stride = static_cast<size_t>(layers) * nodes_out;
    src.grow(sizeof(double) * src_stride * ncomp, "weld source planes");
    out.grow(sizeof(double) * out_stride * ncomp, "welded planes");
    for (int c = 0; c < ncomp; ++c)
        for (int b = 0; b < nb; ++b) {
            const size_t n = static_cast<size_t>(pl.blocks[b].ni) * pl.blocks[b].nj;
            for (int64_t k = 0; k < layers; ++k)
                HIPCHK(hipMemcpyAsync(src.as<double>() + c * src_stride + k * N + pl.blocks[b].off, planes[static_cast<size_t>(c) * nb + b] + k * n, sizeof(double) * n,
                                      hipMemcpyHostToDevice, st));
        }
    hipLaunchKernelGGL(k_weld_gather, dim3(weld_groups(N, WELD_TILE), static_cast<unsigned>(layers)), dim3(WELD_THREADS), 0, st, blocks.as<WeldBlock>(), nb,
                       parent.as<int32_t>(), map.as<int32_t>(), static_cast<int>(N), static_cast<int>(nodes_out), ncomp, src.as<double>(),
                       static_cast<long long>(src_stride), out.as<double>(), static_cast<long long>(out_stride));
    HIPCHK(hipGetLastError());
    gap_run(pl, st, WeldSrc{src.as<double>(), static_cast<long long>(src_stride), nullptr, ncomp, static_cast<int>(layers)}, nodes_out, host_gap);
    for (int c = 0; c < ncomp; ++c) HIPCHK(hipMemcpyAsync(host_out[c], out.as<double>() + c * out_stride, sizeof(double) * out_stride, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
}

void WeldDev::points_resident(const WeldPlan& pl, hipStream_t st, const std::vector<const double2*>& X, int64_t nodes_out, double* x, double* y, WeldGap* host_gap) {
    const int nb = pl.nblocks();
    out.grow(sizeof(double) * 2 * static_cast<size_t>(nodes_out), "welded planes");
    ptrs.grow(sizeof(const double2*) * nb, "weld block pointers");
    HIPCHK(hipMemcpyAsync(ptrs.p, X.data(), sizeof(const double2*) * nb, hipMemcpyHostToDevice, st));
    double* ox = out.as<double>();
    double* oy = ox + nodes_out;
    for (int b = 0; b < nb; ++b) {
        const WeldBlock& B = pl.blocks[b];
        const dim3 grid((B.nj + 31) / 32, (B.ni + 31) / 32);
        if (grid.y > 65535u) throw TmError(TM_E_SIZE, "InconsistentSize: too many rows for one launch");
        hipLaunchKernelGGL(k_weld_gather_resident, grid, dim3(WELD_THREADS), 0, st, X[b], B, parent.as<int32_t>(), map.as<int32_t>(), ox, oy);
        HIPCHK(hipGetLastError());
    }
    gap_run(pl, st, WeldSrc{nullptr, 0, static_cast<const double2* const*>(ptrs.p), 2, 1}, nodes_out, host_gap);
    if (x) HIPCHK(hipMemcpyAsync(x, ox, sizeof(double) * nodes_out, hipMemcpyDeviceToHost, st));   // null: the planes are wanted on the device only (K19)
    if (y) HIPCHK(hipMemcpyAsync(y, oy, sizeof(double) * nodes_out, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
}

void WeldDev::cells_run(const WeldPlan& pl, hipStream_t st, const std::vector<int64_t>& cells_of, int order, uint64_t nk, int64_t nodes_out, int32_t* host_cells) {
    const bool hex = nk >= 2;
    const std::vector<int32_t> order_table = weld_local_order(order, hex);
    const int npe = static_cast<int>(order_table.size()), per_wg = WELD_TILE / npe;   // npe <= WELD_MAX_NPE: orders 1 .. 8 flat, 1 .. 4 in 3-D
    const size_t total = static_cast<size_t>(cells_of.back()) * npe;
    local.grow(sizeof(int32_t) * WELD_MAX_NPE, "weld local order");
    cells.grow(sizeof(int32_t) * total, "welded cells");
    HIPCHK(hipMemcpyAsync(local.p, order_table.data(), sizeof(int32_t) * npe, hipMemcpyHostToDevice, st));
    for (int b = 0; b < pl.nblocks(); ++b) {
        const WeldBlock& B = pl.blocks[b];
        const int ncells = static_cast<int>(cells_of[b + 1] - cells_of[b]);
        if (ncells == 0) continue;
        hipLaunchKernelGGL(k_weld_cells, dim3(weld_groups(ncells, per_wg)), dim3(WELD_THREADS), 0, st, map.as<int32_t>(), B, order, (B.ni - 1) / order,
                           (B.nj - 1) / order, ncells, npe, per_wg, local.as<int32_t>(), static_cast<int>(nodes_out),
                           cells.as<int32_t>() + static_cast<size_t>(cells_of[b]) * npe);
        HIPCHK(hipGetLastError());
    }
    if (total) HIPCHK(hipMemcpyAsync(host_cells, cells.p, sizeof(int32_t) * total, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
}

// ------------------------------------------------------------------ handle: the coordinates resident in X
// the handle's topology as a mesh description without coordinates, and the resident interleaved blocks
void Smoother::weld_tables(std::vector<tm_block>& tb, std::vector<tm_connection>& tc, std::vector<tm_condition>& tq, std::vector<const double2*>& blocks_x) {
    for (int64_t b = 0; b < topo.nblocks(); ++b) tb.push_back(tm_block{nullptr, static_cast<uint64_t>(topo.ni[b]), static_cast<uint64_t>(topo.nj[b])});
    for (const TopoConn& c : topo.conns) {
        tm_connection t{};
        for (int s = 0; s < 2; ++s) t.r[s] = tm_range{static_cast<uint64_t>(c.r[s].block), c.r[s].side, 0, static_cast<uint64_t>(c.r[s].start), static_cast<uint64_t>(c.r[s].end)};
        t.has_periodicity = c.periodic ? 1 : 0;
        t.periodicity[0] = c.per[0];
        t.periodicity[1] = c.per[1];
        tc.push_back(t);
    }
    for (const TopoCond& c : topo.bcs)
        tq.push_back(tm_condition{tm_range{static_cast<uint64_t>(c.range.block), c.range.side, 0, static_cast<uint64_t>(c.range.start), static_cast<uint64_t>(c.range.end)}, c.kind, 0});
    for (int64_t b = 0; b < topo.nblocks(); ++b) {
        const auto it = std::lower_bound(lp.owned_blocks.begin(), lp.owned_blocks.end(), b);
        if (it == lp.owned_blocks.end() || *it != b) throw TmError(TM_E_UNSUPPORTED, "a block is not owned by this handle");
        blocks_x.push_back(X + lp.local_start[it - lp.owned_blocks.begin()]);
    }
}

void Smoother::weld_host(int32_t* map_out, double* x, double* y, tm_weld_info* info) {
    if (lp.nranks > 1) throw TmError(TM_E_UNSUPPORTED, "welding needs every block in one handle: not served with rank hooks");
    std::vector<tm_block> tb;
    std::vector<tm_connection> tc;
    std::vector<tm_condition> tq;
    std::vector<const double2*> blocks_x;
    weld_tables(tb, tc, tq, blocks_x);
    tm_mesh_desc desc{tb.data(), tb.size(), tc.data(), tc.size(), nullptr, 0};
    const WeldPlan pl = weld_plan(&desc);
    if (!welddev) welddev = new WeldDev();
    tm_weld_info rec;
    welddev->link(pl, stream);
    welddev->number(pl, stream);
    welddev->read_map(pl, stream, map_out, &rec);
    WeldGap gap{0.0, 0ull};
    welddev->points_resident(pl, stream, blocks_x, static_cast<int64_t>(rec.nodes_out), x, y, &gap);
    rec.max_gap = gap.gap;
    rec.gap_node = gap.node;
    if (pl.periodic_pairs) {   // from the welded planes; the map is needed on the host for it
        std::vector<int32_t> m;
        const int32_t* mp = map_out;
        if (!mp) {
            m.resize(static_cast<size_t>(pl.nodes));
            HIPCHK(hipMemcpy(m.data(), welddev->map.p, sizeof(int32_t) * m.size(), hipMemcpyDeviceToHost));
            mp = m.data();
        }
        const double* planes[2] = {x, y};
        rec.periodic_gap = weld_periodic_gap(pl, mp, 2, 1, rec.nodes_out, planes);
    }
    if (info) *info = rec;
}

}  // namespace tmh

using namespace tmh;

extern "C" int tm_weld_map(const tm_mesh_desc* mesh, int32_t* map, tm_weld_info* info) {
    return guarded([&]() {
        const WeldPlan pl = weld_plan(mesh);
        require_gfx950();
        WeldDev dev;
        dev.link(pl, nullptr);
        dev.number(pl, nullptr);
        dev.read_map(pl, nullptr, map, info);
        return TM_OK;
    });
}

extern "C" int tm_weld_points(const tm_mesh_desc* mesh, const int32_t* map, int32_t ncomp, uint64_t nk, const double* const* planes, double* const* out,
                              tm_weld_info* info) {
    return guarded([&]() {
        const WeldPlan pl = weld_plan(mesh);
        weld_points_check(pl, map, ncomp, planes, out);
        const uint64_t nodes_out = weld_nodes_out(pl, map);
        const int64_t layers = weld_layers(nk, nodes_out);
        require_gfx950();
        WeldDev dev;
        dev.link(pl, nullptr);   // the owner flags; the ids are the caller's
        dev.upload_map(pl, nullptr, map);
        WeldGap gap{0.0, 0ull};
        dev.points_planes(pl, nullptr, ncomp, layers, static_cast<int64_t>(nodes_out), planes, out, &gap);
        if (info) {
            info->nodes_in = static_cast<uint64_t>(pl.nodes);
            info->nodes_out = nodes_out;
            info->periodic_pairs = static_cast<uint64_t>(pl.periodic_pairs);
            info->max_gap = gap.gap;
            info->gap_node = gap.node;
            info->periodic_gap = weld_periodic_gap(pl, map, ncomp, static_cast<uint64_t>(layers), nodes_out, out);
        }
        return TM_OK;
    });
}

extern "C" int tm_weld_cells(const tm_mesh_desc* mesh, const int32_t* map, uint64_t nodes_out, int32_t order, uint64_t nk, int32_t* cells) {
    return guarded([&]() {
        weld_layers(nk, nodes_out);   // sizes first: nothing is read when the ids cannot be held
        const WeldPlan pl = weld_plan(mesh);
        std::vector<int64_t> cells_of;
        weld_cells_plan(mesh, pl, order, nk, cells_of);
        if (!map || !cells) throw TmError(TM_E_ARG, "null argument");
        require_gfx950();
        WeldDev dev;
        dev.upload_map(pl, nullptr, map);
        dev.cells_run(pl, nullptr, cells_of, order, nk, static_cast<int64_t>(nodes_out), cells);
        return TM_OK;
    });
}

extern "C" int tm_smoother_weld(tm_smoother* s, int32_t* map_or_null, double* X, double* Y, tm_weld_info* info) {
    return guarded([&]() {
        if (!s || !smoother_is_live(s)) throw TmError(TM_E_ARG, "not a live handle");
        if (!X || !Y) throw TmError(TM_E_ARG, "X and Y are needed");
        s->impl.weld_host(map_or_null, X, Y, info);
        return TM_OK;
    });
}
