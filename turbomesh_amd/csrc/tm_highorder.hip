// K13 high-order elevation: one launch per block elevates every element of order p, writes the two planes transposed to i fastest and
//     forms the element records.  gfx950, wave64.  Definitions: include/tm_hip.h, "high-order elements"; the contraction of a target
//     column and the records are tm_highorder.hpp, shared with the host loop, so device and host agree bit for bit.
//
// Tile.  A workgroup takes E x E whole elements, E = 32 / p (16 at p = 1): 33 x 33 source nodes at p = 2, 4, 8, 31 x 31 at p = 3, 5, 6,
// 29 x 29 at p = 7 and 17 x 17 at p = 1 (one lane per element forms the records: at most 256 elements per tile).  The nodes on tile seams are read by both neighbours: that is the halo (6 % of the loads).  The tile
// goes through LDS once: loaded with the lanes along j (one 16 B node per lane, rows of the block are contiguous), read by the
// contraction, and -- with TM_HO_EQUIDISTANT or p = 1, where the nodes are copied -- by the transposed store, which is K8's.
//
// Contraction.  One lane takes one target column (e, f, b) of an element: it forms W[m][b] for the p+1 source rows of the element from
// LDS with ITS rows b of T and D (held in registers, read once from the table in global memory: b differs between the lanes of a wave),
// then the p+1 targets a along i with rows a of T and D under compile-time indices (scalar loads from the table).  The W of a column
// serve Y, d/du and d/dv: 5(p+1) multiply-adds per component and node.  Lanes run along e first, so the elevated nodes of a column go
// to LDS and leave through the transposed store, coalesced along i.
//
// Records.  The (Jmin, Jmax) of the columns meet in LDS, one lane per element combines them in the order b = 0 .. p, counts the element
// (ho_count_element) and writes its pair; in-wave by shuffles, across the waves through LDS, one HoAcc per workgroup; the histogram by
// integer LDS atomics.  k_ho_finalize (behind k_ho_reduce on blocks of more than 256 workgroups) combines the records in fixed order and
// picks the orientation's candidate set (ho_finish).  No
// floating-point atomics: results do not depend on scheduling.
#include "tm_highorder_dev.hpp"
#include "tm_stack_dev.hpp"
#include "tm_dispatch.hpp"

#include <algorithm>
#include <cstring>

namespace tmh {

// 256 lanes take the E * E * (p+1) target columns of a tile in rounds.  Workgroups sized to whole rounds (384 lanes at p = 2, 320 at
// p = 4) were measured and are slower (437 / 602 us against 306 / 327 us on 4097^2): fewer workgroups fit a CU, and the kernel lives on
// the overlap of one workgroup's loads with another's arithmetic.
constexpr int HO_THREADS = 256, HO_WAVES = HO_THREADS / 64;
constexpr int ho_tile_elements(int p) { return p == 1 ? 16 : 32 / p; }

__device__ __forceinline__ unsigned long long ho_shfl(unsigned long long v, int off) { return __shfl_down(v, off, 64); }

// px, py null: the report alone.  pairs: (Jmin, Jmax) per element, element f*Ei + e, NaN pairs where a J is not finite.
template <int P>
__global__ __launch_bounds__(HO_THREADS) void k_ho_elevate(const double2* __restrict__ X, int ni, int nj, int Ei, int Ej, const double* __restrict__ tab,
                                                           int identity, double* __restrict__ px, double* __restrict__ py, double2* __restrict__ pairs,
                                                           HoAcc* __restrict__ partials) {
    constexpr int E = ho_tile_elements(P), TN = E * P + 1, PITCH = TN | 1, NB = P + 1, TB = E * NB;
    __shared__ double2 sX[TN * PITCH];
    __shared__ double2 sY[TN * PITCH];
    __shared__ double2 sJ[E * TB];
    __shared__ unsigned sh_hist[20];
    __shared__ HoAcc sh_acc[HO_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int e0 = static_cast<int>(blockIdx.y) * E, f0 = static_cast<int>(blockIdx.x) * E;
    const int eli = Ei - e0 < E ? Ei - e0 : E, elj = Ej - f0 < E ? Ej - f0 : E;   // elements of the tile that exist (>= 1 by the grid)
    const int tni = eli * P + 1, tnj = elj * P + 1;                               // its nodes: i0 + tni <= ni, j0 + tnj <= nj
    const int i0 = e0 * P, j0 = f0 * P;
    if (tid < 20) sh_hist[tid] = 0;
    for (int idx = tid; idx < TN * TN; idx += HO_THREADS) {
        const int m = idx / TN, n = idx - m * TN;
        if (m < tni && n < tnj) sX[m * PITCH + n] = X[static_cast<size_t>(i0 + m) * nj + (j0 + n)];
    }
    __syncthreads();

    const double* __restrict__ T = tab;
    const double* __restrict__ D = tab + NB * NB;
    const bool want_y = px != nullptr && !identity;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int it = tid; it < E * TB; it += HO_THREADS) {
        const int e = it % E, col = it / E, f = col / NB, b = col - f * NB;
        if (e >= eli || f >= elj) continue;
        const double2* base = sX + (e * P) * PITCH + f * P;
        auto at = [&](int m, int n) {
            const double2 v = base[m * PITCH + n];
            return QPoint{v.x, v.y};
        };
        double trow[NB], drow[NB];
#pragma unroll
        for (int n = 0; n < NB; ++n) {
            trow[n] = T[b * NB + n];
            drow[n] = D[b * NB + n];
        }
        double cmin, cmax;
        bool cbad;
        const bool own_b = ho_owns(b, P, f, elj);
        double2* ycol = sY + (e * P) * PITCH + f * P + b;
        auto put = [&](int a, double vx, double vy) {
            if (own_b && ho_owns(a, P, e, eli)) ycol[a * PITCH] = double2{vx, vy};
        };
        ho_column<P>(at, trow, drow, T, D, want_y, put, cmin, cmax, cbad);
        sJ[e * TB + col] = cbad ? double2{nan, nan} : double2{cmin, cmax};
    }
    __syncthreads();

    if (px) {   // K8's transposed store: lanes along i; a seam node is written by the tile above it, the block's last node by the last tile
        const double2* src = identity ? sX : sY;
        const bool last_i = e0 + eli == Ei, last_j = f0 + elj == Ej;
        for (int idx = tid; idx < TN * TN; idx += HO_THREADS) {
            const int ty = idx / TN, tx = idx - ty * TN;
            if ((tx < tni - 1 || (last_i && tx == tni - 1)) && (ty < tnj - 1 || (last_j && ty == tnj - 1))) {
                const double2 v = src[tx * PITCH + ty];
                const size_t o = static_cast<size_t>(j0 + ty) * ni + (i0 + tx);
                px[o] = v.x;
                py[o] = v.y;
            }
        }
    }

    HoAcc acc;
    ho_init(acc);
    for (int el = tid; el < E * E; el += HO_THREADS) {
        const int e = el % E, f = el / E;
        if (e >= eli || f >= elj) continue;
        const double inf = std::numeric_limits<double>::infinity();
        double jmin = inf, jmax = -inf;
        bool bad = false;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const double2 c = sJ[e * TB + f * NB + b];
            ho_take_column(jmin, jmax, bad, c.x, c.y, c.x != c.x);
        }
        const double2* base = sX + (e * P) * PITCH + f * P;
        const double2 A = base[0], B = base[P * PITCH], C = base[P * PITCH + P], Dn = base[P];
        const double area = ho_corner_area(QPoint{A.x, A.y}, QPoint{B.x, B.y}, QPoint{C.x, C.y}, QPoint{Dn.x, Dn.y});
        const int bin = ho_count_element(jmin, jmax, bad, area, static_cast<unsigned long long>(e0 + e) * Ej + (f0 + f), acc);
        if (bin >= 0) atomicAdd(&sh_hist[bin], 1u);
        if (pairs) pairs[static_cast<size_t>(f0 + f) * Ei + (e0 + e)] = bad ? double2{nan, nan} : double2{jmin, jmax};
    }
    // in-wave, fixed tree
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            acc.n[s] += ho_shfl(acc.n[s], off);
            q_take_min(acc.sj[s], acc.at[s], __shfl_down(acc.sj[s], off, 64), ho_shfl(acc.at[s], off));
            double v = __shfl_down(acc.lo[s], off, 64);
            if (v < acc.lo[s]) acc.lo[s] = v;
            v = __shfl_down(acc.hi[s], off, 64);
            if (v > acc.hi[s]) acc.hi[s] = v;
        }
        acc.asum += __shfl_down(acc.asum, off, 64);
        acc.aabs += __shfl_down(acc.aabs, off, 64);
    }
    if (lane == 0) sh_acc[wave] = acc;   // hist is zero in every lane: the bins are in sh_hist
    __syncthreads();
    if (tid == 0) {
        HoAcc t = sh_acc[0];
        for (int w = 1; w < HO_WAVES; ++w) ho_combine(t, sh_acc[w]);
        for (int k = 0; k < 20; ++k) t.hist[k / 10][k % 10] = sh_hist[k];
        partials[static_cast<size_t>(blockIdx.y) * gridDim.x + blockIdx.x] = t;
    }
}

// large blocks: workgroup g reduces the records [g * chunk, (g+1) * chunk) to one
__global__ __launch_bounds__(64) void k_ho_reduce(const HoAcc* __restrict__ partials, int nwg, int chunk, HoAcc* __restrict__ out) {
    __shared__ HoAcc sh[64];
    const int begin = static_cast<int>(blockIdx.x) * chunk, end = begin + chunk < nwg ? begin + chunk : nwg;
    records_reduce_wave<HoAcc, ho_init, ho_combine>(partials, begin, end, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = sh[0];
}
__global__ __launch_bounds__(64) void k_ho_finalize(const HoAcc* __restrict__ partials, int nwg, unsigned long long block, int Ei, int Ej, int order,
                                                    tm_ho_quality* __restrict__ out) {
    __shared__ HoAcc sh[64];
    records_reduce_wave<HoAcc, ho_init, ho_combine>(partials, 0, nwg, sh);
    if (threadIdx.x == 0) ho_finish(sh[0], block, static_cast<uint64_t>(Ei), static_cast<uint64_t>(Ej), order, out);
}

// ------------------------------------------------------------------ host driver
void ho_reduce_launch(const HoAcc* partials, int nrec, int chunk, int groups, HoAcc* out, hipStream_t st) {
    hipLaunchKernelGGL(k_ho_reduce, dim3(groups), dim3(64), 0, st, partials, nrec, chunk, out);
}

void HoDev::run(const HoPlan& pl, const double2* X, int ni, int nj, uint64_t block, hipStream_t st, double* x, double* y, tm_ho_quality* q, double* sj) {
    const int p = pl.order, E = ho_tile_elements(p), Ei = (ni - 1) / p, Ej = (nj - 1) / p;
    const size_t n = static_cast<size_t>(ni) * nj, elements = static_cast<size_t>(Ei) * Ej;
    const dim3 grid((Ej + E - 1) / E, (Ei + E - 1) / E);
    if (grid.y > 65535u) throw TmError(TM_E_SIZE, "InconsistentSize: too many element rows for one launch");
    const size_t nwg = static_cast<size_t>(grid.x) * grid.y;
    const bool want_planes = x && y;
    tab.grow(sizeof(double) * 2 * HO_MAX_TABLE, "elevation tables");
    out.grow(sizeof(tm_ho_quality), "elevation record");
    if (want_planes) planes.grow(sizeof(double) * 2 * n, "elevated planes");
    pairs.grow(sizeof(double2) * elements, "element pairs");
    partials.grow(sizeof(HoAcc) * (nwg + RECORDS_REDUCE_GROUPS), "elevation records");   // + the second stage's
    HIPCHK(hipMemcpyAsync(tab.p, pl.tab, sizeof(double) * 2 * (p + 1) * (p + 1), hipMemcpyHostToDevice, st));
    double* dx = want_planes ? planes.as<double>() : nullptr;
    double* dy = want_planes ? planes.as<double>() + n : nullptr;
    const int identity = pl.identity ? 1 : 0;
    dispatch_int<1, 8>(p, [&](auto P) {
        hipLaunchKernelGGL(k_ho_elevate<P()>, grid, dim3(HO_THREADS), 0, st, X, ni, nj, Ei, Ej, tab.as<double>(), identity, dx, dy, pairs.as<double2>(),
                           partials.as<HoAcc>());
    });
    HIPCHK(hipGetLastError());
    const Records<HoAcc> rec_in = records_first_stage(partials.as<HoAcc>(), nwg, st, ho_reduce_launch);   // at most RECORDS_REDUCE_GROUPS records are left for the finalize
    hipLaunchKernelGGL(k_ho_finalize, dim3(1), dim3(64), 0, st, rec_in.p, rec_in.n, static_cast<unsigned long long>(block), Ei, Ej, p, out.as<tm_ho_quality>());
    HIPCHK(hipGetLastError());
    tm_ho_quality rec;
    std::vector<double> jj(sj ? 2 * elements : 0);
    HIPCHK(hipMemcpyAsync(&rec, out.p, sizeof(rec), hipMemcpyDeviceToHost, st));
    if (want_planes) {
        HIPCHK(hipMemcpyAsync(x, dx, sizeof(double) * n, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(y, dy, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    }
    if (sj) HIPCHK(hipMemcpyAsync(jj.data(), pairs.p, sizeof(double2) * elements, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (sj) ho_sj_from_pairs(jj.data(), elements, rec.orientation, sj);
    if (q) *q = rec;
}

// ------------------------------------------------------------------ handle: the coordinates resident in X
void Smoother::elevate_host(const tm_ho_opt* opt, int64_t block, double* x, double* y, tm_ho_quality* q, double* sj) {
    const HoPlan pl = ho_plan(opt);
    const auto it = std::lower_bound(lp.owned_blocks.begin(), lp.owned_blocks.end(), block);
    if (block < 0 || it == lp.owned_blocks.end() || *it != block) throw TmError(TM_E_ARG, "block is not owned by this rank");
    ho_check_block(pl, static_cast<uint64_t>(block), static_cast<uint64_t>(topo.ni[block]), static_cast<uint64_t>(topo.nj[block]));
    if (!hodev) hodev = new HoDev();
    hodev->run(pl, X + lp.local_start[it - lp.owned_blocks.begin()], static_cast<int>(topo.ni[block]), static_cast<int>(topo.nj[block]), static_cast<uint64_t>(block), stream, x, y,
               q, sj);
}

}  // namespace tmh

using namespace tmh;

extern "C" int tm_ho_elevate(const tm_mesh_desc* mesh, const tm_ho_opt* opt, uint64_t block, double* x, double* y, tm_ho_quality* q, double* sj) {
    return guarded([&]() {
        if ((x == nullptr) != (y == nullptr)) throw TmError(TM_E_ARG, "x and y come together");
        const HoPlan pl = ho_plan(opt);
        const tm_block& b = ho_block_of(mesh, pl, block);
        require_gfx950();
        const size_t n = static_cast<size_t>(b.ni) * b.nj;
        DevBuf in(sizeof(double2) * n, "block to elevate");
        HIPCHK(hipMemcpy(in.p, b.xy, sizeof(double2) * n, hipMemcpyHostToDevice));
        HoDev dev;
        dev.run(pl, in.as<double2>(), static_cast<int>(b.ni), static_cast<int>(b.nj), block, nullptr, x, y, q, sj);
        return TM_OK;
    });
}

extern "C" int tm_smoother_elevate(tm_smoother* s, const tm_ho_opt* opt, uint64_t block, double* x, double* y, tm_ho_quality* q, double* sj) {
    return guarded([&]() {
        if (!s || !smoother_is_live(s)) throw TmError(TM_E_ARG, "not a live handle");
        if ((x == nullptr) != (y == nullptr)) throw TmError(TM_E_ARG, "x and y come together");
        if (block >= static_cast<uint64_t>(s->impl.topo.nblocks())) throw TmError(TM_E_ARG, "block index past the mesh");
        s->impl.elevate_host(opt, static_cast<int64_t>(block), x, y, q, sj);
        return TM_OK;
    });
}
