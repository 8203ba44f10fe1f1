// K16  stack_elevate: K smoothed 2-D cuts of one block -> curved hexahedra of order p (include/tm_hip.h, "high-order hexahedra of
//      stacked blocks") in one pass over the cuts: the elevated node layers and the element records, without the fine 3-D block ever
//      being stored.  gfx950, wave64.  The fine nodes are formed with K11's expression (tm_stack.hip, restated here as K12 restates it;
//      the tests hold the two equal bit for bit), every line of the three contraction stages is tm_highorder3.hpp's ho3_line, shared
//      with the host loops.
//
// Tile.  A workgroup of 256 threads owns EI x EJ whole elements in-plane: 16 x 14 at p = 1, 8 x 7 at p = 2, 5 x 5 at p = 3, 4 x 3 at
// p = 4, that is 17 x 15, 17 x 15, 16 x 16 and 17 x 13 nodes (255, 255, 256, 221 of the 256 threads hold a node; the nodes on tile seams
// are held by both neighbours).  The K cut values of a node are loaded once -- lanes along j, 16 B per lane, all K loads in flight --
// pass through LDS like K11's and come back with the lanes along i, and stay in registers under compile-time indices for the whole
// march.  K15's surface stage runs as the cuts pass, as in K11.
//
// March.  The workgroup walks over the span elements g.  Per element every node thread forms its p new fine nodes (the first is the
// last of the element below, carried in registers), the weight row of a layer read under a wave-uniform index.  Then, for each target
// plane c = 0 .. p of the element:
//   stage 1  the node thread contracts ITS p+1 fine nodes along span with rows c of T and D (one LDS address per wave: a broadcast read;
//            scalar loads of the rows cost SGPRs the march does not have): six values per node
//            -- V of (T, D) x (x, y, z) -- to LDS.  The fine nodes never leave the registers of the thread that formed them.
//   stage 2  one lane per (source row m, target column (f, b)): nine W lines -- (T on Vt), (D on Vt), (T on Vd), three components --
//            lanes along i, so the LDS reads of a wave are consecutive; results to LDS.
//   stage 3  one lane per target node (e, a, f, b) of the plane: twelve R lines -- Y, d/du, d/dv, d/dw -- the determinant, and the
//            lane's running extremes of J for its element (kept in registers across the planes).  Elevated nodes are stored from here,
//            lanes along i.
// Two barriers per plane.  With TM_HO_EQUIDISTANT or p = 1 the node threads store their fine nodes themselves (lanes along i) and Y is
// not formed.  After the planes the lanes' extremes meet in LDS, one lane per element combines them, evaluates the corner hexahedron
// (the corner layers of the tile are in LDS for that), counts the element (ho_count_element) and writes its (Jmin, Jmax) pair.
//
// LDS (doubles): 6*256 V, max(9 * stage-2 lanes, ...) W (the load tiles and the element extremes alias it), 6*256 corner layers, the
// tables.  All pitches equal the tile's node count along i, so consecutive lanes read consecutive doubles and a 32-lane group of
// ds_read_b64 covers the 64 banks once; where a group of lanes spans two element rows f the rows lie p * 17 doubles apart and a few
// lanes meet 2-way.  Table entries are read by at most p+1 distinct addresses per wave (broadcast).
//
// Records: in-lane over the march, in-wave by shuffles, across the waves through LDS, one HoAcc per workgroup, the histogram by integer
// LDS atomics; k_ho3_finalize (behind K13's k_ho_reduce from 257 workgroups on) combines them in fixed order and picks the orientation's
// candidate set (ho3_finish).  No floating-point atomics.  `outside` as in K11: ballots, LDS counters, one integer atomic per workgroup
// and cut; a seam node is counted by the tile that owns it.
//
// Instantiations: P x K x MAP = 4 x 15 x 3.  K and MAP must be compile-time (the cut values are register arrays), P as well (the fine
// nodes and the lines are); the four orders are compiled in four translation units (tm_highorder3_p1.hip ..) so that the build takes
// them in parallel.  Compiler's resource usage: DESIGN.md section 4, K16.
#include "tm_highorder3_dev.hpp"
#include "tm_dispatch.hpp"

namespace tmh {

__device__ __forceinline__ unsigned long long ho3_shfl(unsigned long long v, int off) { return __shfl_down(v, off, 64); }

// table: per layer K weights followed by s[k] (row pitch K + 1), all layers.  Span elements [g0, g1) are marched; X, Y, Z (null: no
// planes) receive the node layers of the window [gs0, gs0 + gsn) of span elements, layer (g - gs0)*P + c at ((g - gs0)*P + c)*ni*nj.
// pairs: (Jmin, Jmax) per element (g*Ej + f)*Ei + e, NaN pairs where a J is not finite, or null.  partials: one record per workgroup, or null.
template <int P, int K, int MAP>
__global__ __launch_bounds__(HO3_THREADS) void k_stack_elevate(StackCuts cuts, StackSurf surf, const double* __restrict__ table, int ni, int nj, int Ei, int Ej, int g0,
                                                               int g1, int gs0, int gsn, const double* __restrict__ tab, int identity, double* __restrict__ X,
                                                               double* __restrict__ Y, double* __restrict__ Z, double2* __restrict__ pairs,
                                                               HoAcc* __restrict__ partials, unsigned long long* __restrict__ outside) {
    constexpr bool REV = MAP == TM_STACK_REVOLUTION;
    constexpr int N = P + 1, EI = ho3_tile_ei(P), EJ = ho3_tile_ej(P), TNI = EI * P + 1, TNJ = EJ * P + 1, NN = TNI * TNJ;
    constexpr int S2 = TNI * EJ * N;       // stage-2 lanes: (m, f, b), m fastest
    constexpr int RI = EI * N, S3 = RI * EJ * N;   // stage-3 lanes: (e, a, f, b), (e, a) fastest
    constexpr int NIT = (S3 + HO3_THREADS - 1) / HO3_THREADS;
    constexpr int SW_SIZE = 9 * S2 > 2 * S3 ? (9 * S2 > 4 * HO3_THREADS ? 9 * S2 : 4 * HO3_THREADS) : (2 * S3 > 4 * HO3_THREADS ? 2 * S3 : 4 * HO3_THREADS);
    static_assert(NN <= HO3_THREADS && EI * EJ <= HO3_THREADS, "one thread per node, one per element");
    static_assert(TM_STACK_MAX_KNOTS <= HO3_THREADS, "one thread stages one knot");
    __shared__ __align__(16) double sV[6 * HO3_THREADS];
    __shared__ __align__(16) double sW[SW_SIZE];
    __shared__ double sF[2 * 3 * HO3_THREADS];   // fine layers 0 and P of the current span element
    __shared__ double sTab[2 * N * N];
    __shared__ double sh_u[REV ? 2 : 1][REV ? TM_STACK_MAX_KNOTS : 1];
    __shared__ unsigned sh_out[REV ? K : 1];
    __shared__ unsigned sh_hist[20];
    __shared__ HoAcc sh_acc[HO3_WAVES];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int e0 = static_cast<int>(blockIdx.y) * EI, f0 = static_cast<int>(blockIdx.x) * EJ;
    const int eli = Ei - e0 < EI ? Ei - e0 : EI, elj = Ej - f0 < EJ ? Ej - f0 : EJ;   // elements of the tile that exist (>= 1 by the grid)
    const int tni = eli * P + 1;                                                       // its node rows along i: i0 + tni <= ni
    const int i0 = e0 * P, j0 = f0 * P;
    const bool last_i = e0 + eli == Ei, last_j = f0 + elj == Ej;
    if (t < 20) sh_hist[t] = 0;
    if (t < 2 * N * N) sTab[t] = tab[t];
    if (REV && t < K) sh_out[t] = 0;   // the three are ordered before their first use by the first cut's barrier

    // ---- the K cut values of the node: loaded with the lanes along j, turned in LDS (two tiles alternating, one barrier per cut)
    const bool node = t < NN;
    const int ti = node ? t % TNI : 0, tj = node ? t / TNI : 0;
    const int i = i0 + ti < ni ? i0 + ti : ni - 1, j = j0 + tj < nj ? j0 + tj : nj - 1;   // lanes past the block repeat its last row / column
    const bool own = node && i0 + ti < ni && j0 + tj < nj && (ti < TNI - 1 || i0 + ti == ni - 1) && (tj < TNJ - 1 || j0 + tj == nj - 1);
    double2 v[K];
    double rc[REV ? K : 1];
    {
        const int li = node ? t / TNJ : 0, lj = node ? t % TNJ : 0;
        const int il = i0 + li < ni ? i0 + li : ni - 1, jl = j0 + lj < nj ? j0 + lj : nj - 1;
        const size_t o = static_cast<size_t>(il) * nj + jl;
#pragma unroll
        for (int c = 0; c < K; ++c) v[c] = cuts.xy[c][o];
    }
    double2* tile = reinterpret_cast<double2*>(sW);   // [2][HO3_THREADS]
#pragma unroll
    for (int c = 0; c < K; ++c) {
        tile[(c & 1) * HO3_THREADS + t] = v[c];
        if (REV) stack_surf_stage(sh_u[c & 1], surf, c, t);
        __syncthreads();   // a tile is written again two cuts later: every thread has passed the next barrier, i.e. read it, by then
        v[c] = tile[(c & 1) * HO3_THREADS + ti * TNJ + tj];
        if (REV) {
            double xs, rs;
            const bool out = stack_surf_node(sh_u[c & 1], surf, c, v[c].x, &xs, &rs);
            v[c].x = xs;
            rc[c] = rs;
            v[c].y = v[c].y / cuts.radius[c];
            if (outside) {
                const unsigned long long m = __ballot(out && own);
                if (lane == 0 && m) atomicAdd(&sh_out[c], static_cast<unsigned>(__popcll(m)));
            }
        }
    }
    if (MAP == TM_STACK_CYLINDRICAL) {
#pragma unroll
        for (int c = 0; c < K; ++c) v[c].y = v[c].y / cuts.radius[c];
    }
    __syncthreads();   // the tiles alias sW; sh_out is complete
    if (REV && outside && t < K && sh_out[t]) atomicAdd(&outside[t], static_cast<unsigned long long>(sh_out[t]));

    // K11's expression for layer k, operation for operation
    auto fine = [&](int k) {
        const double* __restrict__ w = table + static_cast<size_t>(k) * (K + 1);   // wave-uniform
        double ax = w[0] * v[0].x, ay = w[0] * v[0].y, ar = REV ? w[0] * rc[0] : 0.0;
#pragma unroll
        for (int c = 1; c < K; ++c) {
            ax = ax + w[c] * v[c].x;
            ay = ay + w[c] * v[c].y;
            if (REV) ar = ar + w[c] * rc[c];
        }
        const double s = REV ? ar : w[K];
        Q3Point r;
        r.x = ax;
        if (MAP == TM_STACK_CYLINDRICAL || REV) {
            double sn, cs;
            sincos(ay, &sn, &cs);
            r.y = s * sn;
            r.z = s * cs;
        } else {
            r.y = ay;
            r.z = s;
        }
        return r;
    };

    const size_t plane = static_cast<size_t>(ni) * nj;
    const size_t onode = static_cast<size_t>(j) * ni + i;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const double* __restrict__ sT = sTab;
    const double* __restrict__ sD = sTab + N * N;
    HoAcc acc;
    ho_init(acc);
    Q3Point F[N];
    F[0] = Q3Point{0.0, 0.0, 0.0};

    for (int g = g0; g < g1; ++g) {
        const bool store = X != nullptr && g >= gs0 && g < gs0 + gsn;
        const int gs = g - gs0;
        if (g == g0) F[0] = fine(g * P);
#pragma unroll
        for (int l = 1; l < N; ++l) F[l] = fine(g * P + l);
        if (store && identity && own) {
#pragma unroll
            for (int l = 0; l < N; ++l)
                if (ho_owns(l, P, gs, gsn)) {
                    const size_t o = (static_cast<size_t>(gs) * P + l) * plane + onode;
                    X[o] = F[l].x;
                    Y[o] = F[l].y;
                    Z[o] = F[l].z;
                }
        }
        if (node) {   // the corner layers, for the element lanes at the end of this span element (the barrier that ends it orders the reuse)
            sF[0 * HO3_THREADS + t] = F[0].x;
            sF[1 * HO3_THREADS + t] = F[0].y;
            sF[2 * HO3_THREADS + t] = F[0].z;
            sF[3 * HO3_THREADS + t] = F[P].x;
            sF[4 * HO3_THREADS + t] = F[P].y;
            sF[5 * HO3_THREADS + t] = F[P].z;
        }
        const bool want_y = store && !identity;
        Ho3Ext ext[NIT];
#pragma unroll
        for (int it = 0; it < NIT; ++it) ho3_ext_init(ext[it]);

#pragma unroll 1
        for (int c = 0; c < N; ++c) {
            // stage 1: span.  sV was last read by stage 2 of the plane before, which every thread left through that plane's second barrier
            if (node) {
                const double* __restrict__ Tc = sT + c * N;   // one address for the whole wave: a broadcast read
                const double* __restrict__ Dc = sD + c * N;
                sV[0 * HO3_THREADS + t] = ho3_line<P>(Tc, [&](int l) { return F[l].x; });
                sV[1 * HO3_THREADS + t] = ho3_line<P>(Tc, [&](int l) { return F[l].y; });
                sV[2 * HO3_THREADS + t] = ho3_line<P>(Tc, [&](int l) { return F[l].z; });
                sV[3 * HO3_THREADS + t] = ho3_line<P>(Dc, [&](int l) { return F[l].x; });
                sV[4 * HO3_THREADS + t] = ho3_line<P>(Dc, [&](int l) { return F[l].y; });
                sV[5 * HO3_THREADS + t] = ho3_line<P>(Dc, [&](int l) { return F[l].z; });
            }
            __syncthreads();
            // stage 2: along j.  sW was last read by stage 3 of the plane before: every thread has left it to arrive at the barrier above
            for (int idx = t; idx < S2; idx += HO3_THREADS) {
                const int m = idx % TNI, col = idx / TNI, f = col / N, b = col - f * N;
                if (m >= tni || f >= elj) continue;
                const double* __restrict__ Tb = sT + b * N;
                const double* __restrict__ Db = sD + b * N;
                const double* __restrict__ src = sV + (f * P) * TNI + m;
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    auto Vt = [&](int n) { return src[q * HO3_THREADS + n * TNI]; };
                    auto Vd = [&](int n) { return src[(3 + q) * HO3_THREADS + n * TNI]; };
                    sW[q * S2 + idx] = ho3_line<P>(Tb, Vt);
                    sW[(3 + q) * S2 + idx] = ho3_line<P>(Db, Vt);
                    sW[(6 + q) * S2 + idx] = ho3_line<P>(Tb, Vd);
                }
            }
            __syncthreads();
            // stage 3: along i, the determinant, the elevated node
            const bool own_c = ho_owns(c, P, gs, gsn);
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int idx = it * HO3_THREADS + t;
                if (idx >= S3) continue;
                const int ia = idx % RI, col = idx / RI, e = ia / N, a = ia - e * N, f = col / N, b = col - f * N;
                if (e >= eli || f >= elj) continue;
                const double* __restrict__ Ta = sT + a * N;
                const double* __restrict__ Da = sD + a * N;
                const double* __restrict__ src = sW + col * TNI + e * P;
                double r[3][4];
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    auto Wtt = [&](int m) { return src[q * S2 + m]; };
                    auto Wdt = [&](int m) { return src[(3 + q) * S2 + m]; };
                    auto Wtd = [&](int m) { return src[(6 + q) * S2 + m]; };
                    r[q][1] = ho3_line<P>(Da, Wtt);
                    r[q][2] = ho3_line<P>(Ta, Wdt);
                    r[q][3] = ho3_line<P>(Ta, Wtd);
                    r[q][0] = want_y ? ho3_line<P>(Ta, Wtt) : 0.0;
                }
                ho3_ext_take(ext[it], ho3_det(Q3Point{r[0][1], r[1][1], r[2][1]}, Q3Point{r[0][2], r[1][2], r[2][2]}, Q3Point{r[0][3], r[1][3], r[2][3]}));
                // a seam node is written by the element (and the tile) above it, the block's last node by the last element
                if (want_y && own_c && (a < P || (e == eli - 1 && last_i)) && (b < P || (f == elj - 1 && last_j))) {
                    const size_t o = (static_cast<size_t>(gs) * P + c) * plane + static_cast<size_t>(j0 + f * P + b) * ni + (i0 + e * P + a);
                    X[o] = r[0][0];
                    Y[o] = r[1][0];
                    Z[o] = r[2][0];
                }
            }
        }
        __syncthreads();   // stage 3 has read sW for the last time: the lanes' extremes take its place
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int idx = it * HO3_THREADS + t;
            if (idx < S3) {
                sW[idx] = ext[it].bad ? nan : ext[it].jmin;
                sW[S3 + idx] = ext[it].bad ? nan : ext[it].jmax;
            }
        }
        __syncthreads();
        if (t < EI * EJ) {
            const int e = t % EI, f = t / EI;
            if (e < eli && f < elj) {
                Ho3Ext x;
                ho3_ext_init(x);
#pragma unroll
                for (int b = 0; b < N; ++b)
#pragma unroll
                    for (int a = 0; a < N; ++a) {
                        const int idx = (f * N + b) * RI + e * N + a;
                        const double lo = sW[idx], hi = sW[S3 + idx];
                        ho3_ext_merge(x, Ho3Ext{lo, hi, lo != lo});
                    }
                Q3Point cx[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int n = (f * P + ((k >> 1) & 1) * P) * TNI + e * P + (k & 1) * P;
                    const double* s = sF + (k >> 2) * 3 * HO3_THREADS + n;
                    cx[k] = Q3Point{s[0], s[HO3_THREADS], s[2 * HO3_THREADS]};
                }
                const double vol = q3_volume(cx);
                const unsigned long long el = (static_cast<unsigned long long>(g) * Ej + (f0 + f)) * Ei + (e0 + e);
                if (partials) {
                    const int bin = ho_count_element(x.jmin, x.jmax, x.bad, vol, el, acc);
                    if (bin >= 0) atomicAdd(&sh_hist[bin], 1u);
                }
                if (pairs) pairs[el] = x.bad ? double2{nan, nan} : double2{x.jmin, x.jmax};
            }
        }
        __syncthreads();   // sF, sW and sV are free for the next span element
        F[0] = F[P];
    }
    if (!partials) return;

    // in-wave, fixed tree
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            acc.n[s] += ho3_shfl(acc.n[s], off);
            q_take_min(acc.sj[s], acc.at[s], __shfl_down(acc.sj[s], off, 64), ho3_shfl(acc.at[s], off));
            double u = __shfl_down(acc.lo[s], off, 64);
            if (u < acc.lo[s]) acc.lo[s] = u;
            u = __shfl_down(acc.hi[s], off, 64);
            if (u > acc.hi[s]) acc.hi[s] = u;
        }
        acc.asum += __shfl_down(acc.asum, off, 64);
        acc.aabs += __shfl_down(acc.aabs, off, 64);
    }
    if (lane == 0) sh_acc[wave] = acc;   // hist is zero in every lane: the bins are in sh_hist
    __syncthreads();
    if (t == 0) {
        HoAcc r = sh_acc[0];
        for (int w = 1; w < HO3_WAVES; ++w) ho_combine(r, sh_acc[w]);
        for (int k = 0; k < 20; ++k) r.hist[k / 10][k % 10] = sh_hist[k];
        partials[static_cast<size_t>(blockIdx.y) * gridDim.x + blockIdx.x] = r;
    }
}

template <int P, int K>
static void ho3_launch_k(const Ho3Launch& a, hipStream_t st) {
    const dim3 grid((a.Ej + ho3_tile_ej(P) - 1) / ho3_tile_ej(P), (a.Ei + ho3_tile_ei(P) - 1) / ho3_tile_ei(P)), block(HO3_THREADS);
#define TM_HO3_ARGS a.cuts, a.surf, a.table, a.ni, a.nj, a.Ei, a.Ej, a.g0, a.g1, a.gs0, a.gsn, a.tab, a.identity, a.X, a.Y, a.Z, a.pairs, a.partials, a.outside
    if (a.mapping == TM_STACK_REVOLUTION)
        hipLaunchKernelGGL((k_stack_elevate<P, K, TM_STACK_REVOLUTION>), grid, block, 0, st, TM_HO3_ARGS);
    else if (a.mapping == TM_STACK_CYLINDRICAL)
        hipLaunchKernelGGL((k_stack_elevate<P, K, TM_STACK_CYLINDRICAL>), grid, block, 0, st, TM_HO3_ARGS);
    else
        hipLaunchKernelGGL((k_stack_elevate<P, K, TM_STACK_PLANAR>), grid, block, 0, st, TM_HO3_ARGS);
#undef TM_HO3_ARGS
}

template <int P>
hipError_t ho3_launch(int K, const Ho3Launch& a, hipStream_t st) {
    if (K < 2 || K > TM_STACK_MAX_CUTS) return hipErrorInvalidValue;
    dispatch_int<2, TM_STACK_MAX_CUTS>(K, [&](auto k) { ho3_launch_k<P, k()>(a, st); });
    return hipGetLastError();
}

}  // namespace tmh
