// K14 high-order certificate: Bernstein coefficients of the Jacobian of every element of a block, judged and subdivided on the device.
//     gfx950, wave64.  Definitions: include/tm_hip.h, "high-order elements: certificate"; every rounded expression and the decision are
//     tm_highorder_cert.hpp, shared with the host loop, so device and host agree bit for bit.
//
// Layout.  A workgroup is ONE wave, so its barriers cost no more than the LDS wait they imply and its control flow is the wave's.  The
// wave is cut into groups of GS = 4 / 16 / 64 lanes (p = 1 / 2 / 3..8), one element per group: 16, 4 or 1 elements per wave; the lanes
// of a group own the (2p)^2 output coefficients, c = lane + r*GS (one per lane up to p = 4, two at p = 5, three at p = 6, four at
// p = 7, 8).  A workgroup takes HC_ROUNDS consecutive rounds of elements, in the order e*Ej + f: the elements of a round are neighbours
// along j, where the rows of the block are contiguous.
//
// Element.  The (p+1)^2 source nodes go to LDS minus the element's first corner; W = d M^T and C = M W are formed there, one entry per
// lane and step, with the rows of M from the tables staged in LDS once per workgroup; the four difference arrays follow, their largest
// magnitudes meet by shuffles (the guard), and every lane sums its coefficients of B (hc_coeff) into the level-0 patch.
//
// Decision.  The quadtree of an element is walked depth first with one patch per level in LDS (5 (2p)^2 doubles per element): child q of
// the patch of level L-1 is formed in place by de Casteljau, 2p-1 steps along k then along l, every lane averaging its coefficient with
// its neighbour's.  The walk is the wave's: all groups follow the same path, a group whose patch on that path is not undecided idles, and
// a subtree that no group wants is skipped.  The extremes of a patch meet by shuffles inside the group; what the levels have shown
// (hc_visit) gives the breadth-first verdict at the end (hc_decide).  No floating-point atomics and no sums: nothing depends on order.
//
// Records.  One HcAcc per workgroup; k_hc_finalize (behind k_hc_reduce from 257 workgroups on) combines them, the scheme of K13.
#include "tm_highorder_cert_dev.hpp"
#include "tm_stack_dev.hpp"
#include "tm_dispatch.hpp"

#include <algorithm>

namespace tmh {

constexpr int HC_ROUNDS = 8;
constexpr int hc_group(int p) { return p == 1 ? 4 : p == 2 ? 16 : 64; }

template <int GS>
__device__ __forceinline__ double hc_group_min(double v) {
#pragma unroll
    for (int off = GS / 2; off > 0; off >>= 1) {
        const double w = __shfl_xor(v, off, 64);
        if (w < v) v = w;
    }
    return v;
}
template <int GS>
__device__ __forceinline__ double hc_group_max(double v) {
#pragma unroll
    for (int off = GS / 2; off > 0; off >>= 1) {
        const double w = __shfl_xor(v, off, 64);
        if (w > v) v = w;
    }
    return v;
}
template <int GS>
__device__ __forceinline__ int hc_group_or(int v) {
#pragma unroll
    for (int off = GS / 2; off > 0; off >>= 1) v |= __shfl_xor(v, off, 64);
    return v;
}

template <int P>
__global__ __launch_bounds__(64) void k_ho_certify(const double2* __restrict__ X, int nj, int Ei, int Ej, const double* __restrict__ tab, double G,
                                                   const double2* __restrict__ pairs, int orientation, int max_depth, unsigned char* __restrict__ status,
                                                   double2* __restrict__ bounds, HcAcc* __restrict__ partials) {
    constexpr int N1 = P + 1, N = 2 * P, NC = N * N, NN = N1 * N1, ND = P * N1;
    constexpr int GS = hc_group(P), EPW = 64 / GS, CPL = (NC + GS - 1) / GS;
    constexpr int NTAB = NN + N * P + N * N1;
    __shared__ double sTab[NTAB];
    __shared__ double sD[EPW][2][NN];      // shifted nodes, then the control points
    __shared__ double sW[EPW][2][NN];
    __shared__ double sDer[EPW][4][ND];    // xu, yu, xv, yv
    __shared__ double sPatch[EPW][HC_LEVELS][NC];
    __shared__ double sStat[EPW][4 * HC_LEVELS];
    __shared__ HcAcc sAcc[EPW];
    const int lane = threadIdx.x, grp = lane / GS, gl = lane % GS;
    for (int t = lane; t < NTAB; t += 64) sTab[t] = tab[t];
    const double* M = sTab;
    const double* WU = sTab + NN;
    const double* WV = WU + N * P;
    const double o = orientation >= 0 ? 1.0 : -1.0;
    const long long nel = static_cast<long long>(Ei) * Ej;
    const double inf = std::numeric_limits<double>::infinity();
    HcAcc acc;
    hc_init(acc);
    __syncthreads();

#pragma unroll 1
    for (int round = 0; round < HC_ROUNDS; ++round) {
        const long long first = (static_cast<long long>(blockIdx.x) * HC_ROUNDS + round) * EPW;
        if (first >= nel) break;   // the wave's
        const long long el = first + grp;
        const bool have = el < nel;
        const int e = have ? static_cast<int>(el / Ej) : 0, f = have ? static_cast<int>(el % Ej) : 0;
        const size_t out = static_cast<size_t>(f) * Ei + e;
        double* d0 = sD[grp][0];
        double* d1 = sD[grp][1];
        double* w0 = sW[grp][0];
        double* w1 = sW[grp][1];
        double* xu = sDer[grp][0];
        double* yu = sDer[grp][1];
        double* xv = sDer[grp][2];
        double* yv = sDer[grp][3];
        double* stat = sStat[grp];
        bool nodal_valid = false;
        if (have) {
            const double2* base = X + static_cast<size_t>(e) * P * nj + static_cast<size_t>(f) * P;   // node (e*P + P, f*P + P) is inside the block
            const double2 b0 = base[0];
            for (int c = gl; c < NN; c += GS) {
                const int m = c / N1, n = c - m * N1;
                const double2 v = base[static_cast<size_t>(m) * nj + n];
                d0[c] = v.x - b0.x;
                d1[c] = v.y - b0.y;
            }
            const double2 pr = pairs[out];
            nodal_valid = hc_nodal_valid(pr.x, pr.y, orientation);
            if (gl == 0) hc_stat_init(stat);
        }
        __syncthreads();
        if (have)
            for (int c = gl; c < NN; c += GS) {
                const int m = c / N1, j = c - m * N1;
                w0[c] = hc_dot(M + j * N1, d0 + m * N1, 1, N1);
                w1[c] = hc_dot(M + j * N1, d1 + m * N1, 1, N1);
            }
        __syncthreads();
        if (have)
            for (int c = gl; c < NN; c += GS) {
                const int i = c / N1, j = c - i * N1;
                d0[c] = hc_dot(M + i * N1, w0 + j, N1, N1);
                d1[c] = hc_dot(M + i * N1, w1 + j, N1, N1);
            }
        __syncthreads();
        double mxu = 0.0, myu = 0.0, mxv = 0.0, myv = 0.0;
        if (have)
            for (int c = gl; c < ND; c += GS) {
                {
                    const int i = c / N1, j = c - i * N1;   // xu, yu: P x (P+1)
                    const double a = d0[(i + 1) * N1 + j] - d0[i * N1 + j], b = d1[(i + 1) * N1 + j] - d1[i * N1 + j];
                    xu[c] = a;
                    yu[c] = b;
                    if (fabs(a) > mxu) mxu = fabs(a);
                    if (fabs(b) > myu) myu = fabs(b);
                }
                {
                    const int i = c / P, j = c - i * P;     // xv, yv: (P+1) x P
                    const double a = d0[i * N1 + j + 1] - d0[i * N1 + j], b = d1[i * N1 + j + 1] - d1[i * N1 + j];
                    xv[c] = a;
                    yv[c] = b;
                    if (fabs(a) > mxv) mxv = fabs(a);
                    if (fabs(b) > myv) myv = fabs(b);
                }
            }
        mxu = hc_group_max<GS>(mxu);
        myu = hc_group_max<GS>(myu);
        mxv = hc_group_max<GS>(mxv);
        myv = hc_group_max<GS>(myv);
        const double g = hc_guard(G, mxu, myu, mxv, myv);
        __syncthreads();
        if (have)
#pragma unroll
            for (int r = 0; r < CPL; ++r) {
                const int c = gl + r * GS;
                if (c < NC) sPatch[grp][0][c] = hc_coeff(P, c / N, c % N, xu, yu, xv, yv, WU, WV);
            }
        __syncthreads();

        // ---- the walk.  path: two bits per level, the child taken at levels 1 .. L; live: bit L set iff this group's patch of level L
        // on the path is undecided and its children are wanted
        unsigned inv = 0, und = 0, live = 0, path = 0;
        auto judge = [&](int L, bool mine) {
            const double* s = sPatch[grp][L];
            double mn = inf, mx = -inf;
            int bad = (L == 0 && !nodal_valid) ? 1 : 0;
            if (mine) {
#pragma unroll
                for (int r = 0; r < CPL; ++r) {
                    const int c = gl + r * GS;
                    if (c < NC) {
                        const double v = o * s[c];
                        const int k = c / N, l = c - k * N;
                        if (!__builtin_isfinite(v)) bad = 1;
                        if ((k == 0 || k == N - 1) && (l == 0 || l == N - 1) && !(v > 0.0)) bad = 1;
                        if (v < mn) mn = v;
                        if (v > mx) mx = v;
                    }
                }
            }
            mn = hc_group_min<GS>(mn);
            mx = hc_group_max<GS>(mx);
            bad = hc_group_or<GS>(bad);
            live &= ~(1u << L);
            if (mine && hc_visit(L, mn, mx, bad != 0, g, gl == 0, stat, inv, und) && hc_descend(L, max_depth, inv)) live |= 1u << L;
        };
        judge(0, have);
        int L = 0;
        bool descend = true;   // the patch of level L has just been judged: its children come next if anybody wants them
        while (true) {
            if (descend && L < max_depth && __ballot((live >> L) & 1u) != 0ull) {
                ++L;
                path &= ~(3u << (2 * L));
            } else {   // next sibling, or up
                while (L > 0 && ((path >> (2 * L)) & 3u) == 3u) --L;
                if (L == 0) break;
                path += 1u << (2 * L);
            }
            // child q of the patch of level L-1 into level L; a verdict since the parent was judged may have made it pointless
            const unsigned q = (path >> (2 * L)) & 3u;
            const bool want = have && ((live >> (L - 1)) & 1u) && hc_descend(L - 1, max_depth, inv);
            if (__ballot(want) == 0ull) {
                path |= 3u << (2 * L);
                descend = false;
                continue;
            }
            double* s = sPatch[grp][L];
            const double* parent = sPatch[grp][L - 1];
            if (want)
#pragma unroll
                for (int r = 0; r < CPL; ++r) {
                    const int c = gl + r * GS;
                    if (c < NC) s[c] = parent[c];
                }
            __syncthreads();
#pragma unroll 1
            for (int dir = 0; dir < 2; ++dir) {
                const int step = dir == 0 ? N : 1;            // along k, then along l
                const bool upper = dir == 0 ? (q >> 1) != 0 : (q & 1u) != 0;
#pragma unroll 1
                for (int r = 1; r < N; ++r) {
                    double nv[CPL];
                    bool upd[CPL];
#pragma unroll
                    for (int t = 0; t < CPL; ++t) {
                        const int c = gl + t * GS;
                        const int k = c / N, l = c - k * N, x = dir == 0 ? k : l;
                        upd[t] = want && c < NC && (upper ? x <= N - 1 - r : x >= r);
                        nv[t] = 0.0;
                        if (upd[t]) nv[t] = upper ? hc_mid(s[c], s[c + step]) : hc_mid(s[c - step], s[c]);
                    }
                    __syncthreads();
#pragma unroll
                    for (int t = 0; t < CPL; ++t)
                        if (upd[t]) s[gl + t * GS] = nv[t];
                    __syncthreads();
                }
            }
            judge(L, want);
            descend = true;
        }
        __syncthreads();
        if (have && gl == 0) {
            const HcElement r = hc_decide(stat, inv, und, max_depth, g);
            hc_count_element(r, nodal_valid, static_cast<unsigned long long>(el), acc);
            if (status) status[out] = static_cast<unsigned char>(r.status);
            if (bounds) bounds[out] = double2{r.lo, r.hi};
        }
        __syncthreads();
    }
    if (gl == 0) sAcc[grp] = acc;
    __syncthreads();
    if (lane == 0) {
        HcAcc t = sAcc[0];
#pragma unroll 1
        for (int k = 1; k < EPW; ++k) hc_combine(t, sAcc[k]);
        partials[blockIdx.x] = t;
    }
}

// the records are combined in K13's fixed order (the fields are counts and minima, so the order does not reach the result)
__global__ __launch_bounds__(64) void k_hc_reduce(const HcAcc* __restrict__ partials, int nwg, int chunk, HcAcc* __restrict__ out) {
    __shared__ HcAcc sh[64];
    const int begin = static_cast<int>(blockIdx.x) * chunk, end = begin + chunk < nwg ? begin + chunk : nwg;
    records_reduce_wave<HcAcc, hc_init, hc_combine>(partials, begin, end, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = sh[0];
}
__global__ __launch_bounds__(64) void k_hc_finalize(const HcAcc* __restrict__ partials, int nwg, unsigned long long block, int Ei, int Ej, int order, int orientation,
                                                    int max_depth, tm_ho_certificate* __restrict__ out) {
    __shared__ HcAcc sh[64];
    records_reduce_wave<HcAcc, hc_init, hc_combine>(partials, 0, nwg, sh);
    if (threadIdx.x == 0) hc_finish(sh[0], block, static_cast<uint64_t>(Ei), static_cast<uint64_t>(Ej), order, orientation, max_depth, out);
}

// ------------------------------------------------------------------ host driver
void hc_reduce_launch(const HcAcc* partials, int nrec, int chunk, int groups, HcAcc* out, hipStream_t st) {
    hipLaunchKernelGGL(k_hc_reduce, dim3(groups), dim3(64), 0, st, partials, nrec, chunk, out);
}

int hc_workgroups(int p, uint64_t elements) {
    const uint64_t per = static_cast<uint64_t>(HC_ROUNDS) * (64 / hc_group(p));
    return static_cast<int>((elements + per - 1) / per);
}

void HcDev::run(HoDev& ho, const HoPlan& hopl, const double2* X, int ni, int nj, uint64_t block, hipStream_t st, int max_depth,
                tm_ho_certificate* cert, uint8_t* h_status, double* h_bounds) {
    const int p = hopl.order, Ei = (ni - 1) / p, Ej = (nj - 1) / p;
    const size_t elements = static_cast<size_t>(Ei) * Ej;
    tm_ho_quality rec;
    ho.run(hopl, X, ni, nj, block, st, nullptr, nullptr, &rec, nullptr);   // K13's report: the orientation, and the nodal pairs stay in ho.pairs
    const int nwg = hc_workgroups(p, elements);
    tab.grow(sizeof(double) * HC_MAX_TAB, "certificate tables");
    out.grow(sizeof(tm_ho_certificate), "certificate record");
    status.grow(elements, "element status");
    bounds.grow(sizeof(double2) * elements, "element bounds");
    partials.grow(sizeof(HcAcc) * (static_cast<size_t>(nwg) + RECORDS_REDUCE_GROUPS), "certificate records");
    if (plan.order != p) {   // a call always waits for its stream at the end, so no earlier launch still reads the old tables
        plan = hc_plan(p);
        const hipError_t up = hipMemcpyAsync(tab.p, plan.tab, sizeof(double) * plan.tab_size(), hipMemcpyHostToDevice, st);
        if (up != hipSuccess) plan.order = 0;
        HIPCHK(up);
    }
    const int o = rec.orientation;
    dispatch_int<1, 8>(p, [&](auto P) {
        hipLaunchKernelGGL(k_ho_certify<P()>, dim3(static_cast<unsigned>(nwg)), dim3(64), 0, st, X, nj, Ei, Ej, tab.as<double>(), plan.G, ho.pairs.as<double2>(), o,
                           max_depth, status.as<unsigned char>(), bounds.as<double2>(), partials.as<HcAcc>());
    });
    HIPCHK(hipGetLastError());
    const Records<HcAcc> rec_in = records_first_stage(partials.as<HcAcc>(), static_cast<size_t>(nwg), st, hc_reduce_launch);
    hipLaunchKernelGGL(k_hc_finalize, dim3(1), dim3(64), 0, st, rec_in.p, rec_in.n, static_cast<unsigned long long>(block), Ei, Ej, p, o, max_depth,
                       out.as<tm_ho_certificate>());
    HIPCHK(hipGetLastError());
    tm_ho_certificate c;
    HIPCHK(hipMemcpyAsync(&c, out.p, sizeof(c), hipMemcpyDeviceToHost, st));
    if (h_status) HIPCHK(hipMemcpyAsync(h_status, status.p, elements, hipMemcpyDeviceToHost, st));
    if (h_bounds) HIPCHK(hipMemcpyAsync(h_bounds, bounds.p, sizeof(double2) * elements, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (cert) *cert = c;
}

// ------------------------------------------------------------------ handle: the coordinates resident in X
void Smoother::certify_host(const tm_ho_opt* opt, int max_depth, int64_t block, tm_ho_certificate* cert, uint8_t* status, double* bounds) {
    const HoPlan pl = ho_plan(opt);
    hc_check_depth(max_depth);
    const auto it = std::lower_bound(lp.owned_blocks.begin(), lp.owned_blocks.end(), block);
    if (block < 0 || it == lp.owned_blocks.end() || *it != block) throw TmError(TM_E_ARG, "block is not owned by this rank");
    ho_check_block(pl, static_cast<uint64_t>(block), static_cast<uint64_t>(topo.ni[block]), static_cast<uint64_t>(topo.nj[block]));
    if (!hodev) hodev = new HoDev();
    if (!hcdev) hcdev = new HcDev();
    hcdev->run(*hodev, pl, X + lp.local_start[it - lp.owned_blocks.begin()], static_cast<int>(topo.ni[block]), static_cast<int>(topo.nj[block]),
               static_cast<uint64_t>(block), stream, max_depth, cert, status, bounds);
}

}  // namespace tmh

using namespace tmh;

extern "C" int tm_ho_certify(const tm_mesh_desc* mesh, const tm_ho_opt* opt, int32_t max_depth, uint64_t block, tm_ho_certificate* cert, uint8_t* status,
                             double* bounds) {
    return guarded([&]() {
        const HoPlan pl = ho_plan(opt);
        hc_check_depth(max_depth);
        const tm_block& b = ho_block_of(mesh, pl, block);
        require_gfx950();
        const size_t n = static_cast<size_t>(b.ni) * b.nj;
        DevBuf in(sizeof(double2) * n, "block to certify");
        HIPCHK(hipMemcpy(in.p, b.xy, sizeof(double2) * n, hipMemcpyHostToDevice));
        HoDev ho;
        HcDev dev;
        dev.run(ho, pl, in.as<double2>(), static_cast<int>(b.ni), static_cast<int>(b.nj), block, nullptr, max_depth, cert, status, bounds);
        return TM_OK;
    });
}

extern "C" int tm_smoother_certify(tm_smoother* s, const tm_ho_opt* opt, int32_t max_depth, uint64_t block, tm_ho_certificate* cert, uint8_t* status,
                                   double* bounds) {
    return guarded([&]() {
        if (!s || !smoother_is_live(s)) throw TmError(TM_E_ARG, "not a live handle");
        if (block >= static_cast<uint64_t>(s->impl.topo.nblocks())) throw TmError(TM_E_ARG, "block index past the mesh");
        s->impl.certify_host(opt, max_depth, static_cast<int64_t>(block), cert, status, bounds);
        return TM_OK;
    });
}
