// K17 certificate of high-order hexahedra: the (3p)^3 Bernstein coefficients of the Jacobian of every element of a stacked block, judged
//     and subdivided on the device.  gfx950, wave64.  Definitions: include/tm_hip.h, "high-order hexahedra: certificate"; every rounded
//     expression is tm_highorder3_cert.hpp, the decision tm_highorder_cert.hpp, both shared with the host loop, so device and host agree
//     bit for bit.
//
// Driver.  K17 is bound by fp64 arithmetic (of the order of 10^5 .. 10^6 operations per element at p = 4 against 3 * 125 doubles read), so
// it reads its nodes from memory: K16's report-only launch gives the orientation and the (Jmin, Jmax) pairs, then per window of span
// elements the existing K11 launch writes the fine planes -- bit for bit tm_stack_block's by construction -- and k_ho3_certify<P> runs on
// the window's elements.  The window is sized so that the planes stay within H3_WINDOW_BYTES (TM_HO3_CERT_WINDOW_BYTES overrides it: a
// knob for tests and measurements).
//
// Kernel.  One element per workgroup and round, 16 / 8 / 4 / 4 consecutive elements (e fastest) per workgroup at p = 1 .. 4; 64 threads at
// p = 1, 256 above.  Everything of an element lives in LDS: the shifted nodes and the three M stages (two buffers alternating), the nine
// derivative arrays, the three cofactors, and one patch per level.  The arrays that are dead once the level-0 patch exists (nodes,
// derivatives, cofactors) share their storage with the patches of levels 1 .. 3.  Threads own output entries of every step
// (c = tid + t * threads).  The octree is walked depth first; a child is its parent copied and halved line by line (a thread owns a line
// of 3p coefficients and runs the whole de Casteljau triangle in registers: four barriers per child).  Only minima, maxima and flags cross
// lanes (shuffles, then one LDS slot per wave and value: the nine guard extremes meet in one pass, the extremes and the flag of a patch in
// another); no floating-point atomics, no sums.  The walk's control flow is uniform over the workgroup: every thread holds the same
// reduced extremes.
//
// Records.  One HcAcc per workgroup; k_h3_finalize (behind K14's k_hc_reduce from 257 records on) combines them, the scheme of K14.
#include "tm_highorder3_cert_dev.hpp"
#include "tm_dispatch.hpp"

#include <algorithm>
#include <cstdlib>

namespace tmh {

constexpr int h3_rounds(int p) { return p == 1 ? 16 : p == 2 ? 8 : 4; }   // consecutive elements per workgroup
constexpr size_t H3_WINDOW_BYTES = size_t{256} << 20;
constexpr int h3_threads(int p) { return p == 1 ? 64 : 256; }
constexpr int h3_cmax(int a, int b) { return a > b ? a : b; }
// doubles behind the level-0 patch: the patches of levels 1 .. 3, or nine derivative arrays + three cofactors + two node buffers
constexpr int h3_work(int p) { return h3_cmax(TM_HO3_CERT_MAX_DEPTH * h3_nc(p), 9 * h3_nd(p) + 3 * h3_nf(p) + 6 * h3_nn(p)); }

__device__ __forceinline__ double h3_wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double w = __shfl_xor(v, off, 64);
        if (w > v) v = w;
    }
    return v;
}
// NV maxima over the workgroup at once, returned to every thread; red: NW * NV doubles, free again after the call.  A minimum travels as
// the maximum of the negated values (negation is exact).
template <int NW, int NV>
__device__ __forceinline__ void h3_block_max(double (&v)[NV], double* red) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = h3_wave_max(v[i]);
    if (NW == 1) return;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) red[(threadIdx.x >> 6) * NV + i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < NW; ++w)
#pragma unroll
        for (int i = 0; i < NV; ++i)
            if (red[w * NV + i] > v[i]) v[i] = red[w * NV + i];
    __syncthreads();
}

struct H3Args {
    const double *X, *Y, *Z;   // the window's fine planes, layer g0*p first
    int ni, nj, Ei, Ej;
    long long first, count;    // the window's elements: global index of its first, and how many
    const double* tab;
    double G;
    const double2* pairs;      // K16's (Jmin, Jmax), whole block
    int orientation, max_depth;
    unsigned char* status;     // whole block
    double2* bounds;
    HcAcc* partials;           // this window's records
};

template <int P>
__global__ __launch_bounds__(h3_threads(P)) void k_ho3_certify(H3Args A) {
    constexpr int N1 = P + 1, N = 3 * P, NN = h3_nn(P), ND = h3_nd(P), NF = h3_nf(P), NC = h3_nc(P), F2 = 2 * P;
    constexpr int NT = h3_threads(P), NW = NT / 64, CPL = (NC + NT - 1) / NT, NTAB = h3_tab_size(P);
    static_assert(N * N <= NT, "a thread per line of a patch");
    __shared__ double sTab[NTAB];
    __shared__ double sMain[NC + h3_work(P)];
    __shared__ double sStat[4 * HC_LEVELS];
    __shared__ double sRed[NW * 9];
    const int tid = threadIdx.x;
    for (int t = tid; t < NTAB; t += NT) sTab[t] = A.tab[t];
    const H3Tab<P> tb(sTab);
    double* const work = sMain + NC;
    double* const sDer = work;                 // du[3], dv[3], dw[3]
    double* const sCof = sDer + 9 * ND;        // cx, cy, cz
    double* const sA = sCof + 3 * NF;          // nodes, W
    double* const sB = sA + 3 * NN;            // V, control points
    const double o = A.orientation >= 0 ? 1.0 : -1.0;
    const double inf = std::numeric_limits<double>::infinity();
    const size_t ni = static_cast<size_t>(A.ni), nj = static_cast<size_t>(A.nj);
    HcAcc acc;
    hc_init(acc);
    __syncthreads();

#pragma unroll 1
    for (int round = 0; round < h3_rounds(P); ++round) {
        const long long wl = static_cast<long long>(blockIdx.x) * h3_rounds(P) + round;
        if (wl >= A.count) break;   // the workgroup's
        const long long el = A.first + wl;
        const int e = static_cast<int>(wl % A.Ei), f = static_cast<int>((wl / A.Ei) % A.Ej), gl = static_cast<int>(wl / (static_cast<long long>(A.Ei) * A.Ej));
        const size_t base = (static_cast<size_t>(gl) * P * nj + static_cast<size_t>(f) * P) * ni + static_cast<size_t>(e) * P;   // node (P, P, P) of it is inside the window
        for (int c = tid; c < 3 * NN; c += NT) {
            const int q = c / NN, r = c - q * NN, m = r / (N1 * N1), n = (r / N1) % N1, l = r % N1;
            const double* __restrict__ pl = q == 0 ? A.X : q == 1 ? A.Y : A.Z;
            sA[c] = pl[base + (static_cast<size_t>(l) * nj + n) * ni + m] - pl[base];
        }
        const double2 pr = A.pairs[el];
        const bool nodal_valid = hc_nodal_valid(pr.x, pr.y, A.orientation);
        if (tid == 0) hc_stat_init(sStat);
        __syncthreads();
        for (int c = tid; c < 3 * NN; c += NT) {   // V[m][n][k]
            const int q = c / NN, r = c - q * NN, mn = r / N1, k = r - mn * N1;
            sB[c] = hc_dot(tb.M + k * N1, sA + q * NN + mn * N1, 1, N1);
        }
        __syncthreads();
        for (int c = tid; c < 3 * NN; c += NT) {   // W[m][j][k]
            const int q = c / NN, r = c - q * NN, m = r / (N1 * N1), j = (r / N1) % N1, k = r % N1;
            sA[c] = hc_dot(tb.M + j * N1, sB + q * NN + m * N1 * N1 + k, N1, N1);
        }
        __syncthreads();
        for (int c = tid; c < 3 * NN; c += NT) {   // C[i][j][k]
            const int q = c / NN, r = c - q * NN, i = r / (N1 * N1), jk = r - i * N1 * N1;
            sB[c] = hc_dot(tb.M + i * N1, sA + q * NN + jk, N1 * N1, N1);
        }
        __syncthreads();
        double ext[9];   // max |derivative coefficient|, [3 * component + direction]
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const double* C = sB + q * NN;
            double mu = 0.0, mv = 0.0, mw = 0.0;
            for (int c = tid; c < ND; c += NT) {
                {
                    const int i = c / (N1 * N1), jk = c - i * N1 * N1;   // P x N1 x N1
                    const double a = C[(i + 1) * N1 * N1 + jk] - C[i * N1 * N1 + jk];
                    sDer[q * ND + c] = a;
                    if (fabs(a) > mu) mu = fabs(a);
                }
                {
                    const int i = c / (P * N1), r = c - i * P * N1, j = r / N1, k = r - j * N1;   // N1 x P x N1
                    const double a = C[(i * N1 + j + 1) * N1 + k] - C[(i * N1 + j) * N1 + k];
                    sDer[(3 + q) * ND + c] = a;
                    if (fabs(a) > mv) mv = fabs(a);
                }
                {
                    const int ij = c / P, k = c - ij * P;   // N1 x N1 x P
                    const double a = C[ij * N1 + k + 1] - C[ij * N1 + k];
                    sDer[(6 + q) * ND + c] = a;
                    if (fabs(a) > mw) mw = fabs(a);
                }
            }
            ext[3 * q] = mu;
            ext[3 * q + 1] = mv;
            ext[3 * q + 2] = mw;
        }
        h3_block_max<NW, 9>(ext, sRed);
        const double mx[3][3] = {{ext[0], ext[1], ext[2]}, {ext[3], ext[4], ext[5]}, {ext[6], ext[7], ext[8]}};
        const double g = h3_guard(A.G, mx);
        __syncthreads();
        for (int c = tid; c < 3 * NF; c += NT) {
            const int q = c / NF, r = c - q * NF, a = r / (F2 * F2), b = (r / F2) % F2, k = r % F2;
            const int fq = q == 2 ? 0 : q + 1, hq = q == 0 ? 2 : q - 1;
            sCof[c] = h3_cofactor<P>(a, b, k, sDer + (3 + fq) * ND, sDer + (3 + hq) * ND, sDer + (6 + fq) * ND, sDer + (6 + hq) * ND, tb);
        }
        __syncthreads();
#pragma unroll 1
        for (int t = 0; t < CPL; ++t) {
            const int c = tid + t * NT;
            if (c < NC) {
                const int a = c / (N * N), r = c - a * N * N, b = r / N, k = r - b * N;
                sMain[c] = h3_coeff<P>(a, b, k, sDer, sDer + ND, sDer + 2 * ND, sCof, sCof + NF, sCof + 2 * NF, tb);
            }
        }
        __syncthreads();   // from here on `work` holds the patches of levels 1 .. 3

        // ---- the walk, uniform over the workgroup.  child[L]: the child taken at level L; live bit L: the patch of level L on the path is
        // undecided and its children are wanted
        unsigned inv = 0, und = 0, live = 0, path = 0;   // path: three bits per level
        auto patch_of = [&](int L) -> double* { return L == 0 ? sMain : work + (L - 1) * NC; };
        auto judge = [&](int L) {
            const double* s = patch_of(L);
            double mn = inf, mxv = -inf, badv = (L == 0 && !nodal_valid) ? 1.0 : 0.0;
#pragma unroll 1
            for (int t = 0; t < CPL; ++t) {
                const int c = tid + t * NT;
                if (c < NC) {
                    const double v = o * s[c];
                    if (!__builtin_isfinite(v)) badv = 1.0;
                    if (h3_is_corner<N>(c) && !(v > 0.0)) badv = 1.0;
                    if (v < mn) mn = v;
                    if (v > mxv) mxv = v;
                }
            }
            double r3[3] = {-mn, mxv, badv};
            h3_block_max<NW, 3>(r3, sRed);
            mn = -r3[0];
            mxv = r3[1];
            badv = r3[2];
            live &= ~(1u << L);
            if (hc_visit(L, mn, mxv, badv != 0.0, g, tid == 0, sStat, inv, und) && hc_descend(L, A.max_depth, inv)) live |= 1u << L;
        };
        judge(0);
        int L = 0;
        bool descend = true;
        while (true) {
            if (descend && L < A.max_depth && ((live >> L) & 1u)) {
                ++L;
                path &= ~(7u << (3 * L));
            } else {   // next sibling, or up
                while (L > 0 && ((path >> (3 * L)) & 7u) == 7u) --L;
                if (L == 0) break;
                path += 1u << (3 * L);
            }
            const unsigned q = (path >> (3 * L)) & 7u;
            double* s = patch_of(L);
            const double* parent = patch_of(L - 1);
#pragma unroll 1
            for (int t = 0; t < CPL; ++t) {
                const int c = tid + t * NT;
                if (c < NC) s[c] = parent[c];
            }
            __syncthreads();
#pragma unroll 1
            for (int dir = 0; dir < 3; ++dir) {
                if (tid < N * N) h3_split<N>(s, dir, tid, ((q >> dir) & 1u) != 0);
                __syncthreads();
            }
            judge(L);
            descend = true;
        }
        __syncthreads();
        if (tid == 0) {
            const HcElement r = hc_decide(sStat, inv, und, A.max_depth, g);
            hc_count_element(r, nodal_valid, static_cast<unsigned long long>(el), acc);
            if (A.status) A.status[el] = static_cast<unsigned char>(r.status);
            if (A.bounds) A.bounds[el] = double2{r.lo, r.hi};
        }
        __syncthreads();
    }
    if (tid == 0) A.partials[blockIdx.x] = acc;
}

__global__ __launch_bounds__(64) void k_h3_finalize(const HcAcc* __restrict__ partials, int nwg, unsigned long long block, int Ei, int Ej, int Eg, int order,
                                                    int orientation, int max_depth, tm_ho3_certificate* __restrict__ out) {
    __shared__ HcAcc sh[64];
    records_reduce_wave<HcAcc, hc_init, hc_combine>(partials, 0, nwg, sh);
    if (threadIdx.x == 0)
        h3_finish(sh[0], block, static_cast<uint64_t>(Ei), static_cast<uint64_t>(Ej), static_cast<uint64_t>(Eg), order, orientation, max_depth, out);
}

// ------------------------------------------------------------------ host driver
static void h3_launch(int p, unsigned groups, hipStream_t st, const H3Args& a) {
    dispatch_int<1, 4>(p, [&](auto P) { hipLaunchKernelGGL(k_ho3_certify<P()>, dim3(groups), dim3(h3_threads(P())), 0, st, a); });
}

uint64_t h3_window_elements(int p, uint64_t ni, uint64_t nj, uint64_t Eg) {
    size_t budget = H3_WINDOW_BYTES;
    if (const char* s = std::getenv("TM_HO3_CERT_WINDOW_BYTES")) {
        const long long v = std::atoll(s);
        if (v > 0) budget = static_cast<size_t>(v);
    }
    const size_t layer = sizeof(double) * 3 * ni * nj, fit = budget / layer;
    const uint64_t gw = fit > static_cast<size_t>(p) ? (fit - 1) / p : 1;
    return std::min<uint64_t>(std::max<uint64_t>(gw, 1), Eg);
}

// K16's report, then window after window K11 and K17 on `st`; record, status and bounds back; returns when they have arrived.  The
// sizes and the depth have been checked.
void h3_run(const StackPlan& p, const HoPlan& pl, StackCuts& cuts, uint64_t block, uint64_t ni, uint64_t nj, int max_depth, tm_ho3_certificate* cert,
            uint8_t* h_status, double* h_bounds, hipStream_t st, const SurfPlan* sf, uint64_t* outside) {
    const int K = p.ncuts, P = pl.order;
    const uint64_t Ei = (ni - 1) / P, Ej = (nj - 1) / P, Eg = (p.nlayers - 1) / P;
    const size_t elements = static_cast<size_t>(Ei) * Ej * Eg, per_layer = static_cast<size_t>(Ei) * Ej;
    const size_t rounds = static_cast<size_t>(h3_rounds(P));
    if (elements / rounds + Eg >= (uint64_t{1} << 31)) throw TmError(TM_E_SIZE, "InconsistentSize: too many elements for one call");
    DevBuf d_pairs(sizeof(double2) * elements, "element pairs");
    tm_ho3_quality rec{};
    ho3_run(p, pl, cuts, block, ni, nj, 0, 0, nullptr, nullptr, nullptr, &rec, nullptr, st, sf, outside, d_pairs.as<double2>());   // synchronises st

    const H3Plan hp = h3_plan(P);
    stack_fill_radii(p, cuts);
    StackSurfDev sd;
    if (sf) stack_surf_upload(p, *sf, cuts, sd, st);
    const size_t rows = static_cast<size_t>(p.nlayers) * (K + 1);
    std::vector<double> table = stack_weight_table(p, 0, p.nlayers, H3_MAX_TAB);   // the weight rows of every layer, then the certificate's tables
    std::memcpy(&table[rows], hp.tab, sizeof(double) * h3_tab_size(P));
    const uint64_t gw = h3_window_elements(P, ni, nj, Eg);
    const size_t plane = static_cast<size_t>(ni) * nj, nmax = plane * (gw * P + 1);
    size_t nwg = 0;
    for (uint64_t g0 = 0; g0 < Eg; g0 += gw) nwg += (std::min(gw, Eg - g0) * per_layer + rounds - 1) / rounds;
    DevBuf d_table, d_planes(sizeof(double) * 3 * nmax, "fine planes of a window"), d_status(elements, "element status"),
        d_bounds(sizeof(double2) * elements, "element bounds"), d_rec(sizeof(HcAcc) * (nwg + RECORDS_REDUCE_GROUPS), "certificate records"),
        d_out(sizeof(tm_ho3_certificate), "certificate record");
    d_table.upload(table.data(), table.size(), st, "stack weights and certificate tables");
    H3Args a{};
    a.X = d_planes.as<double>();
    a.Y = a.X + nmax;
    a.Z = a.Y + nmax;
    a.ni = static_cast<int>(ni);
    a.nj = static_cast<int>(nj);
    a.Ei = static_cast<int>(Ei);
    a.Ej = static_cast<int>(Ej);
    a.tab = d_table.as<double>() + rows;
    a.G = hp.G;
    a.pairs = d_pairs.as<double2>();
    a.orientation = rec.orientation;
    a.max_depth = max_depth;
    a.status = d_status.as<unsigned char>();
    a.bounds = d_bounds.as<double2>();
    size_t wg_at = 0;
    for (uint64_t g0 = 0; g0 < Eg; g0 += gw) {
        const uint64_t cnt = std::min(gw, Eg - g0);
        HIPCHK(launch_stack_planes(K, cuts, sd.surf, p.mapping, d_table.as<double>() + g0 * P * (K + 1), static_cast<int>(cnt * P + 1), static_cast<int>(ni),
                                   static_cast<int>(nj), d_planes.as<double>(), d_planes.as<double>() + nmax, d_planes.as<double>() + 2 * nmax, nullptr, st));
        a.first = static_cast<long long>(g0 * per_layer);
        a.count = static_cast<long long>(cnt * per_layer);
        a.partials = d_rec.as<HcAcc>() + wg_at;
        const size_t groups = (cnt * per_layer + rounds - 1) / rounds;
        h3_launch(P, static_cast<unsigned>(groups), st, a);
        HIPCHK(hipGetLastError());
        wg_at += groups;
    }
    const Records<HcAcc> rec_in = records_first_stage(d_rec.as<HcAcc>(), nwg, st, hc_reduce_launch);
    hipLaunchKernelGGL(k_h3_finalize, dim3(1), dim3(64), 0, st, rec_in.p, rec_in.n, static_cast<unsigned long long>(block), a.Ei, a.Ej, static_cast<int>(Eg), P,
                       rec.orientation, max_depth, d_out.as<tm_ho3_certificate>());
    HIPCHK(hipGetLastError());
    tm_ho3_certificate c;
    HIPCHK(hipMemcpyAsync(&c, d_out.p, sizeof(c), hipMemcpyDeviceToHost, st));
    if (h_status) HIPCHK(hipMemcpyAsync(h_status, d_status.p, elements, hipMemcpyDeviceToHost, st));
    if (h_bounds) HIPCHK(hipMemcpyAsync(h_bounds, d_bounds.p, sizeof(double2) * elements, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));   // `table`, `sd` and the device buffers live until here
    if (cert) *cert = c;
}

}  // namespace tmh

using namespace tmh;

extern "C" int tm_stack_certify(const tm_mesh_desc* const* cuts, const tm_stack_opt* sopt, const tm_stack_surfaces* surfaces, const tm_ho_opt* opt, int32_t max_depth,
                                uint64_t block, tm_ho3_certificate* cert, uint8_t* status, double* bounds, uint64_t* outside) {
    return guarded([&]() {
        SurfPlan sf;
        const SurfPlan* sfp = nullptr;
        const StackPlan p = stack_plan_any(sopt, surfaces, sf, &sfp);
        uint64_t ni = 0, nj = 0;
        stack_check_cuts(cuts, p.ncuts, block, &ni, &nj);
        const HoPlan pl = ho3_plan(opt);
        h3_check_depth(max_depth);
        ho3_check_block(pl, block, ni, nj);
        ho3_check_layers(pl, p.nlayers);
        DevBuf in;
        StackCuts dc{};
        stack_upload_cuts(cuts, p.ncuts, block, ni, nj, in, dc);
        h3_run(p, pl, dc, block, ni, nj, max_depth, cert, status, bounds, nullptr, sfp, outside);
        return TM_OK;
    });
}

extern "C" int tm_stack_smoothers_certify(tm_smoother* const* cuts, const tm_stack_opt* sopt, const tm_stack_surfaces* surfaces, const tm_ho_opt* opt,
                                          int32_t max_depth, uint64_t block, tm_ho3_certificate* cert, uint8_t* status, double* bounds, uint64_t* outside) {
    return guarded([&]() {
        if (!cuts) throw TmError(TM_E_ARG, "null argument");
        SurfPlan sf;
        const SurfPlan* sfp = nullptr;
        const StackPlan p = stack_plan_any(sopt, surfaces, sf, &sfp);
        StackCuts dc{};
        uint64_t ni = 0, nj = 0;
        stack_resident_cuts(cuts, p, block, dc, &ni, &nj);
        const HoPlan pl = ho3_plan(opt);
        h3_check_depth(max_depth);
        ho3_check_block(pl, block, ni, nj);
        ho3_check_layers(pl, p.nlayers);
        std::vector<std::unique_ptr<StackEvent>> events;
        const hipStream_t st = stack_order_behind(cuts, p.ncuts, events);
        h3_run(p, pl, dc, block, ni, nj, max_depth, cert, status, bounds, st, sfp, outside);   // synchronises st
        return TM_OK;
    });
}
