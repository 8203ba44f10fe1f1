// K10 Thomas-Middlecoff control field: (P,Q) of every owned block from its own four edges, one evaluation of the resident coordinates.
//
//   edge function of a polyline e[0..n-1], interior points k = 1..n-2:
//       d1 = (e[k+1] - e[k-1]) / 2,  d2 = e[k+1] - 2 e[k] + e[k-1],  f[k] = -(d1.d2) / (d1.d1)     (0 where d1.d1 == 0)
//       f[0] = f[1], f[n-1] = f[n-2];  n < 3: f = 0
//   phi_lo / phi_hi = f of the j = 0 / j = nj-1 edge (along i), psi_lo / psi_hi = f of the i = 0 / i = ni-1 edge (along j)
//       P[i][j] = (nj-1-j)/(nj-1) phi_lo[i] + j/(nj-1) phi_hi[i]
//       Q[i][j] = (ni-1-i)/(ni-1) psi_lo[j] + i/(ni-1) psi_hi[j]
//
// Two launches for all owned blocks of the rank (block table in device memory):
//   k_tm_edges  one thread per edge point, 2 (ni + nj) doubles of scratch per block: [phi_lo | phi_hi | psi_lo | psi_hi]
//   k_tm_blend  pure streaming write like K1: 16 B per node, a wave = 64 consecutive j of one group of rows, nothing read but the scratch
//
// Accuracy.  The second difference cancels: formed as (e[k+1] - 2 e[k]) + e[k-1] in fp64 it carries an error of eps |e|, which is
// eps |e| / |d2| ~ eps n^2 relative to the result.  It is formed here from two error-free additions (two_sum), so that every term d1.d2
// carries a handful of roundings relative to ITSELF: the field is within 16 eps of the exact expression's term-wise absolute sum.  The
// blend weights are both quotients of exact integers (not t and 1 - t: the latter loses (nj-1) eps next to the far edge).
#include "tm_kernels.h"

namespace tmh {

typedef double d2v __attribute__((ext_vector_type(2)));

// s + t == a + b exactly (Knuth; -ffp-contract=off keeps it as written)
__device__ __forceinline__ void two_sum(double a, double b, double& s, double& t) {
    s = a + b;
    const double bb = s - a;
    t = (a - (s - bb)) + (b - bb);
}
// e0 - 2 e1 + e2 rounded once (up to eps^2 |e|)
__device__ __forceinline__ double second_difference(double e0, double e1, double e2) {
    double s1, t1, s2, t2;
    two_sum(e2, e0, s1, t1);
    two_sum(s1, -2.0 * e1, s2, t2);
    return s2 + (t1 + t2);
}

__device__ __forceinline__ int tm_block_of(const TmFieldBlock* __restrict__ T, int nb, int wg, bool blend) {
    int b = 0;
    while (b + 1 < nb && wg >= (blend ? T[b + 1].wg_blend : T[b + 1].wg_edges)) ++b;
    return b;
}

__global__ __launch_bounds__(256) void k_tm_edges(const TmFieldBlock* __restrict__ T, int nb, const double2* __restrict__ X, double* __restrict__ scratch) {
    const int wg = static_cast<int>(blockIdx.x);
    const int b = tm_block_of(T, nb, wg, false);
    const TmFieldBlock B = T[b];
    const int ni = B.ni, nj = B.nj;
    const int t = (wg - B.wg_edges) * 256 + static_cast<int>(threadIdx.x);
    if (t >= 2 * (ni + nj)) return;
    // which edge, which point of it
    const int along_i = t < 2 * ni;
    const int u = along_i ? t : t - 2 * ni;
    const int n = along_i ? ni : nj;
    const int hi = u >= n;
    const int k = hi ? u - n : u;
    double f = 0.0;
    if (n >= 3) {
        const int kk = min(max(k, 1), n - 2);   // the end points copy their neighbour's value
        const double2* x = X + B.node0;
        // edge point q: along i at (q, 0 | nj-1), along j at (0 | ni-1, q)
        const long long stride = along_i ? nj : 1;
        const long long base = along_i ? (hi ? nj - 1 : 0) : (hi ? static_cast<long long>(ni - 1) * nj : 0);
        const double2 e0 = x[base + (kk - 1) * stride], e1 = x[base + kk * stride], e2 = x[base + (kk + 1) * stride];
        const double d1x = (e2.x - e0.x) / 2.0, d1y = (e2.y - e0.y) / 2.0;
        const double d2x = second_difference(e0.x, e1.x, e2.x), d2y = second_difference(e0.y, e1.y, e2.y);
        const double den = d1x * d1x + d1y * d1y;
        if (den != 0.0) f = -(d1x * d2x + d1y * d2y) / den;
    }
    scratch[B.edge0 + t] = f;
}

constexpr int TMB_ROWS = 8;   // rows per thread, like K1: the column's data (weights, psi) is formed once per 8 nodes
__global__ __launch_bounds__(256) void k_tm_blend(const TmFieldBlock* __restrict__ T, int nb, const double* __restrict__ scratch, double2* __restrict__ PQ) {
    const int wg = static_cast<int>(blockIdx.x);
    const int b = tm_block_of(T, nb, wg, true);
    const TmFieldBlock B = T[b];
    const int ni = B.ni, nj = B.nj;
    const int ncs = (nj + 63) / 64;          // column strips of the block
    const int tile = wg - B.wg_blend;
    const int j = (tile % ncs) * 64 + static_cast<int>(threadIdx.x);
    // a wave = 64 consecutive columns of one group of rows: the row index is wave-uniform (phi through the scalar cache)
    const int ib = __builtin_amdgcn_readfirstlane(((tile / ncs) * 4 + static_cast<int>(threadIdx.y)) * TMB_ROWS);
    if (ib >= ni) return;   // whole wave
    const double* phi_lo = scratch + B.edge0;
    const double* phi_hi = phi_lo + ni;
    const double* psi_lo = phi_hi + ni;
    const double* psi_hi = psi_lo + nj;
    const int jc = min(j, nj - 1);           // lanes past the last column stay in the wave (their row weights are read below) and store nothing
    const double dj = static_cast<double>(nj - 1), di = static_cast<double>(ni - 1);
    const double t_lo = static_cast<double>(nj - 1 - jc) / dj, t_hi = static_cast<double>(jc) / dj;
    const double q_lo = psi_lo[jc], q_hi = psi_hi[jc];
    // the row weights of the wave's 8 rows: lane k forms row ib + k's, every lane reads them from there
    const int ir = min(ib + static_cast<int>(threadIdx.x & 7), ni - 1);
    const double s_lo_l = static_cast<double>(ni - 1 - ir) / di, s_hi_l = static_cast<double>(ir) / di;
    double2* dst = PQ + B.node0 + static_cast<long long>(ib) * nj + jc;
#pragma unroll
    for (int k = 0; k < TMB_ROWS; ++k) {
        if (ib + k >= ni) break;   // scalar
        const double s_lo = __shfl(s_lo_l, k, 64), s_hi = __shfl(s_hi_l, k, 64);
        const double p_lo = phi_lo[ib + k], p_hi = phi_hi[ib + k];
        d2v o;
        o.x = t_lo * p_lo + t_hi * p_hi;
        o.y = s_lo * q_lo + s_hi * q_hi;
        if (j < nj) __builtin_nontemporal_store(o, reinterpret_cast<d2v*>(dst + static_cast<long long>(k) * nj));
    }
}

int tm_field_edges_nwg(int ni, int nj) { return (2 * (ni + nj) + 255) / 256; }
int tm_field_blend_nwg(int ni, int nj) { return ((nj + 63) / 64) * ((ni + 4 * TMB_ROWS - 1) / (4 * TMB_ROWS)); }

hipError_t launch_tm_field(const TmFieldBlock* table, int nblocks, int nwg_edges, int nwg_blend, const double2* X, double* scratch, double2* PQ,
                           hipStream_t st) {
    if (nblocks <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_tm_edges, dim3(nwg_edges), dim3(256), 0, st, table, nblocks, X, scratch);
    hipLaunchKernelGGL(k_tm_blend, dim3(nwg_blend), dim3(64, 4), 0, st, table, nblocks, scratch, PQ);
    return hipGetLastError();
}

}  // namespace tmh
