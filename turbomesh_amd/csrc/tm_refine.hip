// Iterative refinement (TM_OPT_REFINE, tm_csr_residual, tm_smoother_residual): the one thing a refinement step needs that the solvers do
// not have -- a residual formed in MORE than working precision.  An fp64 residual of a solution that is good to fp64 is rounding noise
// (its terms cancel to the last bit); in double-double it carries ~50 digits of the true b - A x, and a correction solved from it in
// working precision brings x to the rounded exact solution.  See tm_refine.hpp for the valid domain and the error bound.
#include "tm_refine.hpp"
#include "tm_devutil.hpp"

namespace tmh {

namespace {

// (hi, lo) with hi + lo the value, |lo| <= ulp(hi) / 2
struct dd {
    double hi, lo;
};
// error-free sum of two doubles (Knuth): s = fl(a + b), e = (a + b) - s exactly, no ordering of |a|, |b| assumed
__device__ __forceinline__ dd two_sum(double a, double b) {
    const double s = a + b;
    const double bb = s - a;
    return dd{s, (a - (s - bb)) + (b - bb)};
}
// acc - a * x: the product exactly as p + e (e = fma(a, x, -p)), p joins the high part by an error-free sum, the three low-order terms
// are added in fp64 (two roundings of quantities <= 2^-52 (|acc| + |p|): error <= 2^-104 (|acc| + |p|)), and a second error-free sum
// renormalises -- the full one, since after cancellation the low part may outweigh the high one
__device__ __forceinline__ dd dd_sub_product(dd acc, double a, double x) {
    const double p = a * x;
    const double e = fma(a, x, -p);
    const dd s = two_sum(acc.hi, -p);
    return two_sum(s.hi, (s.lo + acc.lo) - e);
}

__global__ __launch_bounds__(256) void k_csr_residual_dd(int n, const int32_t* __restrict__ p, const int32_t* __restrict__ ci, const double* __restrict__ vx,
                                                         const double* __restrict__ vy, const double2* __restrict__ x, const double2* b, double2* r) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    const double2 rhs = b[row];
    dd sx{rhs.x, 0.0}, sy{rhs.y, 0.0};   // b enters the same sum
    const int end = p[row + 1];
    for (int k = p[row]; k < end; ++k) {
        const double2 w = x[ci[k]];
        sx = dd_sub_product(sx, vx[k], w.x);
        sy = dd_sub_product(sy, vy[k], w.y);
    }
    r[row] = make_double2(sx.hi, sy.hi);   // hi = fl(hi + lo): the one rounding to fp64
}

__global__ __launch_bounds__(256) void k_refine_update(int n, double2* __restrict__ x, const double2* __restrict__ d, double* partials) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    double acc[MAX_PARTIALS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (row < n) {
        const double2 di = d[row], xi = x[row];
        const double2 o = make_double2(xi.x + di.x, xi.y + di.y);
        x[row] = o;
        acc[0] = di.x * di.x;
        acc[1] = di.y * di.y;
        acc[2] = o.x * o.x;
        acc[3] = o.y * o.y;
    }
    block_partials<256, 4>(acc, partials + static_cast<size_t>(blockIdx.x) * MAX_PARTIALS);
}

}  // namespace

hipError_t launch_csr_residual_dd(int n, const int32_t* p, const int32_t* ci, const double* vx, const double* vy, const double2* x, const double2* b,
                                  double2* r, hipStream_t st) {
    hipLaunchKernelGGL(k_csr_residual_dd, dim3((n + 255) / 256), dim3(256), 0, st, n, p, ci, vx, vy, x, b, r);
    return hipGetLastError();
}
hipError_t launch_refine_update(int n, double2* x, const double2* d, double* partials, hipStream_t st) {
    hipLaunchKernelGGL(k_refine_update, dim3((n + 255) / 256), dim3(256), 0, st, n, x, d, partials);
    return hipGetLastError();
}

}  // namespace tmh
