// K15  the surface stage of the stacking kernels (include/tm_hip.h, "cuts on stream surfaces of revolution"): interval location and the
// Horner evaluation of a cut's meridional table, __host__ __device__, compiled into K11 / K12 and into the host definition
// (tm_stack_host.cpp) -- the same operations in the same order, nothing fused (-ffp-contract=off on both sides), so x_c and r_c are equal
// between host and device bit for bit.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TM_SURF_HD __host__ __device__ inline
#else
#define TM_SURF_HD inline
#endif

namespace tmh {

constexpr int SURF_COEF = 8;   // per interval: ax bx cx dx ar br cr dr

// The first step of the search below: the largest power of two <= max(N - 2, 1).
TM_SURF_HD int surf_first_step(int N) {
    int step = 1;
    while (2 * step <= N - 2) step *= 2;
    return step;
}

// The largest n <= N-2 with u[n] <= un, n = 0 when un < u[0] (or un is NaN): the index is built bit by bit from the top, a fixed number
// of steps for a table (ceil(log2(N - 1)) at the most), no branch on the data.  u: the N knots, strictly increasing.  Reads u[1 .. N-2].
TM_SURF_HD int surf_locate(const double* u, int N, double un) {
    int n = 0;
    for (int step = surf_first_step(N); step > 0; step >>= 1) {
        const int cand = n + step;
        const bool in = cand <= N - 2;
        const double uc = u[in ? cand : 0];
        n = (in && uc <= un) ? cand : n;
    }
    return n;
}

// The same index from a table staged for the kernels: u[n] for n <= N-2 as they are, +inf from u[N-1] on up to index 2 * first_step - 1
// (first_step = surf_first_step(N)), so that no step needs a bound: the comparison with +inf fails where the index would leave the table.
TM_SURF_HD int surf_locate_padded(const double* u, int first_step, double un) {
    int n = 0;
    for (int step = first_step; step > 0; step >>= 1) {
        const int cand = n + step;
        n = u[cand] <= un ? cand : n;
    }
    return n;
}

// t = un - u[n] with one rounding; a + t*(b + t*(c + t*d)), innermost first, every operation rounded; x from coef[0..3], r from coef[4..7]
TM_SURF_HD void surf_eval(const double* coef, double un_minus_knot, double* x, double* r) {
    const double t = un_minus_knot;
    *x = coef[0] + t * (coef[1] + t * (coef[2] + t * coef[3]));
    *r = coef[4] + t * (coef[5] + t * (coef[6] + t * coef[7]));
}

// u outside [u[0], u[N-1]]: the end interval's polynomial is continued, and the node is counted
TM_SURF_HD bool surf_outside(double u0, double ulast, double un) { return un < u0 || un > ulast; }

}  // namespace tmh
