// Device side of the high-order elevation (tm_highorder.hip, K13): the buffers a caller keeps between calls and the one pass.
#pragma once
#include "tm_highorder.hpp"
#include <hip/hip_runtime.h>

namespace tmh {

// Tables, the two planes, one (Jmin, Jmax) pair per element, partial records and the result: hipMalloc'ed on first use, grown on demand,
// freed with the owner.
struct HoDev {
    HoDev() = default;
    ~HoDev();
    HoDev(const HoDev&) = delete;
    HoDev& operator=(const HoDev&) = delete;
    double* tab = nullptr;
    double* planes = nullptr;
    double2* pairs = nullptr;
    HoAcc* partials = nullptr;
    tm_ho_quality* out = nullptr;
    size_t planes_cap = 0, pairs_cap = 0, partials_cap = 0;
    // one k_ho_elevate launch + the finalize (two launches from 257 workgroups on) on the block X (node (i,j) at i*nj + j, already checked against the plan);
    // x, y, q, sj as tm_ho_elevate; synchronises
    void run(const HoPlan& plan, const double2* X, int ni, int nj, uint64_t block, hipStream_t st, double* x, double* y, tm_ho_quality* q, double* sj);
};

#ifdef __HIP__
// lane t of a wave combines records t, t + 64, ... in that order, then the 64 lanes' records pairwise through LDS (32, 16, ... 1): a
// fixed order, so the sums are the same on every run
__device__ __forceinline__ void ho_reduce_wave(const HoAcc* __restrict__ partials, int begin, int end, HoAcc* sh) {
    HoAcc a;
    ho_init(a);
    for (int r = begin + static_cast<int>(threadIdx.x); r < end; r += 64) ho_combine(a, partials[r]);
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int off = 32; off > 0; off >>= 1) {
        if (static_cast<int>(threadIdx.x) < off) ho_combine(sh[threadIdx.x], sh[threadIdx.x + off]);
        __syncthreads();
    }
}
#endif

}  // namespace tmh
