// The fixed-order combination of per-workgroup records that every report ends with (K10 quality, K12, K13, K14, K16, K17), and the
// two-stage choreography of the drivers whose records hold only counts, minima and maxima.
#pragma once
#include "tm_devbuf.hpp"

namespace tmh {

#ifdef __HIP__
// One wave of 64 lanes: lane t combines records begin + t, begin + t + 64, ... in that order, then the 64 lanes' records meet pairwise
// through LDS (32, 16, ... 1): a fixed order, so the sums are the same on every run.  The result is sh[0]; sh holds 64 records.  Index
// is the caller's count type (int, or long long where the count is 64-bit).
template <class Acc, void (*Init)(Acc&), void (*Combine)(Acc&, const Acc&), class Index>
__device__ __forceinline__ void records_reduce_wave(const Acc* __restrict__ records, Index begin, Index end, Acc* sh) {
    Acc a;
    Init(a);
    for (Index r = begin + static_cast<Index>(threadIdx.x); r < end; r += 64) Combine(a, records[r]);
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int off = 32; off > 0; off >>= 1) {
        if (static_cast<int>(threadIdx.x) < off) Combine(sh[threadIdx.x], sh[threadIdx.x + off]);
        __syncthreads();
    }
}
#endif

// records from which the finalize gets a first stage, and that stage's workgroups (a lone wave over the 16 641 records of a 4097^2
// block takes as long as the elevation itself)
constexpr int RECORDS_REDUCE_FROM = 256, RECORDS_REDUCE_GROUPS = 64;

template <class Acc>
struct Records {
    const Acc* p;
    int n;
};
// What the finalize reads.  `partials` holds nwg records and room for RECORDS_REDUCE_GROUPS more behind them; above
// RECORDS_REDUCE_FROM records `first_stage` (workgroup g reduces [g * chunk, (g+1) * chunk) to out[g]) leaves at most
// RECORDS_REDUCE_GROUPS there.  A report that has one stage (K10, K12) keeps it: a second one changes the order of its floating-point sums.
template <class Acc>
inline Records<Acc> records_first_stage(Acc* partials, size_t nwg, hipStream_t st,
                                        void (*first_stage)(const Acc* partials, int nrec, int chunk, int groups, Acc* out, hipStream_t st)) {
    const int nrec = static_cast<int>(nwg);
    if (nrec <= RECORDS_REDUCE_FROM) return {partials, nrec};
    const int chunk = (nrec + RECORDS_REDUCE_GROUPS - 1) / RECORDS_REDUCE_GROUPS, groups = (nrec + chunk - 1) / chunk;
    first_stage(partials, nrec, chunk, groups, partials + nwg, st);
    hip_check(hipGetLastError(), "first stage of the record combination");
    return {partials + nwg, groups};
}

}  // namespace tmh
