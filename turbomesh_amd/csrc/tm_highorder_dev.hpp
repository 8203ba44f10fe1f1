// Device side of the high-order elevation (tm_highorder.hip, K13): the buffers a caller keeps between calls and the one pass.
#pragma once
#include "tm_highorder.hpp"
#include "tm_records.hpp"
#include <hip/hip_runtime.h>

namespace tmh {

// Tables, the two planes, one (Jmin, Jmax) pair per element, partial records and the result: allocated on first use, grown on demand,
// freed with the owner.
struct HoDev {
    DevBuf tab, planes, pairs, partials, out;
    // one k_ho_elevate launch + the finalize (two launches from 257 workgroups on) on the block X (node (i,j) at i*nj + j, already checked against the plan);
    // x, y, q, sj as tm_ho_elevate; synchronises
    void run(const HoPlan& plan, const double2* X, int ni, int nj, uint64_t block, hipStream_t st, double* x, double* y, tm_ho_quality* q, double* sj);
};

// the first stage of records_first_stage over HoAcc: k_ho_reduce (tm_highorder.hip), also K16's
void ho_reduce_launch(const HoAcc* partials, int nrec, int chunk, int groups, HoAcc* out, hipStream_t st);

}  // namespace tmh
