// Device side of the high-order certificate (tm_highorder_cert.hip, K14): the buffers a caller keeps between calls and the one pass.
#pragma once
#include "tm_highorder_cert.hpp"
#include "tm_highorder_dev.hpp"

namespace tmh {

// Tables, one status byte and one (lo, hi) pair per element, partial records and the result: allocated on first use, grown on demand,
// freed with the owner.
struct HcDev {
    DevBuf tab, status, bounds, partials, out;
    HcPlan plan;                       // the tables in `tab`: formed and uploaded when the order changes (plan.order == 0: none yet)
    // K13's report through `ho` (the orientation; its pairs stay on the device), one k_ho_certify launch and the finalize on the block X
    // (already checked against the plan); cert, status, bounds as tm_ho_certify; synchronises
    void run(HoDev& ho, const HoPlan& hoplan, const double2* X, int ni, int nj, uint64_t block, hipStream_t st, int max_depth,
             tm_ho_certificate* cert, uint8_t* status, double* bounds);
};
// workgroups of the K14 launch on a block with that many elements
int hc_workgroups(int order, uint64_t elements);
// the first stage of records_first_stage over HcAcc: k_hc_reduce (tm_highorder_cert.hip), also K17's
void hc_reduce_launch(const HcAcc* partials, int nrec, int chunk, int groups, HcAcc* out, hipStream_t st);

}  // namespace tmh
