// Device side of the mesh quality report (tm_quality.hip): the buffers a caller keeps between calls and the two passes.
#pragma once
#include "tm_quality.h"
#include "tm_records.hpp"
#include <hip/hip_runtime.h>
#include <vector>

namespace tmh {

struct QualityBlock {   // a block resident on the device
    const double2* xy;
    int ni, nj;
    uint64_t block;     // its id in the mesh (worst_block)
};
struct QBlockDesc {     // what k_quality_finalize needs per block
    long long first;    // first record of the block
    int nwg, ni, nj, _pad;
    uint64_t block;
};

int quality_nwg(int ni, int nj);   // workgroups = records of a block's launch

// Records, block table, results and (for the field) one cell plane: allocated on first use, grown on demand, freed with the owner.
struct QualityDev {
    QualityDev() = default;
    ~QualityDev();
    QualityDev(const QualityDev&) = delete;
    QualityDev& operator=(const QualityDev&) = delete;
    DevBuf partials, desc, out, field;
    tm_quality* h_out = nullptr;           // pinned: the copy of the records back is one small asynchronous transfer
    std::vector<QBlockDesc> desc_host;     // what `desc` holds: the table is uploaded when it changes, not per call
    size_t blocks_cap = 0;                 // blocks that desc, out and h_out hold
    // one k_quality launch per block + one finalize launch; host_out[blocks.size()] in the order given, angles in degrees; synchronises
    void run(const std::vector<QualityBlock>& blocks, hipStream_t st, tm_quality* host_out);
    // per-cell min of o*s of one block, host_field[(ni-1)*(nj-1)], element j*(ni-1) + i; synchronises
    void run_field(const QualityBlock& b, int orientation, hipStream_t st, double* host_field);
    void release();
};

}  // namespace tmh
