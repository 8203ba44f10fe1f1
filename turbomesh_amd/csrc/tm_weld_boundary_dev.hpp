// Device side of K19 that other translation units use (K20 reads the faces of a resident weld): the small tables of a faces pass and the
// pass itself (tm_weld_boundary.hip).
#pragma once
#include "tm_weld_boundary.hpp"
#include "tm_weld_dev.hpp"

namespace tmh {

// the small tables of a faces pass, host and device side: they live until the caller has synchronised
struct FaceTables {
    DevBuf blocks, orient, segs, local;
    std::vector<int32_t> h_orient, h_local;
};
// the face ids of a plan on the device (asynchronous on st); d_map: the welded map on the device; d_faces: bp.faces * bp.npf ids
void weld_faces_run(const WeldPlan& pl, const WeldBoundaryPlan& bp, hipStream_t st, const int32_t* d_map, int64_t nodes_out, uint64_t nk, const int32_t* orientation,
                    int32_t* d_faces, FaceTables& keep);

}  // namespace tmh
