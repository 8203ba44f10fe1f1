// Device side of K18 (tm_weld.hip): the buffers a caller keeps between calls and the stages of a weld.
#pragma once
#include "tm_weld.hpp"
#include "tm_devbuf.hpp"
#include <hip/hip_runtime.h>

namespace tmh {

struct WeldGap {   // the largest gap so far and the smallest index at which it occurs
    double gap;
    unsigned long long node;
};
// where k_weld_gap reads a node's own coordinates: planes in flat order, layer-major (component c at planes + c*comp_stride), or the
// interleaved blocks of a handle
struct WeldSrc {
    const double* planes;
    long long comp_stride;
    const double2* const* resident;
    int ncomp, layers;
};
enum { WELD_C2 = 0, WELD_C3, WELD_C4, WELD_C5, WELD_MAX_CLASS, WELD_NODES_OUT, WELD_COUNTERS };

// Tables, labels, partial sums, the map, welded planes and cells: allocated on first use, grown on demand, freed with the owner.
struct WeldDev {
    DevBuf blocks, conns, parent, count, map, part1, off1, part2, off2, counters, src, out, gaps, gap, ptrs, local, cells;
    // 1. tables up, labels of the perimeter slots, hook, compress, class counts (asynchronous on st)
    void link(const WeldPlan& pl, hipStream_t st);
    // 2. owner flags -> exclusive prefix sum -> map on the device; nodes_out into the counters (asynchronous)
    void number(const WeldPlan& pl, hipStream_t st);
    // map and counters to the host (synchronises); info's class fields and node counts
    void read_map(const WeldPlan& pl, hipStream_t st, int32_t* map, tm_weld_info* info);
    // 3. welded planes of host planes (uploaded) into this->out, gap record; downloads into out[] and synchronises
    void points_planes(const WeldPlan& pl, hipStream_t st, int ncomp, int64_t layers, int64_t nodes_out, const double* const* planes, double* const* out, WeldGap* gap);
    // 3. the same from the interleaved blocks of a handle (device pointers per block)
    void points_resident(const WeldPlan& pl, hipStream_t st, const std::vector<const double2*>& X, int64_t nodes_out, double* x, double* y, WeldGap* gap);
    // 4. cells of the map on the device; downloads and synchronises
    void cells_run(const WeldPlan& pl, hipStream_t st, const std::vector<int64_t>& cells_of, int order, uint64_t nk, int64_t nodes_out, int32_t* cells);
    void upload_map(const WeldPlan& pl, hipStream_t st, const int32_t* map);
    // exclusive prefix sum of n int32 values on the device (n <= 2^30) by the launches of stage 2: sums of tiles, their scan, the scan inside
    // the tiles (K21 scans its per-cell face counts with it; asynchronous, uses part1 / off1 / part2 / off2)
    void exscan(hipStream_t st, const int32_t* in, int n, int32_t* out);

private:
    void gap_run(const WeldPlan& pl, hipStream_t st, const WeldSrc& s, int64_t nodes_out, WeldGap* gap);
};

}  // namespace tmh
