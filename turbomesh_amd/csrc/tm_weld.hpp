// K18  welding blocks into one conforming unstructured mesh (include/tm_hip.h, "welded unstructured mesh"): the index arithmetic that the
// kernels (tm_weld.hip) and the host definition (tm_weld_host.cpp) share -- flat index, side and position to node, the perimeter slots
// in which the union-find lives, and the validated view of a mesh description.  Integers only: host and device agree exactly.
#pragma once
#include "../../include/tm_hip.h"

#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TM_WELD_HD __host__ __device__ inline
#else
#define TM_WELD_HD inline
#endif

namespace tmh {

constexpr int64_t WELD_MAX_ID = 2147483647;   // ids are int32_t

// One block as the kernels see it: the flat index of its node (0,0), the global perimeter slot of that node, its size.
struct WeldBlock {
    int32_t off, slot0, ni, nj;
};

// node (i, j) of a side at range position pos: i_min is j = 0 parametrised by i, j_min is i = 0 parametrised by j (tm_plan.cpp range_points)
TM_WELD_HD void weld_side_node(int ni, int nj, uint32_t side, int pos, int& i, int& j) {
    switch (side) {
    case TM_SIDE_I_MIN: i = pos; j = 0; break;
    case TM_SIDE_I_MAX: i = pos; j = nj - 1; break;
    case TM_SIDE_J_MIN: i = 0; j = pos; break;
    default: i = ni - 1; j = pos; break;
    }
}
TM_WELD_HD int weld_side_length(int ni, int nj, uint32_t side) { return side == TM_SIDE_I_MIN || side == TM_SIDE_I_MAX ? ni : nj; }
// position of pair t of a range: start + t, or start - t when the range runs reversed
TM_WELD_HD int64_t weld_range_pos(uint64_t start, uint64_t end, int64_t t) {
    return start > end ? static_cast<int64_t>(start) - t : static_cast<int64_t>(start) + t;
}
TM_WELD_HD int64_t weld_range_length(uint64_t start, uint64_t end) { return static_cast<int64_t>(start > end ? start - end : end - start) + 1; }

// The perimeter of a block in the order of the flat index j*ni + i: row j = 0, then the pairs (0, j), (ni-1, j) of the rows between,
// then row j = nj-1 -- 2 (ni + nj) - 4 slots.  Slots ascend with the flat index, block after block, so the smallest slot of a class is
// its smallest flat index: the union-find runs on slots and never divides.
TM_WELD_HD int weld_perimeter(int ni, int nj) { return 2 * (ni + nj) - 4; }
TM_WELD_HD bool weld_on_perimeter(int ni, int nj, int i, int j) { return i == 0 || j == 0 || i == ni - 1 || j == nj - 1; }
TM_WELD_HD int weld_slot(int ni, int nj, int i, int j) {
    if (j == 0) return i;
    if (j == nj - 1) return ni + 2 * (nj - 2) + i;
    return ni + 2 * (j - 1) + (i == 0 ? 0 : 1);
}
TM_WELD_HD void weld_slot_node(int ni, int nj, int slot, int& i, int& j) {
    if (slot < ni) {
        i = slot;
        j = 0;
    } else if (slot >= ni + 2 * (nj - 2)) {
        i = slot - ni - 2 * (nj - 2);
        j = nj - 1;
    } else {
        const int k = slot - ni;
        i = (k & 1) ? ni - 1 : 0;
        j = 1 + (k >> 1);
    }
}
// the block of flat index n: the last block whose offset is <= n
TM_WELD_HD int weld_block_of(const WeldBlock* blocks, int nblocks, int n) {
    int lo = 0, hi = nblocks - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (blocks[mid].off <= n) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// A mesh description checked once (sizes, ranges, id range): what the host definition and the device driver both start from.
struct WeldPlan {
    std::vector<WeldBlock> blocks;
    std::vector<tm_connection> conns;   // as given
    int64_t nodes = 0, slots = 0, max_pairs = 0, periodic_pairs = 0;
    int nblocks() const { return static_cast<int>(blocks.size()); }
    int slot_of(const tm_range& r, int64_t t) const {   // global perimeter slot of pair t of a range
        const WeldBlock& b = blocks[r.block];
        int i, j;
        weld_side_node(b.ni, b.nj, r.side, static_cast<int>(weld_range_pos(r.start, r.end, t)), i, j);
        return b.slot0 + weld_slot(b.ni, b.nj, i, j);
    }
    int flat_of(const tm_range& r, int64_t t) const {
        const WeldBlock& b = blocks[r.block];
        int i, j;
        weld_side_node(b.ni, b.nj, r.side, static_cast<int>(weld_range_pos(r.start, r.end, t)), i, j);
        return b.off + j * b.ni + i;
    }
};
// TM_E_ARG / TM_E_SIZE / TM_E_MISMATCH as include/tm_hip.h says for tm_weld_map
WeldPlan weld_plan(const tm_mesh_desc* mesh);
// nk * nodes_out <= 2^31 - 1, else TM_E_ARG; returns the layer count that counts (nk <= 1: one)
int64_t weld_layers(uint64_t nk, uint64_t nodes_out);
// tm_ho_check / tm_ho3_check of the order and layer count, and the number of elements of every block into cells_of (prefix, nblocks + 1)
void weld_cells_plan(const tm_mesh_desc* mesh, const WeldPlan& pl, int order, uint64_t nk, std::vector<int64_t>& cells_of);
// local nodes in VTK's Lagrange order, packed a | b << 8 | c << 16: (p+1)^2 for quadrilaterals, (p+1)^3 for hexahedra
std::vector<int32_t> weld_local_order(int order, bool hex);

// The host definition, piecewise (tm_weld_host.cpp): also what the device entry points use for the small host-side parts.
void weld_map_host(const WeldPlan& pl, int32_t* map, tm_weld_info* info);
// 1 + the largest id of a map (TM_E_ARG for a negative id)
uint64_t weld_nodes_out(const WeldPlan& pl, const int32_t* map);
// TM_E_ARG for a null pointer or a component count outside 1 .. 3
void weld_points_check(const WeldPlan& pl, const int32_t* map, int32_t ncomp, const double* const* planes, double* const* out);
// periodic_gap from the welded planes (components 0 and 1 of every layer)
double weld_periodic_gap(const WeldPlan& pl, const int32_t* map, int ncomp, uint64_t layers, uint64_t nodes_out, const double* const* out);

}  // namespace tmh
