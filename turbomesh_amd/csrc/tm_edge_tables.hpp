// Host-side planning of the perimeter-row launches (pure C++, no HIP), one step downstream of tm_plan: compresses selections of
// PlanRows into the run tables the perimeter-row kernels read (tm_edge_types.h), finds the sides of a block whose perimeter rows move,
// generates the zone rows of the coupled sweep triples and plans the strips of the fused level kernel.  Covered on the CPU by
// tests/test_edge_tables_cpu.py through tm_edge_tables_probe (include/tm_hip_diag.h).
#pragma once
#include "tm_edge_types.h"
#include "tm_plan.hpp"
#include <cstddef>
#include <cstdint>
#include <vector>

namespace tmh {

// the block a global row id lies in and, where asked for, its (i, j) there
int64_t block_of(const Topology& topo, int64_t gid, int64_t* i = nullptr, int64_t* j = nullptr);

// where a run lies: the strip plan of the fused level kernel cuts the level-3 runs by position along their lines
struct RunWhere {
    int64_t side_key;            // (block, runs along rows or columns, lower or upper half of the block)
    int32_t pos0, pos_stride;    // position of its first point along the line and the position step
};
struct RunTable {
    std::vector<EdgeRun> runs;
    std::vector<int32_t> wg_run, wg_k0;   // per workgroup: the run it serves and the first point of its stretch (EDGE_BLOCK points)
    std::vector<int32_t> order;           // order[p] = position in the selection of the row at position p of the run order
    std::vector<RunWhere> where;          // per run
};
// Per-row table -> runs (tm_edge_types.h EdgeRun).  Rows are grouped by everything that must be equal along a run (static fields
// and the grid line of their block they lie on), sorted by row id within a group and cut wherever an index stops advancing by
// the stride of the stretch.  Throws PlanError(TM_E_TOPOLOGY) for a column that is neither owned nor ghost.
RunTable build_run_table(const Topology& topo, const LocalPlan& lp, const std::vector<const PlanRow*>& sel);

// Relaxation sweeps never have to touch a `fixed` row: it returns its boundary coordinate (smooth.zig:790-795), which the
// perimeter of every field buffer holds from upload() on.  They run the perimeter-row kernel over the other rows only
// (none at all for a block with fixed walls), and the K2x2 workgroups along sides without such rows do not have to wait
// for it.  nf_rows: positions in lp.rows of the rows that are not `fixed`; dyn_mask per owned block: bit 0 = row i = 0 has
// non-fixed rows, 1 = row ni-1, 2 = column j = 0, 3 = column nj-1.
struct MovingSides {
    std::vector<size_t> nf_rows;
    std::vector<int> dyn_mask;
};
MovingSides moving_sides(const Topology& topo, const LocalPlan& lp);

// Coupled triples: level l = lev + 1 (1..3) evaluates the moving perimeter rows and, as KIND_INTERIOR rows (K2's own arithmetic on the
// gathered 3 x 3 neighbourhood), the interior nodes within 5 - l of a side whose perimeter rows move (Chebyshev distance: the 9-point
// stencil's dependency cone); what level l reads at level l - 1 lies within 6 - l of such a side or on the perimeter.  Ascending gid.
std::vector<PlanRow> zone_rows(const Topology& topo, const LocalPlan& lp, const std::vector<int>& dyn_mask, int lev);

// Strip plan of the fused level kernel (k_edge_levels3): level-3 rows by strips of `strip` positions along their lines, per side of a
// block; per strip the level-2 rows its level-3 rows read, and the level-1 rows THOSE read (hulls per run).  runs[l] = the runs of the
// level l + 1 table, where3 = the RunWhere records of the level-3 table.
struct StripPlan {
    int nstrips = 0;
    std::vector<LevelTask> tasks;   // all strips, level by level
    std::vector<int32_t> off;       // [nstrips * 4], see FusedLevelsDev
};
StripPlan build_strip_plan(const std::vector<EdgeRun>* const runs[3], const std::vector<RunWhere>& where3, int strip);

}  // namespace tmh
