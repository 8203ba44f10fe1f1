// Run tables, moving sides, zone rows and the strip plan of the perimeter-row launches (see tm_edge_tables.hpp).
#include "tm_edge_tables.hpp"
#include "../../include/tm_hip.h"
#include <algorithm>
#include <cstring>
#include <map>
#include <unordered_map>
#include <utility>

namespace tmh {

int64_t block_of(const Topology& topo, int64_t gid, int64_t* i, int64_t* j) {
    int64_t b = topo.nblocks() - 1;
    while (gid < topo.start[b]) --b;
    const int64_t flat = gid - topo.start[b];
    if (i) *i = flat / topo.nj[b];
    if (j) *j = flat % topo.nj[b];
    return b;
}

RunTable build_run_table(const Topology& topo, const LocalPlan& lp, const std::vector<const PlanRow*>& sel) {
    const size_t n = sel.size();
    struct HostRow {
        int32_t row, col[9], met[4];
        uint8_t flags;
        int64_t line;   // (block, grid line) the node lies on: rows of different lines never share a run
        int64_t side_key;
        int32_t pos;
    };
    std::vector<HostRow> hr(n);
    auto loc = [&](int64_t gid) {
        const int64_t l = lp.to_local(gid);
        if (l < 0) throw PlanError(TM_E_TOPOLOGY, "internal: column is neither owned nor ghost");
        return static_cast<int32_t>(l);
    };
    for (size_t k = 0; k < n; ++k) {
        const PlanRow& pr = *sel[k];
        HostRow& h = hr[k];
        std::memset(&h, 0, sizeof(h));
        h.row = loc(pr.gid);
        h.flags = pr.flags;
        // a ghost copy of a row whose rhs is the node's own boundary coordinate takes it from the row's current value
        if (h.row >= lp.n_owned) h.flags |= static_cast<uint8_t>((pr.rhs_coord & 3) << 2);
        for (int q = 0; q < pr.ncols; ++q) h.col[q] = loc(pr.col[q]);
        if (pr.kind == KIND_SMOOTHED)
            for (int q = 0; q < 4; ++q) h.met[q] = loc(pr.metric[q]);
        int64_t bi, bj;
        const int64_t b = block_of(topo, pr.gid, &bi, &bj);
        bool on_row = bi <= 1 || bi >= topo.ni[b] - 2;
        if (pr.kind == KIND_INTERIOR) {   // zone rows of the coupled triples: runs along the nearer pair of sides
            on_row = std::min(bi, topo.ni[b] - 1 - bi) <= std::min(bj, topo.nj[b] - 1 - bj);
            if (h.row < lp.n_owned) h.flags |= 16;
        }
        h.line = (b << 34) | (static_cast<int64_t>(on_row ? 0 : 1) << 33) | (on_row ? bi : bj);
        const int64_t across = on_row ? bi : bj, across_n = on_row ? topo.ni[b] : topo.nj[b];
        h.side_key = (b << 2) | (static_cast<int64_t>(on_row ? 0 : 1) << 1) | (2 * across >= across_n ? 1 : 0);
        h.pos = static_cast<int32_t>(on_row ? bj : bi);
    }
    auto same_static = [&](size_t x, size_t y) {
        const PlanRow &p = *sel[x], &q = *sel[y];
        return p.kind == q.kind && p.ncols == q.ncols && p.self == q.self && hr[x].flags == hr[y].flags && hr[x].line == hr[y].line &&
               std::memcmp(p.slot, q.slot, sizeof(p.slot)) == 0 && std::memcmp(p.cx, q.cx, sizeof(p.cx)) == 0 &&
               std::memcmp(p.cy, q.cy, sizeof(p.cy)) == 0 && std::memcmp(p.per, q.per, sizeof(p.per)) == 0;
    };
    auto static_less = [&](size_t x, size_t y) {   // any strict weak order that is consistent with same_static
        const PlanRow &p = *sel[x], &q = *sel[y];
        if (hr[x].line != hr[y].line) return hr[x].line < hr[y].line;
        if (p.kind != q.kind) return p.kind < q.kind;
        if (p.ncols != q.ncols) return p.ncols < q.ncols;
        if (p.self != q.self) return p.self < q.self;
        if (hr[x].flags != hr[y].flags) return hr[x].flags < hr[y].flags;
        int c = std::memcmp(p.slot, q.slot, sizeof(p.slot));
        if (c) return c < 0;
        c = std::memcmp(p.cx, q.cx, sizeof(p.cx));
        if (c) return c < 0;
        c = std::memcmp(p.cy, q.cy, sizeof(p.cy));
        if (c) return c < 0;
        c = std::memcmp(p.per, q.per, sizeof(p.per));
        if (c) return c < 0;
        return hr[x].row < hr[y].row;
    };
    std::vector<size_t> idx(n);
    for (size_t k = 0; k < n; ++k) idx[k] = k;
    std::sort(idx.begin(), idx.end(), static_less);
    RunTable T;
    std::vector<EdgeRun>& runs = T.runs;
    for (size_t p = 0; p < n;) {
        const size_t k0 = idx[p];
        const PlanRow& pr = *sel[k0];
        EdgeRun R;
        std::memset(&R, 0, sizeof(R));
        R.first = static_cast<int32_t>(p);
        R.count = 1;
        R.row0 = hr[k0].row;
        R.kind = pr.kind;
        R.ncols = pr.ncols;
        R.self = pr.self;
        R.flags = hr[k0].flags;
        std::memcpy(R.slot, pr.slot, sizeof(R.slot));
        std::memcpy(R.cx, pr.cx, sizeof(R.cx));
        std::memcpy(R.cy, pr.cy, sizeof(R.cy));
        std::memcpy(R.per, pr.per, sizeof(R.per));
        for (int q = 0; q < 9; ++q) R.col0[q] = hr[k0].col[q];
        for (int q = 0; q < 4; ++q) R.met0[q] = hr[k0].met[q];
        size_t e_ = p + 1;
        if (e_ < n && same_static(k0, idx[e_])) {   // strides from the second row, then as far as they hold
            const HostRow& h1 = hr[idx[e_]];
            R.row_stride = h1.row - R.row0;
            for (int q = 0; q < 9; ++q) R.col_stride[q] = h1.col[q] - R.col0[q];
            for (int q = 0; q < 4; ++q) R.met_stride[q] = h1.met[q] - R.met0[q];
            auto fits = [&](size_t j) {
                if (!same_static(k0, idx[j])) return false;
                const HostRow& h = hr[idx[j]];
                const int32_t kk = static_cast<int32_t>(j - p);
                if (h.row != R.row0 + kk * R.row_stride) return false;
                for (int q = 0; q < 9; ++q)
                    if (h.col[q] != R.col0[q] + kk * R.col_stride[q]) return false;
                for (int q = 0; q < 4; ++q)
                    if (h.met[q] != R.met0[q] + kk * R.met_stride[q]) return false;
                return true;
            };
            while (e_ < n && fits(e_)) ++e_;
            R.count = static_cast<int32_t>(e_ - p);
        }
        for (size_t j = p; j < e_; ++j) T.order.push_back(static_cast<int32_t>(idx[j]));
        runs.push_back(R);
        T.where.push_back(RunWhere{hr[k0].side_key, hr[k0].pos, e_ - p > 1 ? hr[idx[p + 1]].pos - hr[k0].pos : 0});
        p = e_;
    }
    for (size_t r = 0; r < runs.size(); ++r)
        for (int32_t k0 = 0; k0 < runs[r].count; k0 += EDGE_BLOCK) {
            T.wg_run.push_back(static_cast<int32_t>(r));
            T.wg_k0.push_back(k0);
        }
    return T;
}

MovingSides moving_sides(const Topology& topo, const LocalPlan& lp) {
    MovingSides m;
    m.dyn_mask.assign(lp.owned_blocks.size(), 0);
    for (size_t k = 0; k < lp.rows.size(); ++k) {
        const PlanRow& pr = lp.rows[k];
        if (pr.kind == KIND_FIXED) continue;
        m.nf_rows.push_back(k);
        int64_t bi, bj;
        const int64_t b = block_of(topo, pr.gid, &bi, &bj);
        const size_t kb = std::lower_bound(lp.owned_blocks.begin(), lp.owned_blocks.end(), b) - lp.owned_blocks.begin();
        // a corner node counts for its ROW only (the tiles along that row include the corner tile): the end points of an interface
        // along i = 0 must not turn the two side walls into sides whose workgroups wait for the perimeter-row pass
        const bool corner_row = bi == 0 || bi == topo.ni[b] - 1;
        if (bi == 0) m.dyn_mask[kb] |= 1;
        if (bi == topo.ni[b] - 1) m.dyn_mask[kb] |= 2;
        if (bj == 0 && !corner_row) m.dyn_mask[kb] |= 4;
        if (bj == topo.nj[b] - 1 && !corner_row) m.dyn_mask[kb] |= 8;
    }
    return m;
}

std::vector<PlanRow> zone_rows(const Topology& topo, const LocalPlan& lp, const std::vector<int>& dyn_mask, int lev) {
    std::vector<PlanRow> zone;
    const int64_t depth = 4 - lev;
    for (size_t kb = 0; kb < lp.owned_blocks.size(); ++kb) {
        const int64_t b = lp.owned_blocks[kb], bi_n = topo.ni[b], bj_n = topo.nj[b];
        const int dyn = dyn_mask[kb];
        if (!dyn) continue;
        auto add = [&](int64_t i, int64_t j) {
            PlanRow r{};
            r.gid = topo.start[b] + i * bj_n + j;
            r.kind = KIND_INTERIOR;
            r.ncols = 9;
            r.self = 4;
            int q = 0;
            for (int64_t di = -1; di <= 1; ++di)
                for (int64_t dj = -1; dj <= 1; ++dj) r.col[q++] = r.gid + di * bj_n + dj;
            zone.push_back(r);
        };
        for (int64_t i = 1; i <= bi_n - 2; ++i) {   // ascending gid
            const bool row_in = ((dyn & 1) && i <= depth) || ((dyn & 2) && i >= bi_n - 1 - depth);
            if (row_in) {
                for (int64_t j = 1; j <= bj_n - 2; ++j) add(i, j);
                continue;
            }
            if (dyn & 4)
                for (int64_t j = 1; j <= depth; ++j) add(i, j);
            if (dyn & 8)
                for (int64_t j = bj_n - 1 - depth; j <= bj_n - 2; ++j) add(i, j);
        }
    }
    return zone;
}

StripPlan build_strip_plan(const std::vector<EdgeRun>* const runs[3], const std::vector<RunWhere>& where3, int strip) {
    std::unordered_map<int32_t, std::pair<int32_t, int32_t>> made[2];   // local row id -> (run, k) in the level-1 / level-2 table
    for (int lev = 0; lev < 2; ++lev) {
        const std::vector<EdgeRun>& rl = *runs[lev];
        for (size_t r = 0; r < rl.size(); ++r)
            for (int32_t k = 0; k < rl[r].count; ++k) made[lev][rl[r].row0 + k * rl[r].row_stride] = {static_cast<int32_t>(r), k};
    }
    auto reads = [&](const EdgeRun& R, int32_t k, auto&& f) {   // every local id row k of run R reads at the previous level
        for (int q = 0; q < R.ncols; ++q) f(R.col0[q] + k * R.col_stride[q]);
        if (R.kind == KIND_SMOOTHED)
            for (int q = 0; q < 4; ++q) f(R.met0[q] + k * R.met_stride[q]);
        f(R.row0 + k * R.row_stride);
    };
    using Hull = std::map<int32_t, std::pair<int32_t, int32_t>>;   // run -> [kmin, kmax]
    auto widen = [](Hull& h, int32_t run, int32_t k) {
        auto it = h.find(run);
        if (it == h.end()) h[run] = {k, k};
        else {
            it->second.first = std::min(it->second.first, k);
            it->second.second = std::max(it->second.second, k);
        }
    };
    const std::vector<EdgeRun>& runs3 = *runs[2];
    std::map<std::pair<int64_t, int32_t>, Hull> strips;   // (side, strip number) -> level-3 rows
    for (size_t r = 0; r < runs3.size(); ++r)
        for (int32_t k = 0; k < runs3[r].count; ++k)
            widen(strips[{where3[r].side_key, (where3[r].pos0 + k * where3[r].pos_stride) / strip}], static_cast<int32_t>(r), k);
    StripPlan P;
    auto emit = [&](const Hull& h) {
        for (const auto& kv : h)
            for (int32_t k = kv.second.first; k <= kv.second.second; k += 64)
                P.tasks.push_back(LevelTask{kv.first, k, std::min<int32_t>(64, kv.second.second - k + 1)});
    };
    for (const auto& st : strips) {
        // a strip's level-3 rows need not be one range per run (two strips of one run are separate map entries: they are);
        // level 2 = hull of what they read and level 2 makes, level 1 = hull of what THAT hull reads and level 1 makes
        Hull h2, h1;
        for (const auto& kv : st.second)
            for (int32_t k = kv.second.first; k <= kv.second.second; ++k)
                reads(runs3[kv.first], k, [&](int32_t id) {
                    auto it = made[1].find(id);
                    if (it != made[1].end()) widen(h2, it->second.first, it->second.second);
                });
        for (const auto& kv : h2)
            for (int32_t k = kv.second.first; k <= kv.second.second; ++k)
                reads((*runs[1])[kv.first], k, [&](int32_t id) {
                    auto it = made[0].find(id);
                    if (it != made[0].end()) widen(h1, it->second.first, it->second.second);
                });
        P.off.push_back(static_cast<int32_t>(P.tasks.size()));
        emit(h1);
        P.off.push_back(static_cast<int32_t>(P.tasks.size()));
        emit(h2);
        P.off.push_back(static_cast<int32_t>(P.tasks.size()));
        emit(st.second);
        P.off.push_back(static_cast<int32_t>(P.tasks.size()));
    }
    P.nstrips = static_cast<int>(strips.size());
    return P;
}

}  // namespace tmh
