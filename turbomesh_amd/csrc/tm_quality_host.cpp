// Host side of the mesh quality report: tm_mesh_quality_host (the definitions of include/tm_hip.h as a plain loop over the
// per-cell function the device kernel uses, tm_quality.h) and what both paths do after the blocks' records exist -- cosines to
// degrees, and the `total` record.  No HIP call in this file: it works in a process without a device.
#include "tm_quality.h"
#include "tm_api_util.hpp"
#include "tm_refmath.h"

#include <vector>

namespace tmh {

void quality_angles(tm_quality* q) {
    const double pi = 3.14159265358979323846;
    // largest cosine -> smallest angle; NaN (no non-degenerate cell) stays NaN
    q->min_angle_deg = tm_refmath::acos(q->min_angle_deg) * (180.0 / pi);
    q->max_angle_deg = tm_refmath::acos(q->max_angle_deg) * (180.0 / pi);
}

void quality_block_host(const double* xy, uint64_t ni, uint64_t nj, uint64_t block, tm_quality* out) {
    const QPoint* X = reinterpret_cast<const QPoint*>(xy);
    auto at = [&](uint64_t i, uint64_t j) -> const QPoint& { return X[i * nj + j]; };
    QAcc acc;
    q_init(acc);
    for (uint64_t i = 0; i + 1 < ni; ++i)
        for (uint64_t j = 0; j + 1 < nj; ++j) {
            const QPoint &A = at(i, j), &B = at(i + 1, j), &C = at(i + 1, j + 1), &D = at(i, j + 1);
            double l2_ab, l_ab, l2_dc, l_dc, l2_ad, l_ad, l2_bc, l_bc;
            q_edge(A, B, l2_ab, l_ab);
            q_edge(D, C, l2_dc, l_dc);
            q_edge(A, D, l2_ad, l_ad);
            q_edge(B, C, l2_bc, l_bc);
            const QCell c = q_cell(A, B, C, D, l2_ab, l_ab, l2_dc, l_dc, l2_ad, l_ad, l2_bc, l_bc);
            const int bin = q_count_cell(c, i * (nj - 1) + j, acc);
            if (bin >= 0) acc.hist[bin / 10][bin % 10] += 1;
        }
    // growth along the i lines (fixed j) and the j lines (fixed i), boundary lines included
    for (uint64_t j = 0; j < nj; ++j) {
        double l2, prev = 0.0, cur;
        for (uint64_t i = 0; i + 1 < ni; ++i) {
            q_edge(at(i, j), at(i + 1, j), l2, cur);
            if (i > 0) q_growth(prev, cur, acc.gi);
            prev = cur;
        }
    }
    for (uint64_t i = 0; i < ni; ++i) {
        double l2, prev = 0.0, cur;
        for (uint64_t j = 0; j + 1 < nj; ++j) {
            q_edge(at(i, j), at(i, j + 1), l2, cur);
            if (j > 0) q_growth(prev, cur, acc.gj);
            prev = cur;
        }
    }
    q_finish(acc, block, ni, nj, out);
    quality_angles(out);
}

void quality_total(const tm_quality* pb, uint64_t nblocks, tm_quality* t) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::memset(t, 0, sizeof(*t));
    t->min_scaled_jacobian = t->min_angle_deg = t->max_angle_deg = t->max_aspect = t->min_area = t->max_area = nan;
    t->max_growth_i = t->max_growth_j = 1.0;
    bool first = true;
    auto lower = [](double& a, double b) {   // NaN = no value yet
        if (b == b && !(a <= b)) a = b;
    };
    auto raise = [](double& a, double b) {
        if (b == b && !(a >= b)) a = b;
    };
    for (uint64_t b = 0; b < nblocks; ++b) {
        const tm_quality& q = pb[b];
        if (q.cells == 0) continue;   // a block this rank does not own
        t->cells += q.cells;
        t->inverted += q.inverted;
        t->degenerate += q.degenerate;
        for (int k = 0; k < 10; ++k) t->hist[k] += q.hist[k];
        if (first) t->orientation = q.orientation;
        else if (t->orientation != q.orientation) t->orientation = 0;
        first = false;
        if (q.min_scaled_jacobian == q.min_scaled_jacobian && !(t->min_scaled_jacobian <= q.min_scaled_jacobian)) {   // strict: ties stay with the lower block
            t->min_scaled_jacobian = q.min_scaled_jacobian;
            t->worst_block = q.worst_block;
            t->worst_i = q.worst_i;
            t->worst_j = q.worst_j;
        }
        lower(t->min_angle_deg, q.min_angle_deg);
        raise(t->max_angle_deg, q.max_angle_deg);
        raise(t->max_aspect, q.max_aspect);
        raise(t->max_growth_i, q.max_growth_i);
        raise(t->max_growth_j, q.max_growth_j);
        lower(t->min_area, q.min_area);
        raise(t->max_area, q.max_area);
        t->total_area += q.total_area;
    }
}

}  // namespace tmh

using namespace tmh;

extern "C" int tm_mesh_quality_host(const tm_mesh_desc* mesh, tm_quality* per_block, tm_quality* total) {
    return guarded([&]() {
        if (!mesh || !mesh->blocks || mesh->nblocks == 0) throw TmError(TM_E_ARG, "mesh description without blocks");
        for (uint64_t b = 0; b < mesh->nblocks; ++b) {
            const tm_block& k = mesh->blocks[b];
            if (!k.xy) throw TmError(TM_E_ARG, "block without coordinates");
            if (k.ni < 2 || k.nj < 2 || k.ni * k.nj >= (uint64_t{1} << 31)) throw TmError(TM_E_SIZE, "InconsistentSize: a block needs at least 2 x 2 nodes (and fewer than 2^31)");
        }
        std::vector<tm_quality> rec(mesh->nblocks);
        for (uint64_t b = 0; b < mesh->nblocks; ++b) quality_block_host(mesh->blocks[b].xy, mesh->blocks[b].ni, mesh->blocks[b].nj, b, &rec[b]);
        if (per_block) std::memcpy(per_block, rec.data(), sizeof(tm_quality) * rec.size());
        if (total) quality_total(rec.data(), rec.size(), total);
        return TM_OK;
    });
}
