// Host side of the 3-D quality report (include/tm_hip.h, "3-D quality of stacked blocks"): tm_quality3d_planes_host and
// tm_stack_quality_host -- the definitions as a plain loop over the per-cell function the device kernel uses (tm_quality3d.h) -- and
// tm_quality3d_total.  No HIP call in this file: it works in a process without a device.
#include "tm_quality3d.h"
#include "tm_api_util.hpp"
#include "tm_stack.hpp"

#include <cstring>
#include <vector>

namespace tmh {

// cell (i, j) between the layer below (planes p*) and the layer above (planes x, y, z): its edges by q3_edge, then q3_cell
static Q3Cell cell_between(const double* px, const double* py, const double* pz, const double* x, const double* y, const double* z, uint64_t ni, uint64_t i, uint64_t j) {
    Q3Point c[8];
    for (int m = 0; m < 8; ++m) {
        const size_t o = (j + ((m >> 1) & 1)) * ni + i + (m & 1);
        c[m] = (m & 4) ? Q3Point{x[o], y[o], z[o]} : Q3Point{px[o], py[o], pz[o]};
    }
    double li[4], lj[4], lk[4];
    for (int m = 0; m < 4; ++m) {
        const int lo = m & 1, hi = m >> 1;
        li[m] = q3_edge(c[2 * lo + 4 * hi], c[1 + 2 * lo + 4 * hi]);
        lj[m] = q3_edge(c[lo + 4 * hi], c[lo + 2 + 4 * hi]);
        lk[m] = q3_edge(c[lo + 2 * hi], c[lo + 2 * hi + 4]);
    }
    return q3_cell(c, li, lj, lk);
}

Quality3dStream::Quality3dStream(uint64_t ni_, uint64_t nj_, uint64_t nk_, double* field_) : ni(ni_), nj(nj_), nk(nk_), field(field_), lk_prev(ni_ * nj_, 0.0) {
    q3_init(acc);
}

void Quality3dStream::layer(const double* x, const double* y, const double* z) {
    auto at = [&](const double* X, const double* Y, const double* Z, uint64_t i, uint64_t j) { return Q3Point{X[j * ni + i], Y[j * ni + i], Z[j * ni + i]}; };
    if (k > 0) {
        for (uint64_t j = 0; j + 1 < nj; ++j)
            for (uint64_t i = 0; i + 1 < ni; ++i) {
                const Q3Cell cell = cell_between(px, py, pz, x, y, z, ni, i, j);
                const unsigned long long id = ((k - 1) * (nj - 1) + j) * (ni - 1) + i;
                const int bin = q3_count_cell(cell, id, acc);
                if (bin >= 0) acc.hist[bin / 10][bin % 10] += 1;
                if (field) field[id] = q3_field_value(cell, 1);   // o is not known yet: tm_quality3d_planes_host rewrites the plane when it turns out -1
            }
        // growth along the spanwise lines, boundary lines included
        for (uint64_t j = 0; j < nj; ++j)
            for (uint64_t i = 0; i < ni; ++i) {
                const double l = q3_edge(at(px, py, pz, i, j), at(x, y, z, i, j));
                if (k > 1) q_growth(lk_prev[j * ni + i], l, acc.gk);
                lk_prev[j * ni + i] = l;
            }
    }
    px = x;
    py = y;
    pz = z;
    ++k;
}

void Quality3dStream::finish(uint64_t block, tm_quality3d* out) const { q3_finish(acc, block, ni, nj, nk, out); }

void quality3d_total(const tm_quality3d* pb, uint64_t nblocks, tm_quality3d* t) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::memset(t, 0, sizeof(*t));
    t->min_scaled_jacobian = t->max_aspect = t->min_volume = t->max_volume = nan;
    t->max_growth_k = 1.0;
    bool first = true;
    auto lower = [](double& a, double b) {   // NaN = no value yet
        if (b == b && !(a <= b)) a = b;
    };
    auto raise = [](double& a, double b) {
        if (b == b && !(a >= b)) a = b;
    };
    for (uint64_t b = 0; b < nblocks; ++b) {
        const tm_quality3d& q = pb[b];
        if (q.cells == 0) continue;
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
            t->worst_k = q.worst_k;
        }
        raise(t->max_aspect, q.max_aspect);
        raise(t->max_growth_k, q.max_growth_k);
        lower(t->min_volume, q.min_volume);
        raise(t->max_volume, q.max_volume);
        t->total_volume += q.total_volume;
    }
}

void stack_check_cells(const StackPlan& plan, uint64_t ni, uint64_t nj) {
    if (plan.nlayers < 2) throw TmError(TM_E_SIZE, "InconsistentSize: a stack needs at least 2 layers to have cells");
    if (ni < 2 || nj < 2) throw TmError(TM_E_SIZE, "InconsistentSize: a block needs at least 2 x 2 nodes");
}

// the per-cell values were written as for o = +1 (min s); for o = -1 they are -(max s), which the one pass did not keep: a second pass
static void field_for_negative(const double* x, const double* y, const double* z, uint64_t ni, uint64_t nj, uint64_t nk, double* field) {
    const size_t plane = static_cast<size_t>(ni) * nj;
    for (uint64_t k = 0; k + 1 < nk; ++k)
        for (uint64_t j = 0; j + 1 < nj; ++j)
            for (uint64_t i = 0; i + 1 < ni; ++i) {
                const size_t lo = k * plane, hi = (k + 1) * plane;
                field[(k * (nj - 1) + j) * (ni - 1) + i] = q3_field_value(cell_between(x + lo, y + lo, z + lo, x + hi, y + hi, z + hi, ni, i, j), -1);
            }
}

}  // namespace tmh

using namespace tmh;

extern "C" int tm_quality3d_planes_host(const double* x, const double* y, const double* z, uint64_t ni, uint64_t nj, uint64_t nk, uint64_t block,
                                        tm_quality3d* out, double* field) {
    return guarded([&]() {
        if (!x || !y || !z || !out) throw TmError(TM_E_ARG, "null argument");
        if (ni < 2 || nj < 2 || nk < 2) throw TmError(TM_E_SIZE, "InconsistentSize: a 3-D block needs at least 2 x 2 x 2 nodes");
        const size_t plane = static_cast<size_t>(ni) * nj;
        Quality3dStream s(ni, nj, nk, field);
        for (uint64_t k = 0; k < nk; ++k) s.layer(x + k * plane, y + k * plane, z + k * plane);
        s.finish(block, out);
        if (field && out->orientation < 0) field_for_negative(x, y, z, ni, nj, nk, field);
        return TM_OK;
    });
}

extern "C" int tm_stack_quality_host(const tm_mesh_desc* const* cuts, const tm_stack_opt* opt, uint64_t block, tm_quality3d* out) {
    return guarded([&]() {
        if (!out) throw TmError(TM_E_ARG, "null argument");
        const StackPlan p = stack_plan(opt);
        uint64_t ni = 0, nj = 0;
        stack_check_cuts(cuts, p.ncuts, block, &ni, &nj);
        stack_check_cells(p, ni, nj);
        const double* v[TM_STACK_MAX_CUTS];
        for (int c = 0; c < p.ncuts; ++c) v[c] = cuts[c]->blocks[block].xy;
        const size_t plane = static_cast<size_t>(ni) * nj;
        std::vector<double> buf(6 * plane);   // two layers of x, y, z, alternating
        Quality3dStream s(ni, nj, p.nlayers, nullptr);
        for (uint64_t k = 0; k < p.nlayers; ++k) {
            double* l = buf.data() + (k & 1) * 3 * plane;
            stack_layer_host(p, v, k, ni, nj, l, l + plane, l + 2 * plane);
            s.layer(l, l + plane, l + 2 * plane);
        }
        s.finish(block, out);
        return TM_OK;
    });
}

extern "C" int tm_stack_quality_surf_host(const tm_mesh_desc* const* cuts, const tm_stack_opt* opt, const tm_stack_surfaces* surfaces, uint64_t block,
                                          tm_quality3d* out) {
    return guarded([&]() {
        if (!out) throw TmError(TM_E_ARG, "null argument");
        SurfPlan sf;
        const StackPlan p = stack_plan_surf(opt, surfaces, sf);
        uint64_t ni = 0, nj = 0;
        stack_check_cuts(cuts, p.ncuts, block, &ni, &nj);
        stack_check_cells(p, ni, nj);
        const double* v[TM_STACK_MAX_CUTS];
        for (int c = 0; c < p.ncuts; ++c) v[c] = cuts[c]->blocks[block].xy;
        std::vector<double> xc, rc, thc;
        stack_surf_nodes_host(p, sf, v, ni, nj, xc, rc, thc, nullptr);
        const size_t plane = static_cast<size_t>(ni) * nj;
        std::vector<double> buf(6 * plane);   // two layers of x, y, z, alternating
        Quality3dStream s(ni, nj, p.nlayers, nullptr);
        for (uint64_t k = 0; k < p.nlayers; ++k) {
            double* l = buf.data() + (k & 1) * 3 * plane;
            stack_layer_surf_host(p, xc, rc, thc, k, ni, nj, l, l + plane, l + 2 * plane);
            s.layer(l, l + plane, l + 2 * plane);
        }
        s.finish(block, out);
        return TM_OK;
    });
}

extern "C" int tm_quality3d_total(const tm_quality3d* per_block, uint64_t n, tm_quality3d* total) {
    return guarded([&]() {
        if (!per_block || !total) throw TmError(TM_E_ARG, "null argument");
        quality3d_total(per_block, n, total);
        return TM_OK;
    });
}
