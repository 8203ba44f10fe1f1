// Mesh quality report (tm_mesh_quality, tm_mesh_quality_host, tm_smoother_quality, tm_smoother_quality_field): the per-edge,
// per-cell and combine functions, shared by the device kernel (tm_quality.hip) and the host loop (tm_quality_host.cpp) so that the
// two evaluate the SAME sequence of IEEE fp64 operations (the library is built with -ffp-contract=off; divisions and square roots
// are the correctly rounded ones on both sides).  Definitions: include/tm_hip.h, "mesh quality".
//
// Orientation in one pass: a block's orientation o = sign(sum of cell areas) is known only when every cell has been seen, so a
// record keeps BOTH candidate sets -- min and max of the signed scaled Jacobian s with their cells, the counts of cells with
// min J <= 0 and with max J >= 0, one histogram per sign -- and q_finish picks the set.  min over corners of o*s is min s for
// o = +1 and -(max s) for o = -1; a cell is valid for o = +1 iff min J > 0 and for o = -1 iff max J < 0, never both.
#pragma once
#include "../../include/tm_hip.h"
#include <cstdint>
#include <cmath>
#include <limits>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TM_Q_FN __host__ __device__ inline
#else
#define TM_Q_FN inline
#endif

namespace tmh {

struct QPoint {
    double x, y;
};

constexpr unsigned long long Q_NO_CELL = ~0ull;

// What one workgroup (device) or one block (host) has seen.  Sums and counts add, extremes combine, the two argmin pairs carry
// the cell as i*(nj-1) + j, so "lowest (i, j)" is "lowest index".
struct QAcc {
    unsigned long long deg, jle0, jge0;   // degenerate cells; non-degenerate cells with min J <= 0 / with max J >= 0
    unsigned long long hist[2][10];       // [0]: cells with min J > 0 binned by min s; [1]: cells with max J < 0 binned by -(max s)
    double smin, smax;                    // over the corners of non-degenerate cells
    unsigned long long imin, imax;        // the cells that hold them (Q_NO_CELL: none)
    double cmin, cmax;                    // clamped cosine of the corner angle, non-degenerate cells
    double aspect, gi, gj;
    double amin, amax, asum, aabs;        // signed cell area: extremes over non-degenerate cells; sum and sum of |a| over all cells
};

TM_Q_FN void q_init(QAcc& a) {
    a.deg = a.jle0 = a.jge0 = 0;
    for (int s = 0; s < 2; ++s)
        for (int k = 0; k < 10; ++k) a.hist[s][k] = 0;
    const double inf = std::numeric_limits<double>::infinity();
    a.smin = inf;
    a.smax = -inf;
    a.imin = a.imax = Q_NO_CELL;
    a.cmin = inf;
    a.cmax = -inf;
    a.aspect = 0.0;   // every ratio is >= 1
    a.gi = a.gj = 1.0;
    a.amin = inf;
    a.amax = -inf;
    a.asum = a.aabs = 0.0;
}

// (value, cell) pairs: smaller value wins, ties go to the lower cell
TM_Q_FN void q_take_min(double& v, unsigned long long& i, double v2, unsigned long long i2) {
    if (v2 < v || (v2 == v && i2 < i)) {
        v = v2;
        i = i2;
    }
}
TM_Q_FN void q_take_max(double& v, unsigned long long& i, double v2, unsigned long long i2) {
    if (v2 > v || (v2 == v && i2 < i)) {
        v = v2;
        i = i2;
    }
}

// a <- a combined with b; asum / aabs are added in the order of the calls (fixed on the device: k_quality_finalize)
TM_Q_FN void q_combine(QAcc& a, const QAcc& b) {
    a.deg += b.deg;
    a.jle0 += b.jle0;
    a.jge0 += b.jge0;
    for (int s = 0; s < 2; ++s)
        for (int k = 0; k < 10; ++k) a.hist[s][k] += b.hist[s][k];
    q_take_min(a.smin, a.imin, b.smin, b.imin);
    q_take_max(a.smax, a.imax, b.smax, b.imax);
    if (b.cmin < a.cmin) a.cmin = b.cmin;
    if (b.cmax > a.cmax) a.cmax = b.cmax;
    if (b.aspect > a.aspect) a.aspect = b.aspect;
    if (b.gi > a.gi) a.gi = b.gi;
    if (b.gj > a.gj) a.gj = b.gj;
    if (b.amin < a.amin) a.amin = b.amin;
    if (b.amax > a.amax) a.amax = b.amax;
    a.asum += b.asum;
    a.aabs += b.aabs;
}

// squared length and length of the edge p -> q; (q - p)^2 == (p - q)^2 bit for bit, so an edge has ONE value whichever cell asks
TM_Q_FN void q_edge(const QPoint& p, const QPoint& q, double& l2, double& l) {
    const double dx = q.x - p.x, dy = q.y - p.y;
    l2 = dx * dx + dy * dy;
    l = sqrt(l2);
}

// growth of a pair of consecutive edges along a grid line; pairs with a zero-length edge are skipped
TM_Q_FN void q_growth(double l0, double l1, double& g) {
    if (l0 == 0.0 || l1 == 0.0) return;
    const double hi = l0 > l1 ? l0 : l1, lo = l0 > l1 ? l1 : l0;
    const double r = hi / lo;
    if (r > g) g = r;
}

TM_Q_FN int q_bin(double m) {   // m > 0: the bin k with k/10 <= m < (k+1)/10, everything from 0.9 up in bin 9
    int k = 0;
    k += m >= 1.0 / 10.0;
    k += m >= 2.0 / 10.0;
    k += m >= 3.0 / 10.0;
    k += m >= 4.0 / 10.0;
    k += m >= 5.0 / 10.0;
    k += m >= 6.0 / 10.0;
    k += m >= 7.0 / 10.0;
    k += m >= 8.0 / 10.0;
    k += m >= 9.0 / 10.0;
    return k;
}

struct QCell {
    bool degenerate;
    double jmin, jmax;   // over the four corners
    double smin, smax;   // scaled Jacobian J / sqrt(P)
    double cmin, cmax;   // cosine (u.v) / sqrt(P), clamped to [-1, 1]
    double aspect, area;
};

// One corner: u = next - corner, v = previous - corner; uu, vv their squared lengths (taken from the edges)
TM_Q_FN void q_corner(const QPoint& c, const QPoint& next, const QPoint& prev, double uu, double vv, QCell& r) {
    const double ux = next.x - c.x, uy = next.y - c.y, vx = prev.x - c.x, vy = prev.y - c.y;
    const double J = ux * vy - uy * vx;
    const double P = uu * vv;
    // no branch: a degenerate corner only marks the cell, whose extremes (whatever the divisions below make of it) are then never used
    r.degenerate = r.degenerate || P == 0.0 || !__builtin_isfinite(P) || !__builtin_isfinite(J);
    const double root = sqrt(P);
    const double s = J / root;
    double c_ = (ux * vx + uy * vy) / root;
    if (c_ > 1.0) c_ = 1.0;
    if (c_ < -1.0) c_ = -1.0;
    if (J < r.jmin) r.jmin = J;
    if (J > r.jmax) r.jmax = J;
    if (s < r.smin) r.smin = s;
    if (s > r.smax) r.smax = s;
    if (c_ < r.cmin) r.cmin = c_;
    if (c_ > r.cmax) r.cmax = c_;
}

// Cell with corners A = (i,j), B = (i+1,j), C = (i+1,j+1), D = (i,j+1); l2_* / l_* are q_edge of its four edges
TM_Q_FN QCell q_cell(const QPoint& A, const QPoint& B, const QPoint& C, const QPoint& D, double l2_ab, double l_ab, double l2_dc, double l_dc,
                     double l2_ad, double l_ad, double l2_bc, double l_bc) {
    QCell r;
    const double inf = std::numeric_limits<double>::infinity();
    r.degenerate = false;
    r.jmin = r.smin = r.cmin = inf;
    r.jmax = r.smax = r.cmax = -inf;
    q_corner(A, B, D, l2_ab, l2_ad, r);
    q_corner(B, C, A, l2_bc, l2_ab, r);
    q_corner(C, D, B, l2_dc, l2_bc, r);
    q_corner(D, A, C, l2_ad, l2_dc, r);
    r.area = 0.5 * ((C.x - A.x) * (D.y - B.y) - (D.x - B.x) * (C.y - A.y));
    const double li = l_ab + l_dc, lj = l_ad + l_bc;
    const double hi = li > lj ? li : lj, lo = li > lj ? lj : li;
    r.aspect = hi / lo;   // used for non-degenerate cells only: their four edges are all non-zero
    return r;
}

// Everything a cell contributes but its histogram bin, which the callers count their own way (LDS atomics on the device).
// Returns the (sign, bin) of a valid cell as sign*10 + bin, or -1.
TM_Q_FN int q_count_cell(const QCell& c, unsigned long long cell, QAcc& a) {
    a.asum += c.area;
    a.aabs += fabs(c.area);
    if (c.degenerate) {
        a.deg += 1;
        return -1;
    }
    q_take_min(a.smin, a.imin, c.smin, cell);
    q_take_max(a.smax, a.imax, c.smax, cell);
    if (c.cmin < a.cmin) a.cmin = c.cmin;
    if (c.cmax > a.cmax) a.cmax = c.cmax;
    if (c.aspect > a.aspect) a.aspect = c.aspect;
    if (c.area < a.amin) a.amin = c.area;
    if (c.area > a.amax) a.amax = c.area;
    a.jle0 += c.jmin <= 0.0;
    a.jge0 += c.jmax >= 0.0;
    if (c.jmin > 0.0) return q_bin(c.smin);
    if (c.jmax < 0.0) return 10 + q_bin(-c.smax);
    return -1;
}

// per-cell value of tm_smoother_quality_field for orientation o (0 reports as +1)
TM_Q_FN double q_field_value(const QCell& c, int o) {
    if (c.degenerate) return std::numeric_limits<double>::quiet_NaN();
    return o >= 0 ? c.smin : -c.smax;
}

// The record of a block from what was accumulated over its cells.  min_angle_deg / max_angle_deg leave here as the COSINES
// (largest / smallest); q_angles turns them into degrees on the host -- the device never evaluates an inverse trigonometric function.
TM_Q_FN void q_finish(const QAcc& a, uint64_t block, uint64_t ni, uint64_t nj, tm_quality* out) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const uint64_t cells = (ni - 1) * (nj - 1);
    int o = 0;
    if (fabs(a.asum) > static_cast<double>(cells) * 0x1p-53 * a.aabs) o = a.asum > 0.0 ? 1 : -1;
    const bool pos = o >= 0;
    const bool any = cells > a.deg;
    out->cells = cells;
    out->degenerate = a.deg;
    out->inverted = pos ? a.jle0 : a.jge0;
    out->orientation = o;
    out->_pad = 0;
    const unsigned long long worst = pos ? a.imin : a.imax;
    out->min_scaled_jacobian = any ? (pos ? a.smin : -a.smax) : nan;
    out->worst_block = any ? block : 0;
    out->worst_i = any ? worst / (nj - 1) : 0;
    out->worst_j = any ? worst % (nj - 1) : 0;
    out->min_angle_deg = any ? a.cmax : nan;
    out->max_angle_deg = any ? a.cmin : nan;
    out->max_aspect = any ? a.aspect : nan;
    out->max_growth_i = a.gi;
    out->max_growth_j = a.gj;
    out->min_area = any ? (pos ? a.amin : -a.amax) : nan;
    out->max_area = any ? (pos ? a.amax : -a.amin) : nan;
    out->total_area = pos ? a.asum : -a.asum;
    for (int k = 0; k < 10; ++k) out->hist[k] = a.hist[pos ? 0 : 1][k];
}

// ---- host side (tm_quality_host.cpp)
void quality_angles(tm_quality* q);   // cosines left by q_finish -> degrees (tm_refmath::acos)
// `total` from the records of the blocks; blocks with cells == 0 (not owned by the rank) are left out
void quality_total(const tm_quality* per_block, uint64_t nblocks, tm_quality* total);
void quality_block_host(const double* xy, uint64_t ni, uint64_t nj, uint64_t block, tm_quality* out);

}  // namespace tmh
