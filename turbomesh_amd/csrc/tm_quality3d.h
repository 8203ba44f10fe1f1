// 3-D quality of stacked blocks (tm_quality3d_planes_host, tm_stack_quality*, include/tm_hip.h "3-D quality of stacked blocks"): the
// per-edge, per-corner, per-cell and combine functions, shared by the device kernel (tm_stack_quality.hip, K12) and the host loop
// (tm_quality3d_host.cpp) so that the two evaluate the SAME sequence of IEEE fp64 operations, exactly as tm_quality.h does in 2-D (the
// library is built with -ffp-contract=off; divisions and square roots are the correctly rounded ones on both sides).
//
// Orientation in one pass, as in tm_quality.h: o = sign(sum of cell volumes) is known only when every cell has been seen, so a record
// keeps BOTH candidate sets and q3_finish picks one.
#pragma once
#include "tm_quality.h"
#include <vector>

namespace tmh {

struct Q3Point {
    double x, y, z;
};

// What one workgroup (device) or one block (host) has seen.  The argmin pairs carry the cell as (k*(nj-1) + j)*(ni-1) + i, so "lowest
// (k, j, i)" is "lowest index".
struct Q3Acc {
    unsigned long long deg, jle0, jge0;   // degenerate cells; non-degenerate cells with min J <= 0 / with max J >= 0
    unsigned long long hist[2][10];       // [0]: cells with min J > 0 binned by min s; [1]: cells with max J < 0 binned by -(max s)
    double smin, smax;                    // over the corners of non-degenerate cells
    unsigned long long imin, imax;        // the cells that hold them (Q_NO_CELL: none)
    double aspect, gk;
    double vmin, vmax, vsum, vabs;        // signed cell volume: extremes over non-degenerate cells; sum and sum of |V| over all cells
};

TM_Q_FN void q3_init(Q3Acc& a) {
    a.deg = a.jle0 = a.jge0 = 0;
    for (int s = 0; s < 2; ++s)
        for (int k = 0; k < 10; ++k) a.hist[s][k] = 0;
    const double inf = std::numeric_limits<double>::infinity();
    a.smin = inf;
    a.smax = -inf;
    a.imin = a.imax = Q_NO_CELL;
    a.aspect = 0.0;   // every ratio is >= 1
    a.gk = 1.0;
    a.vmin = inf;
    a.vmax = -inf;
    a.vsum = a.vabs = 0.0;
}

// a <- a combined with b; vsum / vabs are added in the order of the calls (fixed on the device: k_stack_quality_finalize)
TM_Q_FN void q3_combine(Q3Acc& a, const Q3Acc& b) {
    a.deg += b.deg;
    a.jle0 += b.jle0;
    a.jge0 += b.jge0;
    for (int s = 0; s < 2; ++s)
        for (int k = 0; k < 10; ++k) a.hist[s][k] += b.hist[s][k];
    q_take_min(a.smin, a.imin, b.smin, b.imin);
    q_take_max(a.smax, a.imax, b.smax, b.imax);
    if (b.aspect > a.aspect) a.aspect = b.aspect;
    if (b.gk > a.gk) a.gk = b.gk;
    if (b.vmin < a.vmin) a.vmin = b.vmin;
    if (b.vmax > a.vmax) a.vmax = b.vmax;
    a.vsum += b.vsum;
    a.vabs += b.vabs;
}

// length of the edge p -> q; (q - p)^2 == (p - q)^2 bit for bit, so an edge has ONE value whichever cell asks
TM_Q_FN double q3_edge(const Q3Point& p, const Q3Point& q) {
    const double dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
    const double l2 = dx * dx + dy * dy + dz * dz;
    return sqrt(l2);
}

// det[p, q, r] = p . (q x r), parenthesised as the header writes it
TM_Q_FN double q3_det(const Q3Point& p, const Q3Point& q, const Q3Point& r) {
    return p.x * (q.y * r.z - q.z * r.y) + p.y * (q.z * r.x - q.x * r.z) + p.z * (q.x * r.y - q.y * r.x);
}
TM_Q_FN Q3Point q3_sub(const Q3Point& a, const Q3Point& b) { return Q3Point{a.x - b.x, a.y - b.y, a.z - b.z}; }
TM_Q_FN Q3Point q3_add(const Q3Point& a, const Q3Point& b) { return Q3Point{a.x + b.x, a.y + b.y, a.z + b.z}; }

// exact volume of the trilinear hexahedron with corners x[a + 2b + 4c] (also the corner hexahedron of a high-order element: tm_highorder3.hpp)
TM_Q_FN double q3_volume(const Q3Point* x) {
    const Q3Point d71 = q3_sub(x[7], x[1]), d60 = q3_sub(x[6], x[0]), d72 = q3_sub(x[7], x[2]), d30 = q3_sub(x[3], x[0]), d50 = q3_sub(x[5], x[0]),
                  d74 = q3_sub(x[7], x[4]);
    const double v12 = (q3_det(q3_add(d71, d60), d72, d30) + q3_det(d60, q3_add(d72, d50), d74)) + q3_det(d71, d50, q3_add(d74, d30));
    return v12 / 12.0;
}

struct Q3Cell {
    bool degenerate;
    double jmin, jmax;   // over the eight corners
    double smin, smax;   // scaled Jacobian J / ((lu*lv)*lw)
    double aspect, volume;
};

// One corner.  u, v, w: the edge vectors along i, j, k that meet in it, each running from its lower to its upper node -- which IS the
// edge leaving corner (a, b, c) multiplied by (1-2a), (1-2b), (1-2c): IEEE subtraction is antisymmetric and the negation exact.
TM_Q_FN void q3_corner(const Q3Point& u, const Q3Point& v, const Q3Point& w, double lu, double lv, double lw, Q3Cell& r) {
    const double J = q3_det(u, v, w);
    const double P = (lu * lv) * lw;
    // no branch: a degenerate corner only marks the cell, whose extremes (whatever the division below makes of it) are then never used
    r.degenerate = r.degenerate || P == 0.0 || !__builtin_isfinite(P) || !__builtin_isfinite(J);
    const double s = J / P;
    if (J < r.jmin) r.jmin = J;
    if (J > r.jmax) r.jmax = J;
    if (s < r.smin) r.smin = s;
    if (s > r.smax) r.smax = s;
}

// Cell with corners x[a + 2b + 4c] = node (i+a, j+b, k+c).  Edge lengths: li[b + 2c] of the i-edge x[2b+4c] -> x[1+2b+4c], lj[a + 2c] of
// the j-edge x[a+4c] -> x[a+2+4c], lk[a + 2b] of the k-edge x[a+2b] -> x[a+2b+4].
TM_Q_FN Q3Cell q3_cell(const Q3Point* x, const double* li, const double* lj, const double* lk) {
    Q3Cell r;
    const double inf = std::numeric_limits<double>::infinity();
    r.degenerate = false;
    r.jmin = r.smin = inf;
    r.jmax = r.smax = -inf;
    Q3Point ei[4], ej[4], ek[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int lo = m & 1, hi = m >> 1;
        ei[m] = q3_sub(x[1 + 2 * lo + 4 * hi], x[2 * lo + 4 * hi]);
        ej[m] = q3_sub(x[lo + 2 + 4 * hi], x[lo + 4 * hi]);
        ek[m] = q3_sub(x[lo + 2 * hi + 4], x[lo + 2 * hi]);
    }
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int a = 0; a < 2; ++a) q3_corner(ei[b + 2 * c], ej[a + 2 * c], ek[a + 2 * b], li[b + 2 * c], lj[a + 2 * c], lk[a + 2 * b], r);
    r.volume = q3_volume(x);
    const double Li = ((li[0] + li[1]) + li[2]) + li[3], Lj = ((lj[0] + lj[1]) + lj[2]) + lj[3], Lk = ((lk[0] + lk[1]) + lk[2]) + lk[3];
    double hi = Li > Lj ? Li : Lj, lo = Li > Lj ? Lj : Li;
    hi = Lk > hi ? Lk : hi;
    lo = Lk < lo ? Lk : lo;
    r.aspect = hi / lo;   // used for non-degenerate cells only: their twelve edges are all non-zero
    return r;
}

// Everything a cell contributes but its histogram bin, which the callers count their own way (LDS atomics on the device).
// Returns the (sign, bin) of a valid cell as sign*10 + bin, or -1.
TM_Q_FN int q3_count_cell(const Q3Cell& c, unsigned long long cell, Q3Acc& a) {
    a.vsum += c.volume;
    a.vabs += fabs(c.volume);
    if (c.degenerate) {
        a.deg += 1;
        return -1;
    }
    q_take_min(a.smin, a.imin, c.smin, cell);
    q_take_max(a.smax, a.imax, c.smax, cell);
    if (c.aspect > a.aspect) a.aspect = c.aspect;
    if (c.volume < a.vmin) a.vmin = c.volume;
    if (c.volume > a.vmax) a.vmax = c.volume;
    a.jle0 += c.jmin <= 0.0;
    a.jge0 += c.jmax >= 0.0;
    if (c.jmin > 0.0) return q_bin(c.smin);
    if (c.jmax < 0.0) return 10 + q_bin(-c.smax);
    return -1;
}

// per-cell value of tm_stack_smoothers_quality_field for orientation o (0 reports as +1)
TM_Q_FN double q3_field_value(const Q3Cell& c, int o) {
    if (c.degenerate) return std::numeric_limits<double>::quiet_NaN();
    return o >= 0 ? c.smin : -c.smax;
}

// The record of a block from what was accumulated over its cells.
TM_Q_FN void q3_finish(const Q3Acc& a, uint64_t block, uint64_t ni, uint64_t nj, uint64_t nk, tm_quality3d* out) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const uint64_t cells = (ni - 1) * (nj - 1) * (nk - 1);
    int o = 0;
    if (fabs(a.vsum) > static_cast<double>(cells) * 0x1p-53 * a.vabs) o = a.vsum > 0.0 ? 1 : -1;
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
    out->worst_i = any ? worst % (ni - 1) : 0;
    out->worst_j = any ? (worst / (ni - 1)) % (nj - 1) : 0;
    out->worst_k = any ? worst / ((ni - 1) * (nj - 1)) : 0;
    out->max_aspect = any ? a.aspect : nan;
    out->max_growth_k = a.gk;
    out->min_volume = any ? (pos ? a.vmin : -a.vmax) : nan;
    out->max_volume = any ? (pos ? a.vmax : -a.vmin) : nan;
    out->total_volume = pos ? a.vsum : -a.vsum;
    for (int k = 0; k < 10; ++k) out->hist[k] = a.hist[pos ? 0 : 1][k];
}

// ---- host side (tm_quality3d_host.cpp)
// `total` from the records of the blocks; records with cells == 0 are left out
void quality3d_total(const tm_quality3d* per_block, uint64_t nblocks, tm_quality3d* total);

// A block fed layer by layer (planes of ni*nj doubles, i fastest): the host evaluation holds two layers at a time.
struct Quality3dStream {
    Quality3dStream(uint64_t ni, uint64_t nj, uint64_t nk, double* field);
    void layer(const double* x, const double* y, const double* z);   // call nk times, in order; the planes of the previous call must still be valid
    void finish(uint64_t block, tm_quality3d* out) const;
    uint64_t ni, nj, nk, k = 0;
    double* field;   // may be null
    const double *px = nullptr, *py = nullptr, *pz = nullptr;
    std::vector<double> lk_prev;   // length of the k-edge below every node of the previous layer (growth pairs)
    Q3Acc acc;
};

}  // namespace tmh
