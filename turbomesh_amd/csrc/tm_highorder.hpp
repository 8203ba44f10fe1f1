// High-order curved elements from smoothed blocks (include/tm_hip.h, "high-order elements"): the interpolation tables, the
// contraction of one target column of an element and the element / block records, shared by the device kernel (tm_highorder.hip,
// K13) and the host definition (tm_highorder_host.cpp) so that the two evaluate the SAME sequence of IEEE fp64 operations (the library
// is built with -ffp-contract=off; divisions are the correctly rounded ones on both sides).
//
// Orientation in one pass, as in tm_quality.h: o = sign(sum of corner-cell areas) is known only when every element has been seen, so a
// record keeps both candidate sets -- elements with min J > 0 (valid for o = +1, sj = Jmin / Jmax) and elements with max J < 0 (valid
// for o = -1, sj = (-Jmax) / (-Jmin) = Jmax / Jmin bit for bit) -- and ho_finish picks the set.
#pragma once
#include "tm_quality.h"

namespace tmh {

constexpr int HO_MAX_TABLE = (TM_HO_MAX_ORDER + 1) * (TM_HO_MAX_ORDER + 1);

// validated options of one call: nodes t[0..p] and the tables T, D as (p+1) x (p+1) rows, rounded once from long double
struct HoPlan {
    int order = 0;
    int distribution = TM_HO_EQUIDISTANT;
    bool identity = false;   // TM_HO_EQUIDISTANT or p = 1: T is the identity by definition, the nodes are copied
    double nodes[TM_HO_MAX_ORDER + 1];
    double tab[2 * HO_MAX_TABLE];   // T then D, (p+1)^2 entries each, packed
    const double* T() const { return tab; }
    const double* D() const { return tab + (order + 1) * (order + 1); }
};
// throws TmError(TM_E_ARG) on any violation of the definition
HoPlan ho_plan(const tm_ho_opt* opt);
// TM_E_SIZE unless the block has elements of the plan's order (and fewer than 2^31 nodes)
void ho_check_block(const HoPlan& plan, uint64_t block, uint64_t ni, uint64_t nj);
// block `block` of the description: TM_E_ARG for a missing mesh, block or coordinates, then ho_check_block
const tm_block& ho_block_of(const tm_mesh_desc* mesh, const HoPlan& plan, uint64_t block);

// ---- one target column (e, f, b) of an element: the nodes Y[a][b] and the Jacobian extremes over a = 0 .. p.
// at(m, n) = source node X[e*p + m][f*p + n]; trow / drow = rows b of T and D; T, D the whole tables (indexed by compile-time a, m).
// W[m] = B[b][0]*X[m][0] + B[b][1]*X[m][1] + ... (in that order), R[a] = A[a][0]*W[0] + A[a][1]*W[1] + ...: the W of a column are
// formed once and serve Y, d/du and d/dv, 5(p+1) multiply-adds per component and node.
// put(a, x, y) receives the elevated node a of the column when want_y.
#if defined(__HIP_DEVICE_COMPILE__)
#define TM_HO_ROW_DONE() __builtin_amdgcn_sched_barrier(0)   // keep the next row's LDS reads behind this row's arithmetic: registers, not results
#else
#define TM_HO_ROW_DONE() ((void)0)
#endif
template <int P, class At, class Put>
TM_Q_FN void ho_column(const At& at, const double* __restrict__ trow, const double* __restrict__ drow, const double* __restrict__ T,
                       const double* __restrict__ D, bool want_y, const Put& put, double& jmin, double& jmax, bool& bad) {
    double wtx[P + 1], wty[P + 1], wdx[P + 1], wdy[P + 1];
#pragma unroll
    for (int m = 0; m <= P; ++m) {
        const QPoint v0 = at(m, 0);
        double tx = trow[0] * v0.x, ty = trow[0] * v0.y, dx = drow[0] * v0.x, dy = drow[0] * v0.y;
#pragma unroll
        for (int n = 1; n <= P; ++n) {
            const QPoint v = at(m, n);
            tx = tx + trow[n] * v.x;
            ty = ty + trow[n] * v.y;
            dx = dx + drow[n] * v.x;
            dy = dy + drow[n] * v.y;
        }
        wtx[m] = tx;
        wty[m] = ty;
        wdx[m] = dx;
        wdy[m] = dy;
        TM_HO_ROW_DONE();
    }
    const double inf = std::numeric_limits<double>::infinity();
    jmin = inf;
    jmax = -inf;
    bad = false;
#pragma unroll
    for (int a = 0; a <= P; ++a) {
        const double* Ta = T + a * (P + 1);
        const double* Da = D + a * (P + 1);
        double xu = Da[0] * wtx[0], yu = Da[0] * wty[0], xv = Ta[0] * wdx[0], yv = Ta[0] * wdy[0];
#pragma unroll
        for (int m = 1; m <= P; ++m) {
            xu = xu + Da[m] * wtx[m];
            yu = yu + Da[m] * wty[m];
            xv = xv + Ta[m] * wdx[m];
            yv = yv + Ta[m] * wdy[m];
        }
        const double J = xu * yv - xv * yu;
        bad = bad || !__builtin_isfinite(J);
        if (J < jmin) jmin = J;
        if (J > jmax) jmax = J;
        if (want_y) {
            double x = Ta[0] * wtx[0], y = Ta[0] * wty[0];
#pragma unroll
            for (int m = 1; m <= P; ++m) {
                x = x + Ta[m] * wtx[m];
                y = y + Ta[m] * wty[m];
            }
            put(a, x, y);
        }
        TM_HO_ROW_DONE();
    }
}

// the extremes of an element from those of its columns, b = 0 .. p in that order
TM_Q_FN void ho_take_column(double& jmin, double& jmax, bool& bad, double cmin, double cmax, bool cbad) {
    bad = bad || cbad;
    if (cmin < jmin) jmin = cmin;
    if (cmax > jmax) jmax = cmax;
}

// which element writes node i of a grid line with E elements of order p: a seam node belongs to the element above it (local index 0),
// the last node of the block to the last element (local index p)
TM_Q_FN bool ho_owns(int local, int p, int element, int E) { return local < p || element == E - 1; }

// area of the cell of element corners A = (e,f), B = (e+1,f), C = (e+1,f+1), D = (e,f+1): the expression of q_cell
TM_Q_FN double ho_corner_area(const QPoint& A, const QPoint& B, const QPoint& C, const QPoint& D) {
    return 0.5 * ((C.x - A.x) * (D.y - B.y) - (D.x - B.x) * (C.y - A.y));
}

// scaled Jacobian of an element for orientation o (0 reports as +1); NaN for an invalid element
TM_Q_FN double ho_sj(double jmin, double jmax, bool bad, int o) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (bad) return nan;
    if (o >= 0) return jmin > 0.0 ? jmin / jmax : nan;
    return jmax < 0.0 ? jmax / jmin : nan;
}

// What one workgroup (device) or one block (host) has seen; the element index is e*Ej + f, so "lowest (e, f)" is "lowest index".
struct HoAcc {
    unsigned long long n[2];          // valid elements for o = +1 / o = -1
    unsigned long long hist[2][10];
    double sj[2];                     // min scaled Jacobian of the set
    unsigned long long at[2];         // its element (Q_NO_CELL: none)
    double lo[2], hi[2];              // extremes of o*J over the set's elements
    double asum, aabs;                // corner-cell areas: sum and sum of |a| over all elements
};

TM_Q_FN void ho_init(HoAcc& a) {
    const double inf = std::numeric_limits<double>::infinity();
    for (int s = 0; s < 2; ++s) {
        a.n[s] = 0;
        for (int k = 0; k < 10; ++k) a.hist[s][k] = 0;
        a.sj[s] = inf;
        a.at[s] = Q_NO_CELL;
        a.lo[s] = inf;
        a.hi[s] = -inf;
    }
    a.asum = a.aabs = 0.0;
}

// a <- a combined with b; asum / aabs are added in the order of the calls (fixed on the device: k_ho_finalize)
TM_Q_FN void ho_combine(HoAcc& a, const HoAcc& b) {
    for (int s = 0; s < 2; ++s) {
        a.n[s] += b.n[s];
        for (int k = 0; k < 10; ++k) a.hist[s][k] += b.hist[s][k];
        q_take_min(a.sj[s], a.at[s], b.sj[s], b.at[s]);
        if (b.lo[s] < a.lo[s]) a.lo[s] = b.lo[s];
        if (b.hi[s] > a.hi[s]) a.hi[s] = b.hi[s];
    }
    a.asum += b.asum;
    a.aabs += b.aabs;
}

// Everything an element contributes but its histogram bin (LDS atomics on the device).  Returns set*10 + bin of a valid element, or -1.
TM_Q_FN int ho_count_element(double jmin, double jmax, bool bad, double area, unsigned long long element, HoAcc& a) {
    a.asum += area;
    a.aabs += fabs(area);
    if (bad) return -1;
    if (jmin > 0.0) {
        const double s = jmin / jmax;
        a.n[0] += 1;
        q_take_min(a.sj[0], a.at[0], s, element);
        if (jmin < a.lo[0]) a.lo[0] = jmin;
        if (jmax > a.hi[0]) a.hi[0] = jmax;
        return q_bin(s);
    }
    if (jmax < 0.0) {
        const double s = jmax / jmin;
        a.n[1] += 1;
        q_take_min(a.sj[1], a.at[1], s, element);
        if (-jmax < a.lo[1]) a.lo[1] = -jmax;
        if (-jmin > a.hi[1]) a.hi[1] = -jmin;
        return 10 + q_bin(s);
    }
    return -1;
}

TM_Q_FN void ho_finish(const HoAcc& a, uint64_t block, uint64_t Ei, uint64_t Ej, int order, tm_ho_quality* out) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const uint64_t elements = Ei * Ej;
    int o = 0;
    if (fabs(a.asum) > static_cast<double>(elements) * 0x1p-53 * a.aabs) o = a.asum > 0.0 ? 1 : -1;
    const int s = o >= 0 ? 0 : 1;
    const bool any = a.n[s] > 0;
    out->elements = elements;
    out->invalid = elements - a.n[s];
    out->orientation = o;
    out->order = order;
    out->min_scaled_jacobian = any ? a.sj[s] : nan;
    out->worst_block = any ? block : 0;
    out->worst_e = any ? a.at[s] / Ej : 0;
    out->worst_f = any ? a.at[s] % Ej : 0;
    out->min_jacobian = any ? a.lo[s] : nan;
    out->max_jacobian = any ? a.hi[s] : nan;
    for (int k = 0; k < 10; ++k) out->hist[k] = a.hist[s][k];
}

// ---- host side (tm_highorder_host.cpp)
// The definition as a plain loop over ho_column.  xy: the block, node (i,j) at i*nj + j; x, y: planes with i fastest (both NULL: report
// alone); jj, when given, receives (Jmin, Jmax) per element as jj[2*(f*Ei + e)], NaN pairs for elements with a non-finite J.
void ho_block_host(const HoPlan& plan, const double* xy, uint64_t ni, uint64_t nj, uint64_t block, double* x, double* y, tm_ho_quality* q, double* jj);
// sj[f*Ei + e] from the (Jmin, Jmax) pairs and the block's orientation
void ho_sj_from_pairs(const double* jj, uint64_t elements, int orientation, double* sj);
void ho_quality_total(const tm_ho_quality* per_block, uint64_t n, tm_ho_quality* total);

}  // namespace tmh
