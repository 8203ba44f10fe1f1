// High-order hexahedra from stacked cuts (include/tm_hip.h, "high-order hexahedra of stacked blocks"): the contraction of one line, the
// determinant, the corner hexahedron and the element / block records, shared by the device kernel (tm_highorder3.hip, K16) and the host
// definition (tm_highorder3_host.cpp) so that the two evaluate the SAME sequence of IEEE fp64 operations (the library is built with
// -ffp-contract=off; divisions are the correctly rounded ones on both sides).
//
// Every value of the three stages -- V (span), W (j) and R (i) -- is one call of ho3_line: row[0]*f(0), then + row[n]*f(n) for
// n = 1 .. p.  Who evaluates a line, and in which order the lines are taken, is free: the device spreads them over lanes, the host loops.
// The extremes of J over an element are order-free as well (min and max of finite values; a NaN only sets the element's `bad`; the sign
// of a zero extreme never reaches a result: an extreme of 0 makes the element invalid in both candidate sets).
//
// Orientation in one pass, as in tm_highorder.hpp: a record keeps both candidate sets and ho3_finish picks one.  The accumulator is
// K13's HoAcc with the element index (g*Ej + f)*Ei + e, so "lowest (g, f, e)" is "lowest index", and the corner-hexahedron volume in the
// place of the corner-cell area; ho_count_element and ho_sj serve as they are.
#pragma once
#include "tm_highorder.hpp"
#include "tm_quality3d.h"

namespace tmh {

static_assert(TM_HO3_MAX_ORDER <= TM_HO_MAX_ORDER, "the tables are K13's");

// one line of a contraction stage: row[0]*f(0) + row[1]*f(1) + ... in that order, nothing fused
template <int P, class Get>
TM_Q_FN double ho3_line(const double* __restrict__ row, const Get& f) {
    double s = row[0] * f(0);
#pragma unroll
    for (int n = 1; n <= P; ++n) s = s + row[n] * f(n);
    return s;
}

// J = x_u (y_v z_w - y_w z_v) - x_v (y_u z_w - y_w z_u) + x_w (y_u z_v - y_v z_u), left to right
TM_Q_FN double ho3_det(const Q3Point& du, const Q3Point& dv, const Q3Point& dw) {
    return du.x * (dv.y * dw.z - dw.y * dv.z) - dv.x * (du.y * dw.z - dw.y * du.z) + dw.x * (du.y * dv.z - dv.y * du.z);
}

// running extremes of J over the nodes a lane (or the host loop) has seen of one element
struct Ho3Ext {
    double jmin, jmax;
    bool bad;
};
TM_Q_FN void ho3_ext_init(Ho3Ext& x) {
    const double inf = std::numeric_limits<double>::infinity();
    x.jmin = inf;
    x.jmax = -inf;
    x.bad = false;
}
TM_Q_FN void ho3_ext_take(Ho3Ext& x, double J) {
    x.bad = x.bad || !__builtin_isfinite(J);
    if (J < x.jmin) x.jmin = J;
    if (J > x.jmax) x.jmax = J;
}
TM_Q_FN void ho3_ext_merge(Ho3Ext& x, const Ho3Ext& y) { ho_take_column(x.jmin, x.jmax, x.bad, y.jmin, y.jmax, y.bad); }

// the record of a block from what was accumulated over its elements (HoAcc::asum / aabs hold the corner-hexahedron volumes)
TM_Q_FN void ho3_finish(const HoAcc& a, uint64_t block, uint64_t Ei, uint64_t Ej, uint64_t Eg, int order, tm_ho3_quality* out) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const uint64_t elements = Ei * Ej * Eg;
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
    out->worst_e = any ? a.at[s] % Ei : 0;
    out->worst_f = any ? (a.at[s] / Ei) % Ej : 0;
    out->worst_g = any ? a.at[s] / (Ei * Ej) : 0;
    out->min_jacobian = any ? a.lo[s] : nan;
    out->max_jacobian = any ? a.hi[s] : nan;
    for (int k = 0; k < 10; ++k) out->hist[k] = a.hist[s][k];
}

// ---- host side (tm_highorder3_host.cpp)
// ho_plan with the order limited to TM_HO3_MAX_ORDER (TM_E_ARG above it)
HoPlan ho3_plan(const tm_ho_opt* opt);
// TM_E_SIZE unless a block of ni x nj nodes and nk layers has elements of the plan's order
void ho3_check_block(const HoPlan& plan, uint64_t block, uint64_t ni, uint64_t nj);
void ho3_check_layers(const HoPlan& plan, uint64_t nk);
// TM_E_ARG unless [g_begin, g_begin + g_count) lies within the Eg span elements, and is not empty when planes are wanted
void ho3_check_window(uint64_t Eg, uint64_t g_begin, uint64_t g_count, bool planes);

// A block fed span element by span element: p+1 fine layers (planes of ni*nj doubles, i fastest) per call, the last of one call being
// the first of the next.  X, Y, Z (all or none): the planes of the window [g_begin, g_begin + g_count), g_count*p + 1 layers; jj (may be
// null): (Jmin, Jmax) per element, jj[2*((g*Ej + f)*Ei + e)], NaN pairs for elements with a non-finite J.
struct Ho3Stream {
    Ho3Stream(const HoPlan& plan, uint64_t ni, uint64_t nj, uint64_t Eg, uint64_t g_begin, uint64_t g_count, double* X, double* Y, double* Z, double* jj);
    void element_layer(uint64_t g, const double* const* fx, const double* const* fy, const double* const* fz);   // [p+1] layer pointers each
    void finish(uint64_t block, tm_ho3_quality* out) const;
    HoPlan plan;
    uint64_t ni, nj, Ei, Ej, Eg, g_begin, g_count;
    double *X, *Y, *Z, *jj;
    HoAcc acc;
};
// sj[(g*Ej + f)*Ei + e] from the pairs and the orientation: ho_sj_from_pairs (tm_highorder.hpp)
void ho3_quality_total(const tm_ho3_quality* per_block, uint64_t n, tm_ho3_quality* total);

}  // namespace tmh
