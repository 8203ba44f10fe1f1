// Certificate of high-order elements by Bezier bounds of the Jacobian (include/tm_hip.h, "high-order elements: certificate"): the
// tables, the conversion of an element to control points, the Bernstein coefficients of its Jacobian, the de Casteljau step, the
// decision of a patch and the element / block records, shared by the device kernel (tm_highorder_cert.hip, K14) and the host definition
// (tm_highorder_cert_host.cpp) so that the two evaluate the SAME sequence of IEEE fp64 operations (-ffp-contract=off).
//
// Minima and maxima are exact, so the order in which the coefficients of a patch, the patches of a level or the elements of a block are
// combined does not reach the result; every rounded quantity (control points, differences, coefficients, midpoints, the guard) is formed
// by one expression below.
#pragma once
#include "tm_highorder.hpp"

namespace tmh {

constexpr int HC_LEVELS = TM_HO_CERT_MAX_DEPTH + 1;
constexpr int HC_MAX_TAB = (TM_HO_MAX_ORDER + 1) * (TM_HO_MAX_ORDER + 1) + 2 * TM_HO_MAX_ORDER * TM_HO_MAX_ORDER + 2 * TM_HO_MAX_ORDER * (TM_HO_MAX_ORDER + 1);

// tables of one order, every entry rounded once from long double: M (p+1) x (p+1), WU 2p x p, WV 2p x (p+1), packed in that order
struct HcPlan {
    int order = 0;
    double G = 0.0;        // the guard factor G(p)
    double lambda = 0.0;   // ||M||_inf, the largest absolute row sum
    double tab[HC_MAX_TAB];
    const double* M() const { return tab; }
    const double* WU() const { return tab + (order + 1) * (order + 1); }
    const double* WV() const { return WU() + 2 * order * order; }
    int tab_size() const { return (order + 1) * (order + 1) + 2 * order * order + 2 * order * (order + 1); }
};
HcPlan hc_plan(int order);
void hc_check_depth(int max_depth);   // TM_E_ARG outside 0 .. TM_HO_CERT_MAX_DEPTH

// row[0]*v[0], then + row[k]*v[k*stride] for k = 1 .. n-1 in that order
TM_Q_FN double hc_dot(const double* row, const double* v, int stride, int n) {
    double s = row[0] * v[0];
    for (int k = 1; k < n; ++k) s = s + row[k] * v[k * stride];
    return s;
}

// Coefficient (k, l) of the Jacobian.  xu, yu: p x (p+1) (index i*(p+1) + j); xv, yv: (p+1) x p (index i*p + j).  The sum runs over i
// ascending with i' = k - i in 0 .. p; inside, over j ascending with j' = l - j in 0 .. p-1: s_i = 0 + wv*t + wv*t ..., B = 0 + wu*s_i ...
TM_Q_FN double hc_coeff(int p, int k, int l, const double* xu, const double* yu, const double* xv, const double* yv, const double* WU, const double* WV) {
    const int n1 = p + 1;
    const int ia = k - p > 0 ? k - p : 0, ib = k < p - 1 ? k : p - 1;
    const int ja = l - (p - 1) > 0 ? l - (p - 1) : 0, jb = l < p ? l : p;
    double b = 0.0;
    for (int i = ia; i <= ib; ++i) {
        const int i2 = k - i;
        double s = 0.0;
        for (int j = ja; j <= jb; ++j) {
            const int j2 = l - j;
            const double t = xu[i * n1 + j] * yv[i2 * p + j2] - yu[i * n1 + j] * xv[i2 * p + j2];
            s = s + WV[l * n1 + j] * t;
        }
        b = b + WU[k * p + i] * s;
    }
    return b;
}

TM_Q_FN double hc_mid(double a, double b) { return 0.5 * (a + b); }

// g = (G * 2^-53) * R, R = (mxu + mxv) * (myu + myv), the m's the largest |derivative coefficient| of the element.  R is
// S = mxu*myv + mxv*myu PLUS the cross products mxu*myu + mxv*myv: the rounding of the conversion is relative to the element's extent in
// both directions, so S alone does not bound it on thin cells at an angle to the axes.
TM_Q_FN double hc_guard(double G, double mxu, double myu, double mxv, double myv) { return (G * 0x1p-53) * ((mxu + mxv) * (myu + myv)); }

// What the patches of one element have shown, level by level: stat[0..4] = min over PROVEN patches of the level, stat[5..9] their max,
// stat[10..14] / stat[15..19] min / max over ALL patches of the level; bit L of inv: a patch of level L has a corner that is not
// positive (or a non-finite coefficient); bit L of und: a patch of level L is undecided.
TM_Q_FN void hc_stat_init(double* stat) {
    const double inf = std::numeric_limits<double>::infinity();
    for (int L = 0; L < HC_LEVELS; ++L) {
        stat[L] = stat[10 + L] = inf;
        stat[5 + L] = stat[15 + L] = -inf;
    }
}
// one patch of level L: mn, mx the extremes of o*B over its coefficients, bad: a corner with o*B <= 0 or any non-finite coefficient.
// write: whether this caller keeps the level's extremes (one lane of a group on the device).  Returns true iff the patch is undecided.
TM_Q_FN bool hc_visit(int L, double mn, double mx, bool bad, double g, bool write, double* stat, unsigned& inv, unsigned& und) {
    bool undecided = false;
    const bool proven = !bad && mn > g;
    if (bad)
        inv |= 1u << L;
    else if (!proven) {
        und |= 1u << L;
        undecided = true;
    }
    if (write) {
        if (proven) {
            if (mn < stat[L]) stat[L] = mn;
            if (mx > stat[5 + L]) stat[5 + L] = mx;
        }
        if (mn < stat[10 + L]) stat[10 + L] = mn;
        if (mx > stat[15 + L]) stat[15 + L] = mx;
    }
    return undecided;
}
// whether the children of an undecided patch of level L are wanted: there is depth left and no level <= L has shown the element invalid
TM_Q_FN bool hc_descend(int L, int max_depth, unsigned inv) { return L < max_depth && (inv & ((2u << L) - 1u)) == 0; }

struct HcElement {
    int status, depth;
    double lo, hi;
};
// breadth first: the first level with an invalid patch decides INVALID; else the first level without an undecided patch PROVEN; else
// UNDECIDED at max_depth.  The leaves at the deciding level D are the proven patches of the levels above and all patches of level D.
TM_Q_FN HcElement hc_decide(const double* stat, unsigned inv, unsigned und, int max_depth, double g) {
    HcElement r;
    r.status = TM_HO_UNDECIDED;
    r.depth = max_depth;
    for (int L = 0; L <= max_depth; ++L) {
        if (inv & (1u << L)) {
            r.status = TM_HO_INVALID;
            r.depth = L;
            break;
        }
        if (!(und & (1u << L))) {
            r.status = TM_HO_PROVEN;
            r.depth = L;
            break;
        }
    }
    double lo = stat[10 + r.depth], hi = stat[15 + r.depth];
    for (int L = 0; L < r.depth; ++L) {
        if (stat[L] < lo) lo = stat[L];
        if (stat[5 + L] > hi) hi = stat[5 + L];
    }
    r.lo = lo - g;
    r.hi = hi + g;
    return r;
}

// What one workgroup (device) or one block (host) has seen; the element index is e*Ej + f as in HoAcc.  Counts and minima alone: the
// order of combination does not matter.
struct HcAcc {
    unsigned long long proven, invalid, undecided, hidden;
    unsigned long long decided[HC_LEVELS];
    double sb;                        // min certified scaled-Jacobian bound over proven elements
    unsigned long long at;            // its element (Q_NO_CELL: none)
    unsigned long long first;         // lowest element that is not proven (Q_NO_CELL: none)
};
TM_Q_FN void hc_init(HcAcc& a) {
    a.proven = a.invalid = a.undecided = a.hidden = 0;
    for (int L = 0; L < HC_LEVELS; ++L) a.decided[L] = 0;
    a.sb = std::numeric_limits<double>::infinity();
    a.at = Q_NO_CELL;
    a.first = Q_NO_CELL;
}
TM_Q_FN void hc_combine(HcAcc& a, const HcAcc& b) {
    a.proven += b.proven;
    a.invalid += b.invalid;
    a.undecided += b.undecided;
    a.hidden += b.hidden;
    for (int L = 0; L < HC_LEVELS; ++L) a.decided[L] += b.decided[L];
    q_take_min(a.sb, a.at, b.sb, b.at);
    if (b.first < a.first) a.first = b.first;
}
// decided[depth] += 1 without a dynamic index (the record stays in registers on the device)
TM_Q_FN void hc_count_depth(HcAcc& a, int depth) {
    for (int L = 0; L < HC_LEVELS; ++L) a.decided[L] += L == depth ? 1u : 0u;
}
TM_Q_FN void hc_count_element(const HcElement& r, bool nodal_valid, unsigned long long element, HcAcc& a) {
    if (r.status == TM_HO_PROVEN) {
        a.proven += 1;
        hc_count_depth(a, r.depth);
        q_take_min(a.sb, a.at, r.lo / r.hi, element);
        return;
    }
    if (element < a.first) a.first = element;
    if (r.status == TM_HO_INVALID) {
        a.invalid += 1;
        hc_count_depth(a, r.depth);
        if (nodal_valid) a.hidden += 1;
    } else
        a.undecided += 1;
}
TM_Q_FN void hc_finish(const HcAcc& a, uint64_t block, uint64_t Ei, uint64_t Ej, int order, int orientation, int max_depth, tm_ho_certificate* out) {
    const bool any = a.at != Q_NO_CELL, unproven = a.first != Q_NO_CELL;
    out->elements = Ei * Ej;
    out->proven = a.proven;
    out->invalid = a.invalid;
    out->undecided = a.undecided;
    out->hidden_invalid = a.hidden;
    out->orientation = orientation;
    out->order = order;
    out->max_depth = max_depth;
    out->has_unproven = unproven ? 1 : 0;
    for (int L = 0; L < HC_LEVELS; ++L) out->decided_at[L] = a.decided[L];
    out->min_scaled_bound = any ? a.sb : std::numeric_limits<double>::quiet_NaN();
    out->worst_block = any ? block : 0;
    out->worst_e = any ? a.at / Ej : 0;
    out->worst_f = any ? a.at % Ej : 0;
    out->first_unproven_block = unproven ? block : 0;
    out->first_unproven_e = unproven ? a.first / Ej : 0;
    out->first_unproven_f = unproven ? a.first % Ej : 0;
}
// K13's nodal verdict from its (Jmin, Jmax) pair (NaN pair: a non-finite J) and the block's orientation
TM_Q_FN bool hc_nodal_valid(double jmin, double jmax, int o) { return o >= 0 ? jmin > 0.0 : jmax < 0.0; }

// ---- host side (tm_highorder_cert_host.cpp)
// jj: K13's (Jmin, Jmax) pairs, jj[2*(f*Ei + e)]; status[f*Ei + e], bounds[2*(f*Ei + e)] may be NULL
void hc_block_host(const HcPlan& plan, const double* xy, uint64_t ni, uint64_t nj, uint64_t block, int orientation, const double* jj, int max_depth,
                   tm_ho_certificate* cert, uint8_t* status, double* bounds);
void hc_certificate_total(const tm_ho_certificate* per_block, uint64_t n, tm_ho_certificate* total);

}  // namespace tmh
