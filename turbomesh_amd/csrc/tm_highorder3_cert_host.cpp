// Host side of the certificate of high-order hexahedra (include/tm_hip.h, "high-order hexahedra: certificate"): the tables from exact
// integers in long double, and the definition as a plain loop over the functions the kernel uses (tm_highorder3_cert.hpp).  No HIP call
// in this file: it works in a process without a device.
#include "tm_highorder3_cert.hpp"
#include "tm_api_util.hpp"
#include "tm_dispatch.hpp"
#include "tm_stack.hpp"

#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

namespace tmh {

void h3_check_depth(int max_depth) {
    if (max_depth < 0 || max_depth > TM_HO3_CERT_MAX_DEPTH) throw TmError(TM_E_ARG, "max_depth must be 0 .. TM_HO3_CERT_MAX_DEPTH");
}

static long long binom3(int n, int k) {
    if (k < 0 || k > n) return 0;
    long long r = 1;
    for (int i = 1; i <= k; ++i) r = r * (n - k + i) / i;   // exact at every step
    return r;
}
// w^{a,b}: (a+b+1) rows of a+1 entries
static double* product_weights(double* w, int a, int b) {
    for (int k = 0; k <= a + b; ++k)
        for (int i = 0; i <= a; ++i)
            *w++ = static_cast<double>(static_cast<long double>(binom3(a, i) * binom3(b, k - i)) / static_cast<long double>(binom3(a + b, k)));
    return w;
}

H3Plan h3_plan(int p) {
    H3Plan pl;
    pl.order = p;
    const HcPlan hc = hc_plan(p);   // M and its norm are K14's
    std::memcpy(pl.tab, hc.M(), sizeof(double) * (p + 1) * (p + 1));
    pl.lambda = hc.lambda;
    double* w = pl.tab + h3_tab_m(p);
    w = product_weights(w, p, p);
    w = product_weights(w, p - 1, p);
    w = product_weights(w, p, p - 1);
    w = product_weights(w, p - 1, 2 * p);
    w = product_weights(w, p, 2 * p - 1);
    const long double L = static_cast<long double>(pl.lambda);
    pl.G = static_cast<double>(9.0L * p * (6 * p + 20) * (L * L * L) + 99 * p + 52);
    return pl;
}

namespace {

// one element on the host: the arrays the kernel keeps in LDS
template <int P>
struct HostElement3 {
    static constexpr int N1 = P + 1, N = 3 * P, NN = h3_nn(P), ND = h3_nd(P), NF = h3_nf(P), NC = h3_nc(P);
    double d[3][NN], v[3][NN], w[3][NN], c[3][NN];
    double du[3][ND], dv[3][ND], dw[3][ND];
    double cf[3][NF];
    double patch[H3_LEVELS][NC];
    double stat[4 * HC_LEVELS];
    double g;
    unsigned inv, und;

    // at(q, m, n, l): component q of fine node (m, n, l) of the element
    template <class At>
    void coefficients(const H3Plan& pl, const At& at) {
        const H3Tab<P> t(pl.tab);
        const double* M = t.M;
        for (int q = 0; q < 3; ++q) {
            const double base = at(q, 0, 0, 0);
            for (int m = 0; m < N1; ++m)
                for (int n = 0; n < N1; ++n)
                    for (int l = 0; l < N1; ++l) d[q][(m * N1 + n) * N1 + l] = at(q, m, n, l) - base;
            for (int m = 0; m < N1; ++m)
                for (int n = 0; n < N1; ++n)
                    for (int k = 0; k < N1; ++k) v[q][(m * N1 + n) * N1 + k] = hc_dot(M + k * N1, d[q] + (m * N1 + n) * N1, 1, N1);
            for (int m = 0; m < N1; ++m)
                for (int j = 0; j < N1; ++j)
                    for (int k = 0; k < N1; ++k) w[q][(m * N1 + j) * N1 + k] = hc_dot(M + j * N1, v[q] + m * N1 * N1 + k, N1, N1);
            for (int i = 0; i < N1; ++i)
                for (int j = 0; j < N1; ++j)
                    for (int k = 0; k < N1; ++k) c[q][(i * N1 + j) * N1 + k] = hc_dot(M + i * N1, w[q] + j * N1 + k, N1 * N1, N1);
        }
        double mx[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
        auto take = [](double& m, double val) {
            if (fabs(val) > m) m = fabs(val);
        };
        for (int q = 0; q < 3; ++q) {
            for (int i = 0; i < P; ++i)
                for (int j = 0; j < N1; ++j)
                    for (int k = 0; k < N1; ++k) take(mx[q][0], du[q][(i * N1 + j) * N1 + k] = c[q][((i + 1) * N1 + j) * N1 + k] - c[q][(i * N1 + j) * N1 + k]);
            for (int i = 0; i < N1; ++i)
                for (int j = 0; j < P; ++j)
                    for (int k = 0; k < N1; ++k) take(mx[q][1], dv[q][(i * P + j) * N1 + k] = c[q][(i * N1 + j + 1) * N1 + k] - c[q][(i * N1 + j) * N1 + k]);
            for (int i = 0; i < N1; ++i)
                for (int j = 0; j < N1; ++j)
                    for (int k = 0; k < P; ++k) take(mx[q][2], dw[q][(i * N1 + j) * P + k] = c[q][(i * N1 + j) * N1 + k + 1] - c[q][(i * N1 + j) * N1 + k]);
        }
        g = h3_guard(pl.G, mx);
        for (int q = 0; q < 3; ++q) {
            const int f = (q + 1) % 3, h = (q + 2) % 3;
            for (int a = 0; a <= 2 * P; ++a)
                for (int b = 0; b < 2 * P; ++b)
                    for (int k = 0; k < 2 * P; ++k) cf[q][(a * 2 * P + b) * 2 * P + k] = h3_cofactor<P>(a, b, k, dv[f], dv[h], dw[f], dw[h], t);
        }
        for (int a = 0; a < N; ++a)
            for (int b = 0; b < N; ++b)
                for (int k = 0; k < N; ++k) patch[0][(a * N + b) * N + k] = h3_coeff<P>(a, b, k, du[0], du[1], du[2], cf[0], cf[1], cf[2], t);
    }

    bool judge(int L, double o, bool force_bad) {
        const double inf = std::numeric_limits<double>::infinity();
        double mn = inf, mxv = -inf;
        bool bad = force_bad;
        for (int ci = 0; ci < NC; ++ci) {
            const double val = o * patch[L][ci];
            if (!std::isfinite(val)) bad = true;
            if (h3_is_corner<N>(ci) && !(val > 0.0)) bad = true;
            if (val < mn) mn = val;
            if (val > mxv) mxv = val;
        }
        return hc_visit(L, mn, mxv, bad, g, true, stat, inv, und);
    }

    void child(int L, int q) {
        double* s = patch[L];
        std::memcpy(s, patch[L - 1], sizeof(double) * NC);
        for (int dir = 0; dir < 3; ++dir)
            for (int line = 0; line < N * N; ++line) h3_split<N>(s, dir, line, ((q >> dir) & 1) != 0);
    }

    void descend(int L, double o, int max_depth) {   // patch[L-1] is undecided
        for (int q = 0; q < 8; ++q) {
            child(L, q);
            if (judge(L, o, false) && hc_descend(L, max_depth, inv)) descend(L + 1, o, max_depth);
        }
    }

    template <class At>
    HcElement run(const H3Plan& pl, const At& at, int orientation, bool nodal_valid, int max_depth) {
        coefficients(pl, at);
        hc_stat_init(stat);
        inv = und = 0;
        const double o = orientation >= 0 ? 1.0 : -1.0;
        if (judge(0, o, !nodal_valid) && hc_descend(0, max_depth, inv)) descend(1, o, max_depth);
        return hc_decide(stat, inv, und, max_depth, g);
    }
};

struct Planes {
    const double* q[3];
    uint64_t ni, nj;
};

template <int P>
void block_host3(const H3Plan& pl, const Planes& X, uint64_t nk, uint64_t block, int orientation, const double* jj, int max_depth, tm_ho3_certificate* cert,
                 uint8_t* status, double* bounds) {
    const uint64_t Ei = (X.ni - 1) / P, Ej = (X.nj - 1) / P, Eg = (nk - 1) / P;
    HcAcc acc;
    hc_init(acc);
    auto el = std::make_unique<HostElement3<P>>();
    for (uint64_t g = 0; g < Eg; ++g)
        for (uint64_t f = 0; f < Ej; ++f)
            for (uint64_t e = 0; e < Ei; ++e) {
                auto at = [&](int q, int m, int n, int l) { return X.q[q][((g * P + l) * X.nj + f * P + n) * X.ni + e * P + m]; };
                const size_t out = (g * Ej + f) * Ei + e;
                const bool nodal_valid = hc_nodal_valid(jj[2 * out], jj[2 * out + 1], orientation);
                const HcElement r = el->run(pl, at, orientation, nodal_valid, max_depth);
                hc_count_element(r, nodal_valid, out, acc);
                if (status) status[out] = static_cast<uint8_t>(r.status);
                if (bounds) {
                    bounds[2 * out] = r.lo;
                    bounds[2 * out + 1] = r.hi;
                }
            }
    if (cert) h3_finish(acc, block, Ei, Ej, Eg, P, orientation, max_depth, cert);
}

template <int P>
void bezier_host3(const H3Plan& pl, const Planes& X, uint64_t e, uint64_t f, uint64_t g, double* B) {
    auto at = [&](int q, int m, int n, int l) { return X.q[q][((g * P + l) * X.nj + f * P + n) * X.ni + e * P + m]; };
    auto el = std::make_unique<HostElement3<P>>();
    el->coefficients(pl, at);
    std::memcpy(B, el->patch[0], sizeof(double) * h3_nc(P));
}

}  // namespace

void h3_block_host(const H3Plan& pl, const double* x, const double* y, const double* z, uint64_t ni, uint64_t nj, uint64_t nk, uint64_t block, int orientation,
                   const double* jj, int max_depth, tm_ho3_certificate* cert, uint8_t* status, double* bounds) {
    const Planes X{{x, y, z}, ni, nj};
    dispatch_int<1, 4>(pl.order, [&](auto P) { block_host3<P()>(pl, X, nk, block, orientation, jj, max_depth, cert, status, bounds); });
}

void h3_report_host(const HoPlan& pl, const double* x, const double* y, const double* z, uint64_t ni, uint64_t nj, uint64_t nk, uint64_t block, tm_ho3_quality* rec,
                    double* jj) {
    const uint64_t p = static_cast<uint64_t>(pl.order), Eg = (nk - 1) / p;
    const size_t plane = static_cast<size_t>(ni) * nj;
    Ho3Stream st(pl, ni, nj, Eg, 0, 0, nullptr, nullptr, nullptr, jj);
    const double *fx[TM_HO3_MAX_ORDER + 1], *fy[TM_HO3_MAX_ORDER + 1], *fz[TM_HO3_MAX_ORDER + 1];
    for (uint64_t g = 0; g < Eg; ++g) {
        for (uint64_t l = 0; l <= p; ++l) {
            fx[l] = x + (g * p + l) * plane;
            fy[l] = y + (g * p + l) * plane;
            fz[l] = z + (g * p + l) * plane;
        }
        st.element_layer(g, fx, fy, fz);
    }
    st.finish(block, rec);
}

void h3_stack_planes_host(const tm_mesh_desc* const* cuts, const tm_stack_opt* sopt, const tm_stack_surfaces* surfaces, const HoPlan& pl, uint64_t block,
                          uint64_t* ni_out, uint64_t* nj_out, uint64_t* nk_out, std::vector<double>& xyz, uint64_t* outside) {
    if (!sopt) throw TmError(TM_E_ARG, "null stack options, span or layers");
    const bool rev = sopt->mapping == TM_STACK_REVOLUTION;
    if (!rev && surfaces) throw TmError(TM_E_ARG, "meridional tables go with TM_STACK_REVOLUTION only");
    SurfPlan sf;
    const StackPlan p = rev ? stack_plan_surf(sopt, surfaces, sf) : stack_plan(sopt);
    uint64_t ni = 0, nj = 0;
    stack_check_cuts(cuts, p.ncuts, block, &ni, &nj);
    ho3_check_block(pl, block, ni, nj);
    ho3_check_layers(pl, p.nlayers);
    const double* v[TM_STACK_MAX_CUTS];
    for (int c = 0; c < p.ncuts; ++c) v[c] = cuts[c]->blocks[block].xy;
    std::vector<double> xc, rc, thc;
    if (rev) stack_surf_nodes_host(p, sf, v, ni, nj, xc, rc, thc, outside);
    const size_t plane = static_cast<size_t>(ni) * nj, n = plane * p.nlayers;
    xyz.resize(3 * n);
    for (uint64_t k = 0; k < p.nlayers; ++k) {
        double *x = xyz.data() + k * plane, *y = x + n, *z = y + n;
        if (rev) stack_layer_surf_host(p, xc, rc, thc, k, ni, nj, x, y, z);
        else stack_layer_host(p, v, k, ni, nj, x, y, z);
    }
    *ni_out = ni;
    *nj_out = nj;
    *nk_out = p.nlayers;
}

static void certificate_total3(const tm_ho3_certificate* pb, uint64_t n, tm_ho3_certificate* t) {
    std::memset(t, 0, sizeof(*t));
    t->min_scaled_bound = std::numeric_limits<double>::quiet_NaN();
    bool first = true;
    for (uint64_t b = 0; b < n; ++b) {
        const tm_ho3_certificate& c = pb[b];
        if (c.elements == 0) continue;   // a block this rank does not own
        t->elements += c.elements;
        t->proven += c.proven;
        t->invalid += c.invalid;
        t->undecided += c.undecided;
        t->hidden_invalid += c.hidden_invalid;
        for (int L = 0; L < H3_LEVELS; ++L) t->decided_at[L] += c.decided_at[L];
        if (first) {
            t->orientation = c.orientation;
            t->order = c.order;
            t->max_depth = c.max_depth;
        } else {
            if (t->orientation != c.orientation) t->orientation = 0;
            if (t->order != c.order) t->order = 0;
            if (t->max_depth != c.max_depth) t->max_depth = -1;
        }
        first = false;
        if (c.min_scaled_bound == c.min_scaled_bound && !(t->min_scaled_bound <= c.min_scaled_bound)) {   // strict: ties stay with the lower block
            t->min_scaled_bound = c.min_scaled_bound;
            t->worst_block = c.worst_block;
            t->worst_e = c.worst_e;
            t->worst_f = c.worst_f;
            t->worst_g = c.worst_g;
        }
        if (c.has_unproven && !t->has_unproven) {
            t->has_unproven = 1;
            t->first_unproven_block = c.first_unproven_block;
            t->first_unproven_e = c.first_unproven_e;
            t->first_unproven_f = c.first_unproven_f;
            t->first_unproven_g = c.first_unproven_g;
        }
    }
}

// the certificate of a block given as planes, sizes already checked
static void certify_planes(const HoPlan& ho, const double* x, const double* y, const double* z, uint64_t ni, uint64_t nj, uint64_t nk, int max_depth, uint64_t block,
                           tm_ho3_certificate* cert, uint8_t* status, double* bounds) {
    const uint64_t p = static_cast<uint64_t>(ho.order);
    const size_t elements = static_cast<size_t>((ni - 1) / p) * ((nj - 1) / p) * ((nk - 1) / p);
    std::vector<double> jj(2 * elements);
    tm_ho3_quality rec;
    h3_report_host(ho, x, y, z, ni, nj, nk, block, &rec, jj.data());   // K16's report: the orientation and the nodal verdicts
    h3_block_host(h3_plan(ho.order), x, y, z, ni, nj, nk, block, rec.orientation, jj.data(), max_depth, cert, status, bounds);
}

}  // namespace tmh

using namespace tmh;

extern "C" int tm_ho3_certify_tables(const tm_ho_opt* opt, double* M, double* wA, double* wB, double* G, double* norm) {
    return guarded([&]() {
        const HoPlan ho = ho3_plan(opt);
        const H3Plan pl = h3_plan(ho.order);
        const int p = pl.order;
        if (M) std::memcpy(M, pl.M(), sizeof(double) * h3_tab_m(p));
        if (wA) std::memcpy(wA, pl.WA(), sizeof(double) * h3_tab_a(p));
        if (wB) std::memcpy(wB, pl.WB(), sizeof(double) * h3_tab_b(p));
        if (G) *G = pl.G;
        if (norm) *norm = pl.lambda;
        return TM_OK;
    });
}

extern "C" int tm_ho3_jacobian_bezier_host(const double* x, const double* y, const double* z, uint64_t ni, uint64_t nj, uint64_t nk, const tm_ho_opt* opt, uint64_t e,
                                           uint64_t f, uint64_t g, double* B) {
    return guarded([&]() {
        if (!x || !y || !z || !B) throw TmError(TM_E_ARG, "null argument");
        const HoPlan ho = ho3_plan(opt);
        ho3_check_block(ho, 0, ni, nj);
        ho3_check_layers(ho, nk);
        const uint64_t p = static_cast<uint64_t>(ho.order);
        if (e >= (ni - 1) / p || f >= (nj - 1) / p || g >= (nk - 1) / p) throw TmError(TM_E_ARG, "element index past the block");
        const H3Plan pl = h3_plan(ho.order);
        const Planes X{{x, y, z}, ni, nj};
        dispatch_int<1, 4>(ho.order, [&](auto P) { bezier_host3<P()>(pl, X, e, f, g, B); });
        return TM_OK;
    });
}

extern "C" int tm_ho3_certify_planes_host(const double* x, const double* y, const double* z, uint64_t ni, uint64_t nj, uint64_t nk, const tm_ho_opt* opt,
                                          int32_t max_depth, uint64_t block, tm_ho3_certificate* cert, uint8_t* status, double* bounds) {
    return guarded([&]() {
        if (!x || !y || !z) throw TmError(TM_E_ARG, "null argument");
        const HoPlan ho = ho3_plan(opt);
        h3_check_depth(max_depth);
        ho3_check_block(ho, block, ni, nj);
        ho3_check_layers(ho, nk);
        certify_planes(ho, x, y, z, ni, nj, nk, max_depth, block, cert, status, bounds);
        return TM_OK;
    });
}

extern "C" int tm_stack_certify_host(const tm_mesh_desc* const* cuts, const tm_stack_opt* sopt, const tm_stack_surfaces* surfaces, const tm_ho_opt* opt,
                                     int32_t max_depth, uint64_t block, tm_ho3_certificate* cert, uint8_t* status, double* bounds, uint64_t* outside) {
    return guarded([&]() {
        const HoPlan ho = ho3_plan(opt);
        h3_check_depth(max_depth);
        uint64_t ni = 0, nj = 0, nk = 0;
        std::vector<double> xyz;
        h3_stack_planes_host(cuts, sopt, surfaces, ho, block, &ni, &nj, &nk, xyz, outside);
        const size_t n = static_cast<size_t>(ni) * nj * nk;
        certify_planes(ho, xyz.data(), xyz.data() + n, xyz.data() + 2 * n, ni, nj, nk, max_depth, block, cert, status, bounds);
        return TM_OK;
    });
}

extern "C" int tm_ho3_certificate_total(const tm_ho3_certificate* per_block, uint64_t n, tm_ho3_certificate* total) {
    return guarded([&]() {
        if (!total || (n && !per_block)) throw TmError(TM_E_ARG, "null argument");
        certificate_total3(per_block, n, total);
        return TM_OK;
    });
}
