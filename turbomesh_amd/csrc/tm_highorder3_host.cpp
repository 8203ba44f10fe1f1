// Host side of the high-order hexahedra (include/tm_hip.h, "high-order hexahedra of stacked blocks"): validation, tm_ho3_check, and the
// definition as plain loops over the line function the kernel uses (tm_highorder3.hpp) -- tm_ho3_planes_host on any 3-D block,
// tm_stack_elevate_host on K cuts with p+1 fine layers held at a time.  No HIP call in this file: it works in a process without a device.
#include "tm_highorder3.hpp"
#include "tm_api_util.hpp"
#include "tm_dispatch.hpp"
#include "tm_stack.hpp"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace tmh {

HoPlan ho3_plan(const tm_ho_opt* opt) {
    if (!opt) throw TmError(TM_E_ARG, "null high-order options");
    if (opt->order > TM_HO3_MAX_ORDER)
        throw TmError(TM_E_ARG, "hexahedra take the orders 1 .. TM_HO3_MAX_ORDER: the (p+1)^3 working set of an element does not fit above");
    return ho_plan(opt);
}

void ho3_check_block(const HoPlan& pl, uint64_t block, uint64_t ni, uint64_t nj) { ho_check_block(pl, block, ni, nj); }

void ho3_check_layers(const HoPlan& pl, uint64_t nk) {
    const uint64_t p = static_cast<uint64_t>(pl.order);
    if (nk < p + 1 || (nk - 1) % p != 0 || nk >= (uint64_t{1} << 31))
        throw TmError(TM_E_SIZE, "InconsistentSize: " + std::to_string(nk) + " layers: the layer count minus one must be a positive multiple of the order " + std::to_string(p));
}

void ho3_check_window(uint64_t Eg, uint64_t g_begin, uint64_t g_count, bool planes) {
    if (planes && g_count < 1) throw TmError(TM_E_ARG, "planes need a window of at least one span element");
    if (g_begin > Eg || g_count > Eg - g_begin) throw TmError(TM_E_ARG, "the window of span elements reaches past the block");
}

Ho3Stream::Ho3Stream(const HoPlan& pl, uint64_t ni_, uint64_t nj_, uint64_t Eg_, uint64_t g_begin_, uint64_t g_count_, double* X_, double* Y_, double* Z_, double* jj_)
    : plan(pl), ni(ni_), nj(nj_), Ei((ni_ - 1) / pl.order), Ej((nj_ - 1) / pl.order), Eg(Eg_), g_begin(g_begin_), g_count(g_count_), X(X_), Y(Y_), Z(Z_), jj(jj_) {
    ho_init(acc);
}

template <int P>
static void element_layer_host(Ho3Stream& s, uint64_t g, const double* const* fx, const double* const* fy, const double* const* fz) {
    constexpr int N = P + 1;
    const HoPlan& pl = s.plan;
    const double *T = pl.T(), *D = pl.D();
    const uint64_t ni = s.ni, nj = s.nj;
    const size_t plane = static_cast<size_t>(ni) * nj;
    const int Ei = static_cast<int>(s.Ei), Ej = static_cast<int>(s.Ej);
    const bool store = s.X && g >= s.g_begin && g < s.g_begin + s.g_count;
    const int gs = static_cast<int>(g - s.g_begin), gc = static_cast<int>(s.g_count);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const double* const* fin[3] = {fx, fy, fz};
    double* const out[3] = {s.X, s.Y, s.Z};
    if (store && pl.identity)
        for (int l = 0; l < N; ++l)
            if (ho_owns(l, P, gs, gc))
                for (int q = 0; q < 3; ++q) std::memcpy(out[q] + (static_cast<size_t>(gs) * P + l) * plane, fin[q][l], sizeof(double) * plane);
    const bool want_y = store && !pl.identity;
    // per component q: Vt, Vd [m][n][c]; Wtt, Wdt, Wtd [m][b][c]
    static thread_local std::vector<double> buf;
    buf.resize(static_cast<size_t>(3) * 5 * N * N * N);
    auto at = [&](int q, int kind, int m, int n, int c) -> double& { return buf[(((static_cast<size_t>(q) * 5 + kind) * N + m) * N + n) * N + c]; };
    for (int f = 0; f < Ej; ++f)
        for (int e = 0; e < Ei; ++e) {
            const size_t base = static_cast<size_t>(f) * P * ni + static_cast<size_t>(e) * P;
            for (int q = 0; q < 3; ++q) {
                for (int m = 0; m < N; ++m)
                    for (int n = 0; n < N; ++n) {
                        auto F = [&](int l) { return fin[q][l][base + static_cast<size_t>(n) * ni + m]; };
                        for (int c = 0; c < N; ++c) {
                            at(q, 0, m, n, c) = ho3_line<P>(T + c * N, F);
                            at(q, 1, m, n, c) = ho3_line<P>(D + c * N, F);
                        }
                    }
                for (int m = 0; m < N; ++m)
                    for (int b = 0; b < N; ++b)
                        for (int c = 0; c < N; ++c) {
                            auto Vt = [&](int n) { return at(q, 0, m, n, c); };
                            auto Vd = [&](int n) { return at(q, 1, m, n, c); };
                            const double wtt = ho3_line<P>(T + b * N, Vt), wdt = ho3_line<P>(D + b * N, Vt), wtd = ho3_line<P>(T + b * N, Vd);
                            at(q, 2, m, b, c) = wtt;
                            at(q, 3, m, b, c) = wdt;
                            at(q, 4, m, b, c) = wtd;
                        }
            }
            Ho3Ext ext;
            ho3_ext_init(ext);
            for (int c = 0; c < N; ++c)
                for (int b = 0; b < N; ++b)
                    for (int a = 0; a < N; ++a) {
                        double r[3][4];   // per component: Y, d/du, d/dv, d/dw
                        for (int q = 0; q < 3; ++q) {
                            auto Wtt = [&](int m) { return at(q, 2, m, b, c); };
                            auto Wdt = [&](int m) { return at(q, 3, m, b, c); };
                            auto Wtd = [&](int m) { return at(q, 4, m, b, c); };
                            r[q][1] = ho3_line<P>(D + a * N, Wtt);
                            r[q][2] = ho3_line<P>(T + a * N, Wdt);
                            r[q][3] = ho3_line<P>(T + a * N, Wtd);
                            if (want_y) r[q][0] = ho3_line<P>(T + a * N, Wtt);
                        }
                        ho3_ext_take(ext, ho3_det(Q3Point{r[0][1], r[1][1], r[2][1]}, Q3Point{r[0][2], r[1][2], r[2][2]}, Q3Point{r[0][3], r[1][3], r[2][3]}));
                        if (want_y && ho_owns(a, P, e, Ei) && ho_owns(b, P, f, Ej) && ho_owns(c, P, gs, gc)) {
                            const size_t o = (static_cast<size_t>(gs) * P + c) * plane + (static_cast<size_t>(f) * P + b) * ni + static_cast<size_t>(e) * P + a;
                            for (int q = 0; q < 3; ++q) out[q][o] = r[q][0];
                        }
                    }
            Q3Point x[8];
            for (int k = 0; k < 8; ++k) {
                const size_t o = base + static_cast<size_t>((k >> 1) & 1) * P * ni + static_cast<size_t>(k & 1) * P;
                const int l = (k >> 2) * P;
                x[k] = Q3Point{fx[l][o], fy[l][o], fz[l][o]};
            }
            const double vol = q3_volume(x);
            const unsigned long long el = (static_cast<unsigned long long>(g) * Ej + f) * Ei + e;
            const int bin = ho_count_element(ext.jmin, ext.jmax, ext.bad, vol, el, s.acc);
            if (bin >= 0) s.acc.hist[bin / 10][bin % 10] += 1;
            if (s.jj) {
                s.jj[2 * el] = ext.bad ? nan : ext.jmin;
                s.jj[2 * el + 1] = ext.bad ? nan : ext.jmax;
            }
        }
}

void Ho3Stream::element_layer(uint64_t g, const double* const* fx, const double* const* fy, const double* const* fz) {
    dispatch_int<1, 4>(plan.order, [&](auto P) { element_layer_host<P()>(*this, g, fx, fy, fz); });
}

void Ho3Stream::finish(uint64_t block, tm_ho3_quality* out) const { ho3_finish(acc, block, Ei, Ej, Eg, plan.order, out); }

void ho3_quality_total(const tm_ho3_quality* pb, uint64_t n, tm_ho3_quality* t) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::memset(t, 0, sizeof(*t));
    t->min_scaled_jacobian = t->min_jacobian = t->max_jacobian = nan;
    bool first = true;
    for (uint64_t b = 0; b < n; ++b) {
        const tm_ho3_quality& q = pb[b];
        if (q.elements == 0) continue;   // a block this rank does not own
        t->elements += q.elements;
        t->invalid += q.invalid;
        for (int k = 0; k < 10; ++k) t->hist[k] += q.hist[k];
        if (first) {
            t->orientation = q.orientation;
            t->order = q.order;
        } else {
            if (t->orientation != q.orientation) t->orientation = 0;
            if (t->order != q.order) t->order = 0;
        }
        first = false;
        if (q.min_scaled_jacobian == q.min_scaled_jacobian && !(t->min_scaled_jacobian <= q.min_scaled_jacobian)) {   // strict: ties stay with the lower block
            t->min_scaled_jacobian = q.min_scaled_jacobian;
            t->worst_block = q.worst_block;
            t->worst_e = q.worst_e;
            t->worst_f = q.worst_f;
            t->worst_g = q.worst_g;
        }
        if (q.min_jacobian == q.min_jacobian && !(t->min_jacobian <= q.min_jacobian)) t->min_jacobian = q.min_jacobian;
        if (q.max_jacobian == q.max_jacobian && !(t->max_jacobian >= q.max_jacobian)) t->max_jacobian = q.max_jacobian;
    }
}

// what tm_stack_elevate, tm_stack_elevate_host and tm_stack_smoothers_elevate check alike once the block's size is known
static void check_outputs(double* x, double* y, double* z) {
    if ((x == nullptr) != (y == nullptr) || (x == nullptr) != (z == nullptr)) throw TmError(TM_E_ARG, "x, y and z come together");
}

}  // namespace tmh

using namespace tmh;

extern "C" int tm_ho3_check(const tm_mesh_desc* cut0, const tm_stack_opt* sopt, const tm_ho_opt* opt) {
    return guarded([&]() {
        const HoPlan pl = ho3_plan(opt);
        if (!sopt) throw TmError(TM_E_ARG, "null stack options");
        if (!cut0 || !cut0->blocks || cut0->nblocks == 0) throw TmError(TM_E_ARG, "mesh description without blocks");
        if (cut0->nconns && !cut0->conns) throw TmError(TM_E_ARG, "null connection array");
        for (uint64_t b = 0; b < cut0->nblocks; ++b) ho3_check_block(pl, b, cut0->blocks[b].ni, cut0->blocks[b].nj);
        const uint64_t p = static_cast<uint64_t>(pl.order);
        for (uint64_t c = 0; c < cut0->nconns; ++c)
            for (int s = 0; s < 2; ++s) {
                const tm_range& r = cut0->conns[c].r[s];
                if (r.start % p != 0 || r.end % p != 0)
                    throw TmError(TM_E_SIZE, "InconsistentSize: connection " + std::to_string(c) + " range " + std::to_string(s) + " (block " + std::to_string(r.block) +
                                                 ", nodes " + std::to_string(r.start) + " .. " + std::to_string(r.end) + ") does not lie on the element grid of order " +
                                                 std::to_string(p));
            }
        ho3_check_layers(pl, sopt->nlayers);
        return TM_OK;
    });
}

extern "C" int tm_ho3_planes_host(const double* x, const double* y, const double* z, uint64_t ni, uint64_t nj, uint64_t nk, const tm_ho_opt* opt, uint64_t block,
                                  double* X, double* Y, double* Z, tm_ho3_quality* q, double* sj) {
    return guarded([&]() {
        if (!x || !y || !z) throw TmError(TM_E_ARG, "null argument");
        check_outputs(X, Y, Z);
        const HoPlan pl = ho3_plan(opt);
        ho3_check_block(pl, block, ni, nj);
        ho3_check_layers(pl, nk);
        const uint64_t p = static_cast<uint64_t>(pl.order), Eg = (nk - 1) / p;
        const size_t plane = static_cast<size_t>(ni) * nj, elements = static_cast<size_t>((ni - 1) / p) * ((nj - 1) / p) * Eg;
        std::vector<double> jj(sj ? 2 * elements : 0);
        Ho3Stream st(pl, ni, nj, Eg, 0, X ? Eg : 0, X, Y, Z, sj ? jj.data() : nullptr);
        const double *fx[TM_HO3_MAX_ORDER + 1], *fy[TM_HO3_MAX_ORDER + 1], *fz[TM_HO3_MAX_ORDER + 1];
        for (uint64_t g = 0; g < Eg; ++g) {
            for (uint64_t l = 0; l <= p; ++l) {
                fx[l] = x + (g * p + l) * plane;
                fy[l] = y + (g * p + l) * plane;
                fz[l] = z + (g * p + l) * plane;
            }
            st.element_layer(g, fx, fy, fz);
        }
        tm_ho3_quality rec;
        st.finish(block, &rec);
        if (sj) ho_sj_from_pairs(jj.data(), elements, rec.orientation, sj);
        if (q) *q = rec;
        return TM_OK;
    });
}

extern "C" int tm_stack_elevate_host(const tm_mesh_desc* const* cuts, const tm_stack_opt* sopt, const tm_stack_surfaces* surfaces, const tm_ho_opt* opt, uint64_t block,
                                     uint64_t g_begin, uint64_t g_count, double* x, double* y, double* z, tm_ho3_quality* q, double* sj, uint64_t* outside) {
    return guarded([&]() {
        check_outputs(x, y, z);
        if (!sopt) throw TmError(TM_E_ARG, "null stack options, span or layers");
        const bool rev = sopt->mapping == TM_STACK_REVOLUTION;
        if (!rev && surfaces) throw TmError(TM_E_ARG, "meridional tables go with TM_STACK_REVOLUTION only");
        SurfPlan sf;
        const StackPlan p = rev ? stack_plan_surf(sopt, surfaces, sf) : stack_plan(sopt);
        uint64_t ni = 0, nj = 0;
        stack_check_cuts(cuts, p.ncuts, block, &ni, &nj);
        const HoPlan pl = ho3_plan(opt);
        ho3_check_block(pl, block, ni, nj);
        ho3_check_layers(pl, p.nlayers);
        const uint64_t P = static_cast<uint64_t>(pl.order), Eg = (p.nlayers - 1) / P;
        ho3_check_window(Eg, g_begin, g_count, x != nullptr);
        const double* v[TM_STACK_MAX_CUTS];
        for (int c = 0; c < p.ncuts; ++c) v[c] = cuts[c]->blocks[block].xy;
        std::vector<double> xc, rc, thc;
        if (rev) stack_surf_nodes_host(p, sf, v, ni, nj, xc, rc, thc, outside);
        const size_t plane = static_cast<size_t>(ni) * nj, elements = static_cast<size_t>((ni - 1) / P) * ((nj - 1) / P) * Eg;
        const bool whole = q || sj;   // the record and sj cover the block; without them only the window is evaluated
        const uint64_t g0 = whole ? 0 : g_begin, g1 = whole ? Eg : g_begin + g_count;
        std::vector<double> jj(sj ? 2 * elements : 0);
        Ho3Stream st(pl, ni, nj, Eg, g_begin, g_count, x, y, z, sj ? jj.data() : nullptr);
        // p+1 fine layers at a time: layer slot (k % (p+1)) holds fine layer k, and the last layer of an element is the next one's first
        std::vector<double> layers(3 * (P + 1) * plane);
        auto slot = [&](int q3, uint64_t k) { return layers.data() + (static_cast<size_t>(q3) * (P + 1) + k % (P + 1)) * plane; };
        auto fill = [&](uint64_t k) {
            if (rev) stack_layer_surf_host(p, xc, rc, thc, k, ni, nj, slot(0, k), slot(1, k), slot(2, k));
            else stack_layer_host(p, v, k, ni, nj, slot(0, k), slot(1, k), slot(2, k));
        };
        const double *fx[TM_HO3_MAX_ORDER + 1], *fy[TM_HO3_MAX_ORDER + 1], *fz[TM_HO3_MAX_ORDER + 1];
        for (uint64_t g = g0; g < g1; ++g) {
            for (uint64_t l = g == g0 ? 0 : 1; l <= P; ++l) fill(g * P + l);
            for (uint64_t l = 0; l <= P; ++l) {
                fx[l] = slot(0, g * P + l);
                fy[l] = slot(1, g * P + l);
                fz[l] = slot(2, g * P + l);
            }
            st.element_layer(g, fx, fy, fz);
        }
        tm_ho3_quality rec;
        st.finish(block, &rec);
        if (sj) ho_sj_from_pairs(jj.data(), elements, rec.orientation, sj);
        if (q) *q = rec;
        return TM_OK;
    });
}

extern "C" int tm_ho3_quality_total(const tm_ho3_quality* per_block, uint64_t n, tm_ho3_quality* total) {
    return guarded([&]() {
        if (!total || (n && !per_block)) throw TmError(TM_E_ARG, "null argument");
        ho3_quality_total(per_block, n, total);
        return TM_OK;
    });
}
