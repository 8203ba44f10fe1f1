// Host side of the high-order certificate (include/tm_hip.h, "high-order elements: certificate"): the tables from exact integers in long
// double, and tm_ho_certify_host -- the definition as a plain loop over the functions the kernel uses (tm_highorder_cert.hpp).  No HIP
// call in this file: it works in a process without a device.
#include "tm_highorder_cert.hpp"
#include "tm_api_util.hpp"
#include "tm_dispatch.hpp"

#include <cmath>
#include <cstring>
#include <vector>

namespace tmh {

void hc_check_depth(int max_depth) {
    if (max_depth < 0 || max_depth > TM_HO_CERT_MAX_DEPTH) throw TmError(TM_E_ARG, "max_depth must be 0 .. TM_HO_CERT_MAX_DEPTH");
}

static long long binom(int n, int k) {
    if (k < 0 || k > n) return 0;
    long long r = 1;
    for (int i = 1; i <= k; ++i) r = r * (n - k + i) / i;   // exact at every step
    return r;
}

HcPlan hc_plan(int p) {
    HcPlan pl;
    pl.order = p;
    const int n1 = p + 1, N = 2 * p;
    double* M = pl.tab;
    double* WU = M + n1 * n1;
    double* WV = WU + N * p;
    // The Lagrange polynomial of node m is prod_{n != m} (p t - n)/(m - n), and p t - n = -n (1 - t) + (p - n) t.  In the scaled Bernstein
    // basis (coefficient times its binomial) a product of such factors is a plain polynomial product, so the scaled coefficients h are
    // integers (|h| <= p^p); M[i][m] = h[i] / (C(p,i) prod_{n != m} (m - n)) is one long double division of two exact integers.
    for (int m = 0; m <= p; ++m) {
        long long h[TM_HO_MAX_ORDER + 1] = {1};
        long long den = 1;
        int deg = 0;
        for (int n = 0; n <= p; ++n) {
            if (n == m) continue;
            den *= (m - n);
            h[deg + 1] = 0;
            for (int k = deg + 1; k >= 0; --k) h[k] = (k <= deg ? h[k] * -n : 0) + (k > 0 ? h[k - 1] * (p - n) : 0);
            ++deg;
        }
        for (int i = 0; i <= p; ++i) M[i * n1 + m] = static_cast<double>(static_cast<long double>(h[i]) / static_cast<long double>(binom(p, i) * den));
    }
    long double lam = 0.0L;
    for (int i = 0; i <= p; ++i) {
        long double s = 0.0L;
        for (int m = 0; m <= p; ++m) s += std::fabs(static_cast<long double>(M[i * n1 + m]));
        if (s > lam) lam = s;
    }
    pl.lambda = static_cast<double>(lam);
    for (int k = 0; k < N; ++k) {
        for (int i = 0; i < p; ++i)
            WU[k * p + i] = static_cast<double>(static_cast<long double>(binom(p - 1, i) * binom(p, k - i)) / static_cast<long double>(binom(N - 1, k)));
        for (int j = 0; j <= p; ++j)
            WV[k * n1 + j] = static_cast<double>(static_cast<long double>(binom(p, j) * binom(p - 1, k - j)) / static_cast<long double>(binom(N - 1, k)));
    }
    pl.G = static_cast<double>(2.0L * p * (4 * p + 14) * (static_cast<long double>(pl.lambda) * pl.lambda) + 18 * p + 4);
    return pl;
}

namespace {

// one element on the host: the arrays the kernel keeps in LDS
template <int P>
struct HostElement {
    static constexpr int N1 = P + 1, N = 2 * P, NC = N * N;
    double d[2][N1 * N1], w[2][N1 * N1], c[2][N1 * N1];
    double xu[P * N1], yu[P * N1], xv[N1 * P], yv[N1 * P];
    double patch[HC_LEVELS][NC];
    double stat[4 * HC_LEVELS];
    double g;
    unsigned inv, und;

    template <class At>
    void coefficients(const HcPlan& pl, const At& at) {
        const double* M = pl.M();
        const QPoint base = at(0, 0);
        for (int m = 0; m < N1; ++m)
            for (int n = 0; n < N1; ++n) {
                const QPoint v = at(m, n);
                d[0][m * N1 + n] = v.x - base.x;
                d[1][m * N1 + n] = v.y - base.y;
            }
        for (int s = 0; s < 2; ++s) {
            for (int m = 0; m < N1; ++m)
                for (int j = 0; j < N1; ++j) w[s][m * N1 + j] = hc_dot(M + j * N1, d[s] + m * N1, 1, N1);
            for (int i = 0; i < N1; ++i)
                for (int j = 0; j < N1; ++j) c[s][i * N1 + j] = hc_dot(M + i * N1, w[s] + j, N1, N1);
        }
        double mxu = 0.0, myu = 0.0, mxv = 0.0, myv = 0.0;
        auto take = [](double& m, double v) {
            if (fabs(v) > m) m = fabs(v);
        };
        for (int i = 0; i < P; ++i)
            for (int j = 0; j < N1; ++j) {
                take(mxu, xu[i * N1 + j] = c[0][(i + 1) * N1 + j] - c[0][i * N1 + j]);
                take(myu, yu[i * N1 + j] = c[1][(i + 1) * N1 + j] - c[1][i * N1 + j]);
            }
        for (int i = 0; i < N1; ++i)
            for (int j = 0; j < P; ++j) {
                take(mxv, xv[i * P + j] = c[0][i * N1 + j + 1] - c[0][i * N1 + j]);
                take(myv, yv[i * P + j] = c[1][i * N1 + j + 1] - c[1][i * N1 + j]);
            }
        g = hc_guard(pl.G, mxu, myu, mxv, myv);
        for (int k = 0; k < N; ++k)
            for (int l = 0; l < N; ++l) patch[0][k * N + l] = hc_coeff(P, k, l, xu, yu, xv, yv, pl.WU(), pl.WV());
    }

    // judges patch[L]; true iff it is undecided
    bool judge(int L, double o, bool force_bad) {
        const double inf = std::numeric_limits<double>::infinity();
        double mn = inf, mx = -inf;
        bool bad = force_bad;
        for (int cidx = 0; cidx < NC; ++cidx) {
            const double v = o * patch[L][cidx];
            const int k = cidx / N, l = cidx % N;
            if (!std::isfinite(v)) bad = true;
            if ((k == 0 || k == N - 1) && (l == 0 || l == N - 1) && !(v > 0.0)) bad = true;
            if (v < mn) mn = v;
            if (v > mx) mx = v;
        }
        return hc_visit(L, mn, mx, bad, g, true, stat, inv, und);
    }

    // child q (u half q >> 1, v half q & 1) of patch[L-1] into patch[L]
    void child(int L, int q) {
        double* s = patch[L];
        std::memcpy(s, patch[L - 1], sizeof(double) * NC);
        const int qu = q >> 1, qv = q & 1;
        for (int r = 1; r < N; ++r)
            for (int l = 0; l < N; ++l) {
                if (qu == 0)
                    for (int k = N - 1; k >= r; --k) s[k * N + l] = hc_mid(s[(k - 1) * N + l], s[k * N + l]);
                else
                    for (int k = 0; k <= N - 1 - r; ++k) s[k * N + l] = hc_mid(s[k * N + l], s[(k + 1) * N + l]);
            }
        for (int r = 1; r < N; ++r)
            for (int k = 0; k < N; ++k) {
                if (qv == 0)
                    for (int l = N - 1; l >= r; --l) s[k * N + l] = hc_mid(s[k * N + l - 1], s[k * N + l]);
                else
                    for (int l = 0; l <= N - 1 - r; ++l) s[k * N + l] = hc_mid(s[k * N + l], s[k * N + l + 1]);
            }
    }

    void descend(int L, double o, int max_depth) {   // patch[L-1] is undecided
        for (int q = 0; q < 4; ++q) {
            child(L, q);
            if (judge(L, o, false) && hc_descend(L, max_depth, inv)) descend(L + 1, o, max_depth);
        }
    }

    template <class At>
    HcElement run(const HcPlan& pl, const At& at, int orientation, bool nodal_valid, int max_depth) {
        coefficients(pl, at);
        hc_stat_init(stat);
        inv = und = 0;
        const double o = orientation >= 0 ? 1.0 : -1.0;
        if (judge(0, o, !nodal_valid) && hc_descend(0, max_depth, inv)) descend(1, o, max_depth);
        return hc_decide(stat, inv, und, max_depth, g);
    }
};

template <int P>
void block_host(const HcPlan& pl, const double* xy, uint64_t ni, uint64_t nj, uint64_t block, int orientation, const double* jj, int max_depth,
                tm_ho_certificate* cert, uint8_t* status, double* bounds) {
    const QPoint* X = reinterpret_cast<const QPoint*>(xy);
    const int Ei = static_cast<int>((ni - 1) / P), Ej = static_cast<int>((nj - 1) / P);
    HcAcc acc;
    hc_init(acc);
    HostElement<P> el;
    for (int e = 0; e < Ei; ++e)
        for (int f = 0; f < Ej; ++f) {
            const QPoint* base = X + static_cast<size_t>(e) * P * nj + static_cast<size_t>(f) * P;
            auto at = [&](int m, int n) -> const QPoint& { return base[static_cast<size_t>(m) * nj + n]; };
            const size_t out = static_cast<size_t>(f) * Ei + e;
            const bool nodal_valid = hc_nodal_valid(jj[2 * out], jj[2 * out + 1], orientation);
            const HcElement r = el.run(pl, at, orientation, nodal_valid, max_depth);
            hc_count_element(r, nodal_valid, static_cast<unsigned long long>(e) * Ej + f, acc);
            if (status) status[out] = static_cast<uint8_t>(r.status);
            if (bounds) {
                bounds[2 * out] = r.lo;
                bounds[2 * out + 1] = r.hi;
            }
        }
    if (cert) hc_finish(acc, block, Ei, Ej, P, orientation, max_depth, cert);
}

template <int P>
void bezier_host(const HcPlan& pl, const double* xy, uint64_t nj, uint64_t e, uint64_t f, double* B) {
    const QPoint* base = reinterpret_cast<const QPoint*>(xy) + e * P * nj + f * P;
    auto at = [&](int m, int n) -> const QPoint& { return base[static_cast<size_t>(m) * nj + n]; };
    HostElement<P> el;
    el.coefficients(pl, at);
    std::memcpy(B, el.patch[0], sizeof(double) * 4 * P * P);
}

}  // namespace

void hc_block_host(const HcPlan& pl, const double* xy, uint64_t ni, uint64_t nj, uint64_t block, int orientation, const double* jj, int max_depth,
                   tm_ho_certificate* cert, uint8_t* status, double* bounds) {
    dispatch_int<1, 8>(pl.order, [&](auto P) { block_host<P()>(pl, xy, ni, nj, block, orientation, jj, max_depth, cert, status, bounds); });
}

void hc_certificate_total(const tm_ho_certificate* pb, uint64_t n, tm_ho_certificate* t) {
    std::memset(t, 0, sizeof(*t));
    t->min_scaled_bound = std::numeric_limits<double>::quiet_NaN();
    bool first = true;
    for (uint64_t b = 0; b < n; ++b) {
        const tm_ho_certificate& c = pb[b];
        if (c.elements == 0) continue;   // a block this rank does not own
        t->elements += c.elements;
        t->proven += c.proven;
        t->invalid += c.invalid;
        t->undecided += c.undecided;
        t->hidden_invalid += c.hidden_invalid;
        for (int L = 0; L < HC_LEVELS; ++L) t->decided_at[L] += c.decided_at[L];
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
        }
        if (c.has_unproven && !t->has_unproven) {
            t->has_unproven = 1;
            t->first_unproven_block = c.first_unproven_block;
            t->first_unproven_e = c.first_unproven_e;
            t->first_unproven_f = c.first_unproven_f;
        }
    }
}

}  // namespace tmh

using namespace tmh;

extern "C" int tm_ho_certify_tables(const tm_ho_opt* opt, double* M, double* wu, double* wv, double* G, double* norm) {
    return guarded([&]() {
        const HoPlan ho = ho_plan(opt);
        const HcPlan pl = hc_plan(ho.order);
        const int p = pl.order;
        if (M) std::memcpy(M, pl.M(), sizeof(double) * (p + 1) * (p + 1));
        if (wu) std::memcpy(wu, pl.WU(), sizeof(double) * 2 * p * p);
        if (wv) std::memcpy(wv, pl.WV(), sizeof(double) * 2 * p * (p + 1));
        if (G) *G = pl.G;
        if (norm) *norm = pl.lambda;
        return TM_OK;
    });
}

extern "C" int tm_ho_certify_host(const tm_mesh_desc* mesh, const tm_ho_opt* opt, int32_t max_depth, uint64_t block, tm_ho_certificate* cert, uint8_t* status,
                                  double* bounds) {
    return guarded([&]() {
        const HoPlan ho = ho_plan(opt);
        hc_check_depth(max_depth);
        const tm_block& b = ho_block_of(mesh, ho, block);
        const uint64_t elements = ((b.ni - 1) / ho.order) * ((b.nj - 1) / ho.order);
        std::vector<double> jj(2 * elements);
        tm_ho_quality rec;
        ho_block_host(ho, b.xy, b.ni, b.nj, block, nullptr, nullptr, &rec, jj.data());   // K13's report: the orientation and the nodal verdicts
        hc_block_host(hc_plan(ho.order), b.xy, b.ni, b.nj, block, rec.orientation, jj.data(), max_depth, cert, status, bounds);
        return TM_OK;
    });
}

extern "C" int tm_ho_jacobian_bezier_host(const tm_mesh_desc* mesh, const tm_ho_opt* opt, uint64_t block, uint64_t e, uint64_t f, double* B) {
    return guarded([&]() {
        if (!B) throw TmError(TM_E_ARG, "null argument");
        const HoPlan ho = ho_plan(opt);
        const tm_block& b = ho_block_of(mesh, ho, block);
        const uint64_t p = static_cast<uint64_t>(ho.order);
        if (e >= (b.ni - 1) / p || f >= (b.nj - 1) / p) throw TmError(TM_E_ARG, "element index past the block");
        const HcPlan pl = hc_plan(ho.order);
        dispatch_int<1, 8>(ho.order, [&](auto P) { bezier_host<P()>(pl, b.xy, b.nj, e, f, B); });
        return TM_OK;
    });
}

extern "C" int tm_ho_certificate_total(const tm_ho_certificate* per_block, uint64_t n, tm_ho_certificate* total) {
    return guarded([&]() {
        if (!total || (n && !per_block)) throw TmError(TM_E_ARG, "null argument");
        hc_certificate_total(per_block, n, total);
        return TM_OK;
    });
}
