// Host side of the spanwise stacking (include/tm_hip.h, "3-D from 2-D cuts"): validation, the weight matrix in long double, and
// tm_stack_block_host -- the definition as a plain loop, summed over c = 0 .. K-1 like the kernel.  No HIP call in this file: it works
// in a process without a device.
#include "tm_stack.hpp"
#include "tm_api_util.hpp"
#include "tm_stack_surface.hpp"

#include <cmath>
#include <vector>

namespace tmh {

// One weight row in long double.  G = T^-1 D maps the cut values to the interior second derivatives of the natural spline (rows
// 1 .. K-2; M_0 = M_{K-1} = 0): g[m * K + c] = dM_m / dv_c.
static void weight_row(const std::vector<long double>& z, const std::vector<long double>& g, int K, bool cubic, double s_fp64, long double* row) {
    for (int c = 0; c < K; ++c) row[c] = 0.0L;
    for (int c = 0; c < K; ++c)
        if (s_fp64 == static_cast<double>(z[c])) {   // a layer at a cut: the unit vector, nothing computed
            row[c] = 1.0L;
            return;
        }
    const long double s = s_fp64;
    int c = 0;
    while (c < K - 2 && z[c + 1] <= s) ++c;   // the largest index <= K-2 with z[c] <= s
    const long double h = z[c + 1] - z[c];
    if (!cubic) {
        const long double t = (s - z[c]) / h;
        row[c] = 1.0L - t;
        row[c + 1] = t;
        return;
    }
    const long double a = (z[c + 1] - s) / h, b = (s - z[c]) / h;
    const long double fa = (a * a * a - a) * h * h / 6.0L, fb = (b * b * b - b) * h * h / 6.0L;
    for (int q = 0; q < K; ++q) row[q] = fa * g[static_cast<size_t>(c) * K + q] + fb * g[static_cast<size_t>(c + 1) * K + q];
    row[c] += a;
    row[c + 1] += b;
}

// rows 1 .. K-2 of: h_{m-1}/6 M_{m-1} + (h_{m-1} + h_m)/3 M_m + h_m/6 M_{m+1} = (v_{m+1} - v_m)/h_m - (v_m - v_{m-1})/h_{m-1}, solved for
// every unit vector v = e_c by the Thomas algorithm (the matrix is strictly diagonally dominant: no pivoting needed)
static std::vector<long double> spline_second_derivatives(const std::vector<long double>& z, int K) {
    std::vector<long double> g(static_cast<size_t>(K) * K, 0.0L);
    const int n = K - 2;
    if (n < 1) return g;
    std::vector<long double> lo(n), di(n), up(n), cp(n), rhs(n);
    for (int m = 1; m <= n; ++m) {
        const long double h0 = z[m] - z[m - 1], h1 = z[m + 1] - z[m];
        lo[m - 1] = h0 / 6.0L;
        di[m - 1] = (h0 + h1) / 3.0L;
        up[m - 1] = h1 / 6.0L;
    }
    for (int c = 0; c < K; ++c) {
        for (int m = 1; m <= n; ++m) {
            const long double h0 = z[m] - z[m - 1], h1 = z[m + 1] - z[m];
            long double r = 0.0L;
            if (c == m + 1) r += 1.0L / h1;
            if (c == m) r -= 1.0L / h1 + 1.0L / h0;
            if (c == m - 1) r += 1.0L / h0;
            rhs[m - 1] = r;
        }
        cp[0] = up[0] / di[0];
        rhs[0] = rhs[0] / di[0];
        for (int m = 1; m < n; ++m) {
            const long double den = di[m] - lo[m] * cp[m - 1];
            cp[m] = up[m] / den;
            rhs[m] = (rhs[m] - lo[m] * rhs[m - 1]) / den;
        }
        for (int m = n - 2; m >= 0; --m) rhs[m] -= cp[m] * rhs[m + 1];
        for (int m = 1; m <= n; ++m) g[static_cast<size_t>(m) * K + c] = rhs[m - 1];
    }
    return g;
}

static StackPlan stack_plan_of(const tm_stack_opt* opt, bool revolution) {
    if (!opt || !opt->span || !opt->layers) throw TmError(TM_E_ARG, "null stack options, span or layers");
    if (opt->ncuts < 2 || opt->ncuts > TM_STACK_MAX_CUTS) throw TmError(TM_E_ARG, "a stack takes 2 .. TM_STACK_MAX_CUTS cuts");
    if (opt->nlayers < 1) throw TmError(TM_E_ARG, "a stack needs at least one layer");
    if (opt->interpolation != TM_STACK_LINEAR && opt->interpolation != TM_STACK_CUBIC) throw TmError(TM_E_ARG, "unknown stack interpolation");
    if (revolution) {
        if (opt->mapping != TM_STACK_REVOLUTION) throw TmError(TM_E_ARG, "the calls that take meridional tables serve TM_STACK_REVOLUTION only");
    } else {
        if (opt->mapping == TM_STACK_REVOLUTION) throw TmError(TM_E_ARG, "TM_STACK_REVOLUTION needs meridional tables: use the *_surf calls");
        if (opt->mapping != TM_STACK_PLANAR && opt->mapping != TM_STACK_CYLINDRICAL) throw TmError(TM_E_ARG, "unknown stack mapping");
    }
    StackPlan p;
    p.ncuts = static_cast<int>(opt->ncuts);
    p.mapping = opt->mapping;
    p.nlayers = opt->nlayers;
    p.span.assign(opt->span, opt->span + opt->ncuts);
    p.layers.assign(opt->layers, opt->layers + opt->nlayers);
    const int K = p.ncuts;
    for (int c = 0; c < K; ++c) {
        if (!std::isfinite(p.span[c])) throw TmError(TM_E_ARG, "span coordinates must be finite");
        if (c > 0 && !(p.span[c] > p.span[c - 1])) throw TmError(TM_E_ARG, "span coordinates must be strictly increasing");
        if (p.mapping == TM_STACK_CYLINDRICAL && !(p.span[c] > 0.0)) throw TmError(TM_E_ARG, "the cylindrical mapping needs radii > 0");
    }
    for (double s : p.layers)
        if (!std::isfinite(s) || s < p.span[0] || s > p.span[K - 1]) throw TmError(TM_E_ARG, "a layer lies outside the span of the cuts (no extrapolation)");
    const std::vector<long double> z(p.span.begin(), p.span.end());
    const bool cubic = opt->interpolation == TM_STACK_CUBIC && K > 2;   // at K = 2 the natural spline IS the linear interpolant
    const std::vector<long double> g = cubic ? spline_second_derivatives(z, K) : std::vector<long double>();
    p.weights.resize(static_cast<size_t>(p.nlayers) * K);
    long double row[TM_STACK_MAX_CUTS];
    for (uint64_t k = 0; k < p.nlayers; ++k) {
        weight_row(z, g, K, cubic, p.layers[k], row);
        for (int c = 0; c < K; ++c) p.weights[static_cast<size_t>(k) * K + c] = static_cast<double>(row[c]);   // the one rounding
    }
    return p;
}

StackPlan stack_plan(const tm_stack_opt* opt) { return stack_plan_of(opt, false); }

// The second derivatives M of the natural spline through (z_m, v_m), M_0 = M_{N-1} = 0: the system of spline_second_derivatives with the
// data's own right-hand side (exact zeros where the data are constant, so a constant column stays a constant curve), the same Thomas sweep.
static std::vector<long double> spline_second_derivatives_of(const std::vector<long double>& z, const double* v, int N) {
    std::vector<long double> M(N, 0.0L);
    const int n = N - 2;
    if (n < 1) return M;
    std::vector<long double> cp(n), rhs(n);
    for (int m = 1; m <= n; ++m) {
        const long double h0 = z[m] - z[m - 1], h1 = z[m + 1] - z[m];
        const long double lo = h0 / 6.0L, di = (h0 + h1) / 3.0L, up = h1 / 6.0L;
        const long double r = (static_cast<long double>(v[m + 1]) - v[m]) / h1 - (static_cast<long double>(v[m]) - v[m - 1]) / h0;
        if (m == 1) {
            cp[0] = up / di;
            rhs[0] = r / di;
        } else {
            const long double den = di - lo * cp[m - 2];
            cp[m - 1] = up / den;
            rhs[m - 1] = (r - lo * rhs[m - 2]) / den;
        }
    }
    for (int m = n - 2; m >= 0; --m) rhs[m] -= cp[m] * rhs[m + 1];
    for (int m = 1; m <= n; ++m) M[m] = rhs[m - 1];
    return M;
}

StackPlan stack_plan_surf(const tm_stack_opt* opt, const tm_stack_surfaces* sf, SurfPlan& surf) {
    StackPlan p = stack_plan_of(opt, true);
    if (!sf || !sf->nknots || !sf->u || !sf->x || !sf->r) throw TmError(TM_E_ARG, "null surfaces or tables");
    if (sf->ncuts != opt->ncuts) throw TmError(TM_E_ARG, "the surfaces and the stack disagree in the number of cuts");
    if (sf->interpolation != TM_SURF_LINEAR && sf->interpolation != TM_SURF_CUBIC) throw TmError(TM_E_ARG, "unknown interpolation of the meridional curves");
    const int K = p.ncuts;
    surf = SurfPlan();
    for (int c = 0; c < K; ++c) {
        const double rr = sf->rref ? sf->rref[c] : p.span[c];
        if (!std::isfinite(rr) || !(rr > 0.0)) throw TmError(TM_E_ARG, sf->rref ? "reference radii must be finite and > 0" : "without reference radii every span coordinate must be > 0");
        surf.rref.push_back(rr);
        const uint64_t N = sf->nknots[c];
        if (N < 2 || N > TM_STACK_MAX_KNOTS) throw TmError(TM_E_ARG, "a meridional table takes 2 .. TM_STACK_MAX_KNOTS knots");
        const double *u = sf->u[c], *x = sf->x[c], *r = sf->r[c];
        if (!u || !x || !r) throw TmError(TM_E_ARG, "null meridional table");
        for (uint64_t n = 0; n < N; ++n) {
            if (!std::isfinite(u[n]) || !std::isfinite(x[n]) || !std::isfinite(r[n])) throw TmError(TM_E_ARG, "meridional tables must be finite");
            if (n > 0 && !(u[n] > u[n - 1])) throw TmError(TM_E_ARG, "the knots of a meridional table must be strictly increasing");
            if (!(r[n] > 0.0)) throw TmError(TM_E_ARG, "the radii of a meridional table must be > 0");
        }
        surf.nknots.push_back(static_cast<int>(N));
        surf.first.push_back(static_cast<int>(surf.knots.size()));
        surf.knots.insert(surf.knots.end(), u, u + N);
        // the coefficients in long double, each rounded once
        const int Ni = static_cast<int>(N);
        const std::vector<long double> z(u, u + N);
        const bool cubic = sf->interpolation == TM_SURF_CUBIC && Ni > 2;
        const double* val[2] = {x, r};
        std::vector<long double> M[2] = {std::vector<long double>(N, 0.0L), std::vector<long double>(N, 0.0L)};
        if (cubic)
            for (int q = 0; q < 2; ++q) M[q] = spline_second_derivatives_of(z, val[q], Ni);
        for (int n = 0; n + 1 < Ni; ++n) {
            const long double h = z[n + 1] - z[n];
            for (int q = 0; q < 2; ++q) {
                const long double v0 = val[q][n], v1 = val[q][n + 1];
                surf.coef.push_back(val[q][n]);
                surf.coef.push_back(static_cast<double>((v1 - v0) / h - h * (2.0L * M[q][n] + M[q][n + 1]) / 6.0L));
                surf.coef.push_back(static_cast<double>(M[q][n] / 2.0L));
                surf.coef.push_back(static_cast<double>((M[q][n + 1] - M[q][n]) / (6.0L * h)));
            }
        }
    }
    return p;
}

void stack_check_window(const StackPlan& plan, uint64_t k_begin, uint64_t k_count) {
    if (k_count < 1 || k_begin >= plan.nlayers || k_count > plan.nlayers - k_begin) throw TmError(TM_E_ARG, "the layer window is empty or reaches past nlayers");
}

void stack_check_cuts(const tm_mesh_desc* const* cuts, int ncuts, uint64_t block, uint64_t* ni, uint64_t* nj) {
    if (!cuts) throw TmError(TM_E_ARG, "null list of cuts");
    for (int c = 0; c < ncuts; ++c)
        if (!cuts[c] || !cuts[c]->blocks || cuts[c]->nblocks == 0) throw TmError(TM_E_ARG, "a cut without a mesh description or without blocks");
    for (int c = 1; c < ncuts; ++c)
        if (cuts[c]->nblocks != cuts[0]->nblocks) throw TmError(TM_E_SIZE, "InconsistentSize: the cuts differ in block count");
    if (block >= cuts[0]->nblocks) throw TmError(TM_E_ARG, "block index past the mesh");
    const tm_block& b0 = cuts[0]->blocks[block];
    for (int c = 0; c < ncuts; ++c) {
        const tm_block& b = cuts[c]->blocks[block];
        if (b.ni != b0.ni || b.nj != b0.nj) throw TmError(TM_E_SIZE, "InconsistentSize: the cuts differ in the size of the block");
        if (!b.xy) throw TmError(TM_E_ARG, "block without coordinates");
    }
    if (b0.ni < 1 || b0.nj < 1 || b0.ni * b0.nj >= (uint64_t{1} << 31)) throw TmError(TM_E_SIZE, "block size out of range");
    *ni = b0.ni;
    *nj = b0.nj;
}

void stack_layer_host(const StackPlan& p, const double* const* v, uint64_t k, uint64_t ni, uint64_t nj, double* x, double* y, double* z) {
    const int K = p.ncuts;
    const bool cyl = p.mapping == TM_STACK_CYLINDRICAL;
    const double* w = &p.weights[static_cast<size_t>(k) * K];
    const double s = p.layers[k];
    for (uint64_t j = 0; j < nj; ++j)
        for (uint64_t i = 0; i < ni; ++i) {
            const size_t n = static_cast<size_t>(i) * nj + j, o = static_cast<size_t>(j) * ni + i;
            double ax = w[0] * v[0][2 * n], ay = w[0] * (cyl ? v[0][2 * n + 1] / p.span[0] : v[0][2 * n + 1]);
            for (int c = 1; c < K; ++c) {
                ax = ax + w[c] * v[c][2 * n];
                ay = ay + w[c] * (cyl ? v[c][2 * n + 1] / p.span[c] : v[c][2 * n + 1]);
            }
            x[o] = ax;
            y[o] = cyl ? s * std::sin(ay) : ay;
            z[o] = cyl ? s * std::cos(ay) : s;
        }
}

void stack_surf_nodes_host(const StackPlan& p, const SurfPlan& sf, const double* const* v, uint64_t ni, uint64_t nj, std::vector<double>& x, std::vector<double>& r,
                           std::vector<double>& th, uint64_t* outside) {
    const size_t plane = static_cast<size_t>(ni) * nj;
    x.resize(plane * p.ncuts);
    r.resize(plane * p.ncuts);
    th.resize(plane * p.ncuts);
    for (int c = 0; c < p.ncuts; ++c) {
        const int N = sf.nknots[c];
        const double* u = &sf.knots[sf.first[c]];
        const double* coef = &sf.coef[static_cast<size_t>(sf.first[c] - c) * SURF_COEF];
        uint64_t out = 0;
        for (size_t n = 0; n < plane; ++n) {
            const double un = v[c][2 * n];
            const int m = surf_locate(u, N, un);
            surf_eval(coef + static_cast<size_t>(m) * SURF_COEF, un - u[m], &x[c * plane + n], &r[c * plane + n]);
            th[c * plane + n] = v[c][2 * n + 1] / sf.rref[c];
            out += surf_outside(u[0], u[N - 1], un) ? 1 : 0;
        }
        if (outside) outside[c] = out;
    }
}

void stack_layer_surf_host(const StackPlan& p, const std::vector<double>& xc, const std::vector<double>& rc, const std::vector<double>& thc, uint64_t k, uint64_t ni,
                           uint64_t nj, double* x, double* y, double* z) {
    const int K = p.ncuts;
    const double* w = &p.weights[static_cast<size_t>(k) * K];
    const size_t plane = static_cast<size_t>(ni) * nj;
    for (uint64_t j = 0; j < nj; ++j)
        for (uint64_t i = 0; i < ni; ++i) {
            const size_t n = static_cast<size_t>(i) * nj + j, o = static_cast<size_t>(j) * ni + i;
            double ax = w[0] * xc[n], ar = w[0] * rc[n], at = w[0] * thc[n];
            for (int c = 1; c < K; ++c) {
                ax = ax + w[c] * xc[c * plane + n];
                ar = ar + w[c] * rc[c * plane + n];
                at = at + w[c] * thc[c * plane + n];
            }
            x[o] = ax;
            y[o] = ar * std::sin(at);
            z[o] = ar * std::cos(at);
        }
}

}  // namespace tmh

using namespace tmh;

extern "C" int tm_stack_surface_tables(const tm_stack_opt* opt, const tm_stack_surfaces* surfaces, double* coeff) {
    return guarded([&]() {
        if (!coeff) throw TmError(TM_E_ARG, "null argument");
        SurfPlan sf;
        stack_plan_surf(opt, surfaces, sf);
        for (size_t k = 0; k < sf.coef.size(); ++k) coeff[k] = sf.coef[k];
        return TM_OK;
    });
}

extern "C" int tm_stack_block_surf_host(const tm_mesh_desc* const* cuts, const tm_stack_opt* opt, const tm_stack_surfaces* surfaces, uint64_t block,
                                        uint64_t k_begin, uint64_t k_count, double* x, double* y, double* z, uint64_t* outside) {
    return guarded([&]() {
        if (!x || !y || !z) throw TmError(TM_E_ARG, "null argument");
        SurfPlan sf;
        const StackPlan p = stack_plan_surf(opt, surfaces, sf);
        stack_check_window(p, k_begin, k_count);
        uint64_t ni = 0, nj = 0;
        stack_check_cuts(cuts, p.ncuts, block, &ni, &nj);
        const double* v[TM_STACK_MAX_CUTS];
        for (int c = 0; c < p.ncuts; ++c) v[c] = cuts[c]->blocks[block].xy;
        std::vector<double> xc, rc, thc;
        stack_surf_nodes_host(p, sf, v, ni, nj, xc, rc, thc, outside);
        const size_t plane = static_cast<size_t>(ni) * nj;
        for (uint64_t k = 0; k < k_count; ++k) stack_layer_surf_host(p, xc, rc, thc, k_begin + k, ni, nj, x + k * plane, y + k * plane, z + k * plane);
        return TM_OK;
    });
}

extern "C" int tm_stack_weights(const tm_stack_opt* opt, double* weights) {
    return guarded([&]() {
        if (!weights) throw TmError(TM_E_ARG, "null argument");
        const StackPlan p = stack_plan(opt);
        for (size_t k = 0; k < p.weights.size(); ++k) weights[k] = p.weights[k];
        return TM_OK;
    });
}

extern "C" int tm_stack_block_host(const tm_mesh_desc* const* cuts, const tm_stack_opt* opt, uint64_t block, uint64_t k_begin, uint64_t k_count,
                                   double* x, double* y, double* z) {
    return guarded([&]() {
        if (!x || !y || !z) throw TmError(TM_E_ARG, "null argument");
        const StackPlan p = stack_plan(opt);
        stack_check_window(p, k_begin, k_count);
        uint64_t ni = 0, nj = 0;
        stack_check_cuts(cuts, p.ncuts, block, &ni, &nj);
        const double* v[TM_STACK_MAX_CUTS];
        for (int c = 0; c < p.ncuts; ++c) v[c] = cuts[c]->blocks[block].xy;
        const size_t plane = static_cast<size_t>(ni) * nj;
        for (uint64_t k = 0; k < k_count; ++k) stack_layer_host(p, v, k_begin + k, ni, nj, x + k * plane, y + k * plane, z + k * plane);
        return TM_OK;
    });
}
