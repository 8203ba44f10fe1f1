// Host side of the spanwise stacking (include/tm_hip.h, "3-D from 2-D cuts"): validation, the weight matrix in long double, and
// tm_stack_block_host -- the definition as a plain loop, summed over c = 0 .. K-1 like the kernel.  No HIP call in this file: it works
// in a process without a device.
#include "tm_stack.hpp"
#include "tm_api_util.hpp"

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

StackPlan stack_plan(const tm_stack_opt* opt) {
    if (!opt || !opt->span || !opt->layers) throw TmError(TM_E_ARG, "null stack options, span or layers");
    if (opt->ncuts < 2 || opt->ncuts > TM_STACK_MAX_CUTS) throw TmError(TM_E_ARG, "a stack takes 2 .. TM_STACK_MAX_CUTS cuts");
    if (opt->nlayers < 1) throw TmError(TM_E_ARG, "a stack needs at least one layer");
    if (opt->interpolation != TM_STACK_LINEAR && opt->interpolation != TM_STACK_CUBIC) throw TmError(TM_E_ARG, "unknown stack interpolation");
    if (opt->mapping != TM_STACK_PLANAR && opt->mapping != TM_STACK_CYLINDRICAL) throw TmError(TM_E_ARG, "unknown stack mapping");
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

}  // namespace tmh

using namespace tmh;

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
