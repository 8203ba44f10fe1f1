// Certificate of high-order hexahedra by Bezier bounds of the Jacobian (include/tm_hip.h, "high-order hexahedra: certificate"): the
// tables, the cofactor and Jacobian coefficients as two Bernstein products, the de Casteljau line, the guard and the block record, shared
// by the device kernel (tm_highorder3_cert.hip, K17) and the host definition (tm_highorder3_cert_host.cpp) so that the two evaluate the
// SAME sequence of IEEE fp64 operations (-ffp-contract=off).
//
// The decision of a patch, the per-level bookkeeping and the verdict are K14's (tm_highorder_cert.hpp: hc_visit, hc_descend, hc_decide,
// hc_count_element) with levels 0 .. TM_HO3_CERT_MAX_DEPTH; the element index of the accumulator is (g*Ej + f)*Ei + e, K16's.
//
// Array shapes of one element, all row-major, N1 = p+1:
//   control points C[i][j][k]                       N1 x N1 x N1   (i along i, j along j, k along span)
//   ·u[i][j][k] = C[i+1][j][k] - C[i][j][k]         p  x N1 x N1
//   ·v[i][j][k] = C[i][j+1][k] - C[i][j][k]         N1 x p  x N1
//   ·w[i][j][k] = C[i][j][k+1] - C[i][j][k]         N1 x N1 x p
//   cofactors c·[a][b][c]                           (2p+1) x 2p x 2p
//   B[a][b][c]                                      3p x 3p x 3p
#pragma once
#include "tm_highorder3.hpp"
#include "tm_highorder_cert.hpp"
#include "tm_stack.hpp"

namespace tmh {

static_assert(TM_HO3_CERT_MAX_DEPTH < HC_LEVELS, "the per-level bookkeeping is K14's");
constexpr int H3_LEVELS = TM_HO3_CERT_MAX_DEPTH + 1;

constexpr int h3_nn(int p) { return (p + 1) * (p + 1) * (p + 1); }   // nodes / control points
constexpr int h3_nd(int p) { return p * (p + 1) * (p + 1); }         // one derivative array
constexpr int h3_nf(int p) { return (2 * p + 1) * 2 * p * 2 * p; }   // one cofactor
constexpr int h3_nc(int p) { return 27 * p * p * p; }                // the Jacobian
// tables, packed in this order: M (p+1)^2; the product weights w^{a,b}[k][i] = C(a,i) C(b,k-i) / C(a+b,k), row k of a+1 entries:
// step 1  w^{p,p} (2p+1) x (p+1),  w^{p-1,p} 2p x p,  w^{p,p-1} 2p x (p+1);   step 2  w^{p-1,2p} 3p x p,  w^{p,2p-1} 3p x (p+1) (used along v
// and along w)
constexpr int h3_tab_m(int p) { return (p + 1) * (p + 1); }
constexpr int h3_tab_a(int p) { return (2 * p + 1) * (p + 1) + 2 * p * p + 2 * p * (p + 1); }
constexpr int h3_tab_b(int p) { return 3 * p * p + 3 * p * (p + 1); }
constexpr int h3_tab_size(int p) { return h3_tab_m(p) + h3_tab_a(p) + h3_tab_b(p); }
constexpr int H3_MAX_TAB = h3_tab_size(TM_HO3_MAX_ORDER);

struct H3Plan {
    int order = 0;
    double G = 0.0;        // the guard factor G3(p)
    double lambda = 0.0;   // ||M||_inf
    double tab[H3_MAX_TAB];
    const double* M() const { return tab; }
    const double* WA() const { return tab + h3_tab_m(order); }
    const double* WB() const { return WA() + h3_tab_a(order); }
};
H3Plan h3_plan(int order);
void h3_check_depth(int max_depth);   // TM_E_ARG outside 0 .. TM_HO3_CERT_MAX_DEPTH

// the five weight tables inside a packed table
template <int P>
struct H3Tab {
    const double *M, *Wpp, *Wqp, *Wpq, *Wq2p, *Wp2q;
    TM_Q_FN explicit H3Tab(const double* tab) {
        M = tab;
        Wpp = M + (P + 1) * (P + 1);
        Wqp = Wpp + (2 * P + 1) * (P + 1);
        Wpq = Wqp + 2 * P * P;
        Wq2p = Wpq + 2 * P * (P + 1);
        Wp2q = Wq2p + 3 * P * P;
    }
};

TM_Q_FN int h3_max(int a, int b) { return a > b ? a : b; }
TM_Q_FN int h3_min(int a, int b) { return a < b ? a : b; }

// Coefficient (a, b, c) of the cofactor  fv * gw - gv * fw  of two components f, g: fv, gv their v-derivatives (N1 x p x N1), fw, gw
// their w-derivatives (N1 x N1 x p).  Three nested sums, u outside, each over its admissible range ascending and started from 0.
template <int P>
TM_Q_FN double h3_cofactor(int a, int b, int c, const double* fv, const double* gv, const double* fw, const double* gw, const H3Tab<P>& t) {
    constexpr int N1 = P + 1;
    const int ia = h3_max(0, a - P), ib = h3_min(P, a);
    const int ja = h3_max(0, b - P), jb = h3_min(P - 1, b);
    const int ka = h3_max(0, c - (P - 1)), kb = h3_min(P, c);
    double su = 0.0;
    for (int i = ia; i <= ib; ++i) {
        double sv = 0.0;
        for (int j = ja; j <= jb; ++j) {
            double sw = 0.0;
            for (int k = ka; k <= kb; ++k) {
                const int x = (i * P + j) * N1 + k, y = ((a - i) * N1 + (b - j)) * P + (c - k);
                const double term = fv[x] * gw[y] - gv[x] * fw[y];
                sw = sw + t.Wpq[c * N1 + k] * term;
            }
            sv = sv + t.Wqp[b * P + j] * sw;
        }
        su = su + t.Wpp[a * N1 + i] * sv;
    }
    return su;
}

// Coefficient (a, b, c) of B = xu*cx + yu*cy + zu*cz: du[q] the u-derivatives (p x N1 x N1), cf[q] the cofactors ((2p+1) x 2p x 2p)
template <int P>
TM_Q_FN double h3_coeff(int a, int b, int c, const double* xu, const double* yu, const double* zu, const double* cx, const double* cy, const double* cz,
                        const H3Tab<P>& t) {
    constexpr int N1 = P + 1, F = 2 * P;
    const int ia = h3_max(0, a - 2 * P), ib = h3_min(P - 1, a);
    const int ja = h3_max(0, b - (2 * P - 1)), jb = h3_min(P, b);
    const int ka = h3_max(0, c - (2 * P - 1)), kb = h3_min(P, c);
    double su = 0.0;
    for (int i = ia; i <= ib; ++i) {
        double sv = 0.0;
        for (int j = ja; j <= jb; ++j) {
            double sw = 0.0;
            for (int k = ka; k <= kb; ++k) {
                const int x = (i * N1 + j) * N1 + k, y = ((a - i) * F + (b - j)) * F + (c - k);
                const double term = xu[x] * cx[y] + yu[x] * cy[y] + zu[x] * cz[y];
                sw = sw + t.Wp2q[c * N1 + k] * term;
            }
            sv = sv + t.Wp2q[b * N1 + j] * sw;
        }
        su = su + t.Wq2p[a * P + i] * sv;
    }
    return su;
}

// One line of N coefficients (stride `st`) halved by de Casteljau in place; upper: keep the half [1/2, 1], else [0, 1/2]
template <int N>
TM_Q_FN void h3_split_line(double* s, int st, bool upper) {
    double v[N];
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = s[k * st];
    if (upper) {
#pragma unroll
        for (int r = 1; r < N; ++r)
#pragma unroll
            for (int k = 0; k <= N - 1 - r; ++k) v[k] = hc_mid(v[k], v[k + 1]);
    } else {
#pragma unroll
        for (int r = 1; r < N; ++r)
#pragma unroll
            for (int k = N - 1; k >= r; --k) v[k] = hc_mid(v[k - 1], v[k]);
    }
#pragma unroll
    for (int k = 0; k < N; ++k) s[k * st] = v[k];
}
// line `line` (0 .. N*N-1) of direction dir (0: u, 1: v, 2: w) of a patch of N^3 coefficients
template <int N>
TM_Q_FN void h3_split(double* patch, int dir, int line, bool upper) {
    const int p0 = line / N, p1 = line - p0 * N;
    if (dir == 0) h3_split_line<N>(patch + p0 * N + p1, N * N, upper);
    else if (dir == 1) h3_split_line<N>(patch + p0 * N * N + p1, N, upper);
    else h3_split_line<N>(patch + (p0 * N + p1) * N, 1, upper);
}

// g = (G3 * 2^-53) * R3, R3 = ((sx * sy) * sz), s· = (max|·u| + max|·v|) + max|·w| over the element's derivative coefficients; m[q][d]
TM_Q_FN double h3_guard(double G, const double m[3][3]) {
    const double sx = (m[0][0] + m[0][1]) + m[0][2], sy = (m[1][0] + m[1][1]) + m[1][2], sz = (m[2][0] + m[2][1]) + m[2][2];
    return (G * 0x1p-53) * ((sx * sy) * sz);
}

// whether coefficient index c of an N^3 patch is one of its eight corners
template <int N>
TM_Q_FN bool h3_is_corner(int c) {
    const int a = c / (N * N), r = c - a * N * N, b = r / N, k = r - b * N;
    return (a == 0 || a == N - 1) && (b == 0 || b == N - 1) && (k == 0 || k == N - 1);
}

TM_Q_FN void h3_finish(const HcAcc& a, uint64_t block, uint64_t Ei, uint64_t Ej, uint64_t Eg, int order, int orientation, int max_depth, tm_ho3_certificate* out) {
    const bool any = a.at != Q_NO_CELL, unproven = a.first != Q_NO_CELL;
    out->elements = Ei * Ej * Eg;
    out->proven = a.proven;
    out->invalid = a.invalid;
    out->undecided = a.undecided;
    out->hidden_invalid = a.hidden;
    out->orientation = orientation;
    out->order = order;
    out->max_depth = max_depth;
    out->has_unproven = unproven ? 1 : 0;
    for (int L = 0; L < H3_LEVELS; ++L) out->decided_at[L] = a.decided[L];
    out->min_scaled_bound = any ? a.sb : std::numeric_limits<double>::quiet_NaN();
    out->worst_block = any ? block : 0;
    out->worst_e = any ? a.at % Ei : 0;
    out->worst_f = any ? (a.at / Ei) % Ej : 0;
    out->worst_g = any ? a.at / (Ei * Ej) : 0;
    out->first_unproven_block = unproven ? block : 0;
    out->first_unproven_e = unproven ? a.first % Ei : 0;
    out->first_unproven_f = unproven ? (a.first / Ei) % Ej : 0;
    out->first_unproven_g = unproven ? a.first / (Ei * Ej) : 0;
}

// ---- host side (tm_highorder3_cert_host.cpp)
// x, y, z: planes of nk*nj*ni doubles in PLOT3D order, already checked against the order; jj: K16's (Jmin, Jmax) pairs,
// jj[2*((g*Ej + f)*Ei + e)]; status and bounds in the same element order, may be NULL
void h3_block_host(const H3Plan& plan, const double* x, const double* y, const double* z, uint64_t ni, uint64_t nj, uint64_t nk, uint64_t block, int orientation,
                   const double* jj, int max_depth, tm_ho3_certificate* cert, uint8_t* status, double* bounds);
// K16's report of a block given as planes: the record and the pairs
void h3_report_host(const HoPlan& plan, const double* x, const double* y, const double* z, uint64_t ni, uint64_t nj, uint64_t nk, uint64_t block, tm_ho3_quality* rec,
                    double* jj);
// the fine planes of the whole stacked block on the host (tm_stack_block[_surf]_host for every layer); checks cuts and sizes
void h3_stack_planes_host(const tm_mesh_desc* const* cuts, const tm_stack_opt* sopt, const tm_stack_surfaces* surfaces, const HoPlan& plan, uint64_t block,
                          uint64_t* ni, uint64_t* nj, uint64_t* nk, std::vector<double>& xyz, uint64_t* outside);

}  // namespace tmh
