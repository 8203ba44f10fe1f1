// K22  elliptic smoothing of a stored 3-D block (include/tm_hip.h, "elliptic smoothing of stacked blocks"): the node update of one Jacobi
// sweep of the 3-D Winslow equations, the line formula and the transfinite blend of the Thomas-Middlecoff control field, and the record
// of a sweep -- shared by the kernels (tm_smooth3d.hip) and the host twin (tm_smooth3d_host.cpp).  Compiled with contraction off on both
// sides (csrc/Makefile); the one division per node and the divisions of the line formula are the correctly rounded ones on both sides.
// Every expression order below is part of the definition: host and device give the same bits.
#pragma once
#include "../../include/tm_hip.h"

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TM_S3_HD __host__ __device__ inline
#else
#define TM_S3_HD inline
#endif

namespace tmh {

constexpr uint64_t S3_NO_NODE = ~uint64_t{0};

struct S3Vec {
    double x, y, z;
};

// the 19 points a node reads: p[dk+1][dj+1][di+1]; the eight cube corners are never filled nor read
struct S3Stencil {
    S3Vec p[3][3][3];
};

struct S3Node {
    S3Vec out;      // the node behind the sweep (the input where it is frozen)
    double d2;      // |out - P|^2, 0 where frozen
    double J;       // K12's expression on the central differences
    bool frozen;
};

TM_S3_HD S3Vec s3_sub(const S3Vec& a, const S3Vec& b) { return S3Vec{a.x - b.x, a.y - b.y, a.z - b.z}; }
TM_S3_HD S3Vec s3_add(const S3Vec& a, const S3Vec& b) { return S3Vec{a.x + b.x, a.y + b.y, a.z + b.z}; }
TM_S3_HD S3Vec s3_scale(double c, const S3Vec& a) { return S3Vec{c * a.x, c * a.y, c * a.z}; }
TM_S3_HD double s3_dot(const S3Vec& a, const S3Vec& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
// 0.25*(((pp - pm) - mp) + mm)
TM_S3_HD S3Vec s3_mixed(const S3Vec& pp, const S3Vec& pm, const S3Vec& mp, const S3Vec& mm) {
    return S3Vec{0.25 * (((pp.x - pm.x) - mp.x) + mm.x), 0.25 * (((pp.y - pm.y) - mp.y) + mm.y), 0.25 * (((pp.z - pm.z) - mp.z) + mm.z)};
}
TM_S3_HD bool s3_finite(double v) { return v - v == 0.0; }

// One interior node.  CONTROL false: the three products with f are not formed at all (f1..f3 are not read), so a Laplace sweep does not
// depend on the field code.
template <bool CONTROL>
TM_S3_HD S3Node s3_node(const S3Stencil& s, double f1, double f2, double f3, double omega) {
    const S3Vec &P = s.p[1][1][1];
    const S3Vec &ip = s.p[1][1][2], &im = s.p[1][1][0], &jp = s.p[1][2][1], &jm = s.p[1][0][1], &kp = s.p[2][1][1], &km = s.p[0][1][1];
    const S3Vec r1 = s3_scale(0.5, s3_sub(ip, im)), r2 = s3_scale(0.5, s3_sub(jp, jm)), r3 = s3_scale(0.5, s3_sub(kp, km));
    const S3Vec s1 = s3_add(ip, im), s2 = s3_add(jp, jm), s3 = s3_add(kp, km);
    const double g11 = s3_dot(r1, r1), g22 = s3_dot(r2, r2), g33 = s3_dot(r3, r3);
    const double g12 = s3_dot(r1, r2), g13 = s3_dot(r1, r3), g23 = s3_dot(r2, r3);
    const double a11 = g22 * g33 - g23 * g23;
    const double a22 = g11 * g33 - g13 * g13;
    const double a33 = g11 * g22 - g12 * g12;
    const double a12 = g13 * g23 - g12 * g33;
    const double a13 = g12 * g23 - g13 * g22;
    const double a23 = g12 * g13 - g23 * g11;
    const S3Vec m12 = s3_mixed(s.p[1][2][2], s.p[1][0][2], s.p[1][2][0], s.p[1][0][0]);
    const S3Vec m13 = s3_mixed(s.p[2][1][2], s.p[0][1][2], s.p[2][1][0], s.p[0][1][0]);
    const S3Vec m23 = s3_mixed(s.p[2][2][1], s.p[0][2][1], s.p[2][0][1], s.p[0][0][1]);
    S3Vec num;
    num.x = ((a11 * s1.x + a22 * s2.x) + a33 * s3.x) + 2.0 * ((a12 * m12.x + a13 * m13.x) + a23 * m23.x);
    num.y = ((a11 * s1.y + a22 * s2.y) + a33 * s3.y) + 2.0 * ((a12 * m12.y + a13 * m13.y) + a23 * m23.y);
    num.z = ((a11 * s1.z + a22 * s2.z) + a33 * s3.z) + 2.0 * ((a12 * m12.z + a13 * m13.z) + a23 * m23.z);
    if (CONTROL) {
        const double c1 = a11 * f1, c2 = a22 * f2, c3 = a33 * f3;
        num.x = num.x + ((c1 * r1.x + c2 * r2.x) + c3 * r3.x);
        num.y = num.y + ((c1 * r1.y + c2 * r2.y) + c3 * r3.y);
        num.z = num.z + ((c1 * r1.z + c2 * r2.z) + c3 * r3.z);
    }
    const double den = 2.0 * ((a11 + a22) + a33);
    S3Node n;
    n.J = (r1.x * (r2.y * r3.z - r2.z * r3.y) + r1.y * (r2.z * r3.x - r2.x * r3.z)) + r1.z * (r2.x * r3.y - r2.y * r3.x);
    n.frozen = !(s3_finite(den) && den > 0.0 && s3_finite(num.x) && s3_finite(num.y) && s3_finite(num.z));
    if (n.frozen) {
        n.out = P;
        n.d2 = 0.0;
        return n;
    }
    const double inv = 1.0 / den;
    n.out.x = P.x + omega * (num.x * inv - P.x);
    n.out.y = P.y + omega * (num.y * inv - P.y);
    n.out.z = P.z + omega * (num.z * inv - P.z);
    const S3Vec d = s3_sub(n.out, P);
    n.d2 = (d.x * d.x + d.y * d.y) + d.z * d.z;
    return n;
}

// What a thread, a workgroup (device) or the block (host) has seen of one sweep.  Counts, the sum in the order of the calls, and the
// largest update by its square with the smallest flat index at a tie; a NaN never wins.
struct S3Acc {
    unsigned long long neg, pos, zero_or_nan, frozen;
    unsigned long long max_node;
    double sum_sq, max_sq;
};

TM_S3_HD void s3_init(S3Acc& a) {
    a.neg = a.pos = a.zero_or_nan = a.frozen = 0;
    a.max_node = S3_NO_NODE;
    a.sum_sq = 0.0;
    a.max_sq = -1.0;   // below every square: the first node that is not a NaN wins
}
TM_S3_HD void s3_take(S3Acc& a, double d2, unsigned long long node) {
    if (d2 > a.max_sq || (d2 == a.max_sq && node < a.max_node)) {
        a.max_sq = d2;
        a.max_node = node;
    }
}
TM_S3_HD void s3_count(S3Acc& a, const S3Node& n, unsigned long long node) {
    if (n.J < 0.0)
        a.neg += 1;
    else if (n.J > 0.0)
        a.pos += 1;
    else
        a.zero_or_nan += 1;
    a.frozen += n.frozen ? 1 : 0;
    a.sum_sq = a.sum_sq + n.d2;
    s3_take(a, n.d2, node);
}
TM_S3_HD void s3_combine(S3Acc& a, const S3Acc& b) {
    a.neg += b.neg;
    a.pos += b.pos;
    a.zero_or_nan += b.zero_or_nan;
    a.frozen += b.frozen;
    a.sum_sq = a.sum_sq + b.sum_sq;
    if (b.max_node != S3_NO_NODE) s3_take(a, b.max_sq, b.max_node);
}

// ------------------------------------------------------------------ control field
// Axis d of a line and the two axes across it, p < q: d = 0: (j, k), d = 1: (i, k), d = 2: (i, j).
TM_S3_HD int s3_axis_p(int d) { return d == 0 ? 1 : 0; }
TM_S3_HD int s3_axis_q(int d) { return d == 2 ? 1 : 2; }
// flat index of the node at position t along axis d, a along p, b along q
TM_S3_HD size_t s3_flat(int d, size_t t, size_t a, size_t b, size_t ni, size_t nj) {
    const size_t i = d == 0 ? t : a, j = d == 0 ? a : (d == 1 ? t : b), k = d == 2 ? t : b;
    return (k * nj + j) * ni + i;
}
// The face values of direction d: four tables of lines, [p = 0][b][t], [p = np-1][b][t], [q = 0][a][t], [q = nq-1][a][t], one behind the
// other; n[3] = {ni, nj, nk}.
TM_S3_HD size_t s3_face_count(int d, const size_t* n) { return 2 * n[d] * (n[s3_axis_p(d)] + n[s3_axis_q(d)]); }
TM_S3_HD size_t s3_face_p(int d, const size_t* n, int hi, size_t b, size_t t) { return (static_cast<size_t>(hi) * n[s3_axis_q(d)] + b) * n[d] + t; }
TM_S3_HD size_t s3_face_q(int d, const size_t* n, int hi, size_t a, size_t t) {
    return 2 * n[s3_axis_q(d)] * n[d] + (static_cast<size_t>(hi) * n[s3_axis_p(d)] + a) * n[d] + t;
}

// phi of the middle one of three consecutive points of a grid line
TM_S3_HD double s3_line_phi(const S3Vec& rm, const S3Vec& r0, const S3Vec& rp) {
    const S3Vec d1 = s3_scale(0.5, s3_sub(rp, rm));
    const S3Vec d2 = s3_sub(s3_sub(rp, r0), s3_sub(r0, rm));
    const double dd = s3_dot(d1, d1);
    if (dd == 0.0 || !s3_finite(dd)) return 0.0;
    return -s3_dot(d1, d2) / dd;
}

// entry e of the face tables of direction d (e < s3_face_count): 0 at the ends of a line
TM_S3_HD double s3_face_value(int d, size_t e, const size_t* n, const double* X, const double* Y, const double* Z) {
    const size_t nd = n[d], np = n[s3_axis_p(d)], nq = n[s3_axis_q(d)];
    const size_t t = e % nd;
    size_t line = e / nd, a, b;
    if (line < 2 * nq) {
        a = line < nq ? 0 : np - 1;
        b = line < nq ? line : line - nq;
    } else {
        line -= 2 * nq;
        a = line < np ? line : line - np;
        b = line < np ? 0 : nq - 1;
    }
    if (t == 0 || t + 1 >= nd) return 0.0;
    const size_t om = s3_flat(d, t - 1, a, b, n[0], n[1]), o0 = s3_flat(d, t, a, b, n[0], n[1]), op = s3_flat(d, t + 1, a, b, n[0], n[1]);
    return s3_line_phi(S3Vec{X[om], Y[om], Z[om]}, S3Vec{X[o0], Y[o0], Z[o0]}, S3Vec{X[op], Y[op], Z[op]});
}

// the boolean-sum transfinite interpolation of the face values of direction d at the interior node (t, a, b)
TM_S3_HD double s3_blend(int d, const size_t* n, const double* F, size_t t, size_t a, size_t b) {
    const size_t np = n[s3_axis_p(d)], nq = n[s3_axis_q(d)];
    const double u = static_cast<double>(a) / static_cast<double>(np - 1), v = static_cast<double>(b) / static_cast<double>(nq - 1);
    const double Fp0 = F[s3_face_p(d, n, 0, b, t)], Fp1 = F[s3_face_p(d, n, 1, b, t)];
    const double Fq0 = F[s3_face_q(d, n, 0, a, t)], Fq1 = F[s3_face_q(d, n, 1, a, t)];
    const double E00 = F[s3_face_p(d, n, 0, 0, t)], E10 = F[s3_face_p(d, n, 1, 0, t)];
    const double E01 = F[s3_face_p(d, n, 0, nq - 1, t)], E11 = F[s3_face_p(d, n, 1, nq - 1, t)];
    const double um = 1.0 - u, vm = 1.0 - v;
    return ((((um * Fp0 + u * Fp1) + vm * Fq0) + v * Fq1)) - ((((um * vm) * E00 + (u * vm) * E10) + (um * v) * E01) + (u * v) * E11);
}

// ------------------------------------------------------------------ the call
struct S3Plan {
    size_t n[3];   // ni, nj, nk
    size_t nodes, interior;
    int algorithm;
    uint64_t sweeps;
    double omega, tol;
};
// TM_E_SIZE / TM_E_ARG as include/tm_hip.h says; `with_planes`: the call carries coordinates (x, y, z must not be null)
S3Plan s3_plan(uint64_t ni, uint64_t nj, uint64_t nk, const double* x, const double* y, const double* z, const tm_smooth3d_opt* opt);
// the sweep count behind which the stopping test is made
inline bool s3_check_after(const S3Plan& p, uint64_t done) { return p.tol > 0.0 && (done % 8 == 0 || done == p.sweeps); }
inline bool s3_converged(const S3Plan& p, double sum_sq) { return std::sqrt(sum_sq / static_cast<double>(p.interior)) <= p.tol; }
// the record from the reduced first and last sweep (null: no sweep was made)
void s3_fill_info(const S3Plan& p, uint64_t done, const S3Acc* first, const S3Acc* last, const double* control_max, tm_smooth3d_info* info);
// the host definition of the field: f[0..2], nodes doubles each; 0 on every node that is not interior
void s3_control_host(const S3Plan& p, const double* X, const double* Y, const double* Z, double* const* f);

}  // namespace tmh
