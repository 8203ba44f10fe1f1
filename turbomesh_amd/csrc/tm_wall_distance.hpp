// K20  wall distance of the welded mesh (include/tm_hip.h, "wall distance of the welded mesh"): the definition -- image of a query point,
// the primitive tables, point to segment, point to triangle, the key that is minimised -- shared by the kernels (tm_wall_distance.hip)
// and the host twin (tm_wall_distance_host.cpp).  Compiled with contraction off on both sides (csrc/Makefile); the only fused operations
// are the explicit fma() of the compensated cross product, which rounds once on both sides.  Every expression order below is part of the
// definition: host and device give the same bits.
#pragma once
#include "tm_weld.hpp"

#include <cmath>

namespace tmh {

constexpr int WD_GROUP = 64;             // consecutive primitives that share one bounding box
constexpr int WD_CHUNK = 64;             // group records per LDS chunk of the kernel
constexpr int WD_MAX_IMAGES = 16;
// |computed d2 - exact d2| <= WD_G * 2^-53 * rho2 for every pair, rho2 = the largest squared distance from the query to the nodes of the
// face + its longest squared edge (26 for a segment and the edge regions of a triangle, 23 for its interior, 2 for the square of the rounded root).  The culling guard adds 8 for
// the rounding of the box bound and of rho2 itself.
constexpr double WD_G = 32.0;
constexpr double WD_EPS = 1.1102230246251565e-16;   // 2^-53
constexpr double WD_GUARD = (WD_G + 8.0) * WD_EPS;

struct WdSeg {   // 64 bytes: edge A -> B of a plane mesh
    double A[2], B[2], a[2], L, iL;
};
struct WdTri {   // 208 bytes: triangle A, B, C of a stacked mesh; a collinear one is stored as (A', B', B') of its longest edge, n = 0
    double A[3], B[3], C[3], ab[3], ac[3], bc[3], n[3];
    double nn, iLab, iLac, iLbc, Lbc;   // n: the unit normal (0 when collinear); nn: the squared length it had before
};
struct WdGroup {   // 80 bytes: box of WD_GROUP consecutive primitives, one of their vertices, their longest squared edge
    double lo[3], hi[3], seed[3], E2;
};
struct WdKey {
    double d2;
    int32_t face, image;
};

// P' of a query point under an image: formed once per point and image, in this order
TM_WELD_HD void wd_image_point(int dim, const tm_wall_image& m, const double* P, double* Q) {
    Q[0] = P[0] - m.t[0];
    if (dim == 2) {
        Q[1] = P[1] - m.t[1];
        Q[2] = 0.0;
    } else {
        Q[1] = (m.c * P[1] + m.s * P[2]) - m.t[1];
        Q[2] = (-m.s * P[1] + m.c * P[2]) - m.t[2];
    }
}

TM_WELD_HD WdSeg wd_build_seg(const double* A, const double* B) {
    WdSeg s;
    for (int c = 0; c < 2; ++c) {
        s.A[c] = A[c];
        s.B[c] = B[c];
        s.a[c] = B[c] - A[c];
    }
    s.L = s.a[0] * s.a[0] + s.a[1] * s.a[1];
    s.iL = 1.0 / s.L;
    return s;
}

TM_WELD_HD double wd_seg_d2(const WdSeg& s, const double* Q) {
    const double px = Q[0] - s.A[0], py = Q[1] - s.A[1];
    const double t = px * s.a[0] + py * s.a[1];
    if (t <= 0.0) return px * px + py * py;
    if (t >= s.L) {
        const double bx = Q[0] - s.B[0], by = Q[1] - s.B[1];
        return bx * bx + by * by;
    }
    const double r = t * s.iL;
    const double qx = px - r * s.a[0], qy = py - r * s.a[1];
    return qx * qx + qy * qy;
}

TM_WELD_HD double wd_dot3(const double* u, const double* v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }
// a*b - c*d with both products error-free: the result carries the rounding of one subtraction and one addition
TM_WELD_HD double wd_diff_of_products(double a, double b, double c, double d) {
    const double p = a * b, q = c * d;
    const double ep = fma(a, b, -p), eq = fma(c, d, -q);
    return (p - q) + (ep - eq);
}

TM_WELD_HD void wd_tri_edges(WdTri& t) {
    for (int c = 0; c < 3; ++c) {
        t.ab[c] = t.B[c] - t.A[c];
        t.ac[c] = t.C[c] - t.A[c];
        t.bc[c] = t.C[c] - t.B[c];
    }
}
// longest squared edge of the triangle as given (before a collinear one is replaced)
TM_WELD_HD WdTri wd_build_tri(const double* A, const double* B, const double* C, double* longest) {
    WdTri t;
    for (int c = 0; c < 3; ++c) {
        t.A[c] = A[c];
        t.B[c] = B[c];
        t.C[c] = C[c];
    }
    wd_tri_edges(t);
    double Lab = wd_dot3(t.ab, t.ab), Lac = wd_dot3(t.ac, t.ac), Lbc = wd_dot3(t.bc, t.bc);
    double E = Lab;
    if (Lac > E) E = Lac;
    if (Lbc > E) E = Lbc;
    *longest = E;
    t.n[0] = wd_diff_of_products(t.ab[1], t.ac[2], t.ab[2], t.ac[1]);
    t.n[1] = wd_diff_of_products(t.ab[2], t.ac[0], t.ab[0], t.ac[2]);
    t.n[2] = wd_diff_of_products(t.ab[0], t.ac[1], t.ab[1], t.ac[0]);
    const double nn = wd_dot3(t.n, t.n);
    if (!(nn > 0.0)) {   // collinear (or NaN): the longest edge twice, so that the vertex and edge regions of A'B' take every query
        const double* P0 = A;
        const double* P1 = B;
        if (!(Lab >= Lac && Lab >= Lbc)) {
            P1 = C;
            if (!(Lac >= Lbc)) P0 = B;
        }
        for (int c = 0; c < 3; ++c) {
            const double p0 = P0[c], p1 = P1[c];
            t.A[c] = p0;
            t.B[c] = p1;
            t.C[c] = p1;
        }
        wd_tri_edges(t);
        Lab = wd_dot3(t.ab, t.ab);
        Lac = Lab;
        Lbc = 0.0;
        t.n[0] = t.n[1] = t.n[2] = 0.0;
        t.nn = 0.0;
    } else {   // the unit normal: an axis-parallel one comes out as +-1 exactly, so the distance above a flat hub is the coordinate itself
        const double len = sqrt(nn);
        for (int c = 0; c < 3; ++c) t.n[c] = t.n[c] / len;
        t.nn = nn;
    }
    t.iLab = 1.0 / Lab;
    t.iLac = 1.0 / Lac;
    t.iLbc = 1.0 / Lbc;
    t.Lbc = Lbc;
    return t;
}
// true when the interior formula's bound needs care: the largest sine of the three angles is below 2^-20 (DESIGN: such a sliver keeps its
// group from being culled, the results stay the contract's)
TM_WELD_HD bool wd_tri_sliver(const WdTri& t) {
    const double nn = t.nn;
    if (!(nn > 0.0)) return false;
    const double Lab = wd_dot3(t.ab, t.ab), Lac = wd_dot3(t.ac, t.ac), Lbc = t.Lbc;
    double m = Lab * Lac;   // the product of the two shortest squared edges
    if (Lab * Lbc < m) m = Lab * Lbc;
    if (Lac * Lbc < m) m = Lac * Lbc;
    return nn < 9.094947017729282e-13 * m;   // 2^-40
}

// closest point by Voronoi region: vertex A, vertex B, edge AB, vertex C, edge AC, edge BC, interior
TM_WELD_HD double wd_tri_d2(const WdTri& t, const double* Q) {
    const double ap[3] = {Q[0] - t.A[0], Q[1] - t.A[1], Q[2] - t.A[2]};
    const double d1 = wd_dot3(t.ab, ap), d2 = wd_dot3(t.ac, ap);
    if (d1 <= 0.0 && d2 <= 0.0) return wd_dot3(ap, ap);
    const double bp[3] = {Q[0] - t.B[0], Q[1] - t.B[1], Q[2] - t.B[2]};
    const double d3 = wd_dot3(t.ab, bp), d4 = wd_dot3(t.ac, bp);
    if (d3 >= 0.0 && d4 <= d3) return wd_dot3(bp, bp);
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        const double r = d1 * t.iLab;
        const double q[3] = {ap[0] - r * t.ab[0], ap[1] - r * t.ab[1], ap[2] - r * t.ab[2]};
        return wd_dot3(q, q);
    }
    const double cp[3] = {Q[0] - t.C[0], Q[1] - t.C[1], Q[2] - t.C[2]};
    const double d5 = wd_dot3(t.ab, cp), d6 = wd_dot3(t.ac, cp);
    if (d6 >= 0.0 && d5 <= d6) return wd_dot3(cp, cp);
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        const double r = d2 * t.iLac;
        const double q[3] = {ap[0] - r * t.ac[0], ap[1] - r * t.ac[1], ap[2] - r * t.ac[2]};
        return wd_dot3(q, q);
    }
    const double va = d3 * d6 - d5 * d4;
    const double tb = wd_dot3(t.bc, bp);
    if (va <= 0.0 && tb >= 0.0 && tb <= t.Lbc) {
        const double r = tb * t.iLbc;
        const double q[3] = {bp[0] - r * t.bc[0], bp[1] - r * t.bc[1], bp[2] - r * t.bc[2]};
        return wd_dot3(q, q);
    }
    const double h = wd_dot3(ap, t.n);
    return h * h;
}

// (d2, face, image) lexicographically; a NaN d2 never wins
TM_WELD_HD void wd_take(WdKey& k, double d2, int32_t face, int32_t image) {
    if (d2 < k.d2 || (d2 == k.d2 && (face < k.face || (face == k.face && image < k.image)))) {
        k.d2 = d2;
        k.face = face;
        k.image = image;
    }
}

// argument checks of tm_wall_distance (TM_E_ARG), before anything is read or launched; returns the primitives
int64_t wall_check(int dim, uint64_t nfaces, const int32_t* faces, uint64_t npoints, const double* const* points, uint64_t nimages, const tm_wall_image* images,
                   const double* distance);
void wall_distance_host(int dim, uint64_t nfaces, const int32_t* faces, uint64_t npoints, const double* const* points, uint64_t nimages, const tm_wall_image* images,
                        double* distance, int32_t* face, int32_t* image, tm_wall_info* info);
// the record's fields that are counts of the call
void wall_info_sizes(int dim, uint64_t nfaces, uint64_t npoints, uint64_t nimages, tm_wall_info* info);
// tm_wall_select on a boundary plan
struct WeldBoundaryPlan;
void wall_select(const WeldBoundaryPlan& bp, uint32_t kinds_mask, std::vector<int32_t>& face_index, std::vector<tm_wall_image>& images);

}  // namespace tmh
