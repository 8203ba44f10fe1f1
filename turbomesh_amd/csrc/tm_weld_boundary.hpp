// K19  boundary of the welded mesh (include/tm_hip.h, "boundary of the welded mesh"): what the kernels (tm_weld_boundary.hip) and the host
// definition (tm_weld_boundary_host.cpp) share -- segment and local node to block node, the local orders of the faces, the terms of a fine
// sub-face.  The terms are compiled with contraction off on both sides (csrc/Makefile), so each is bit-identical between host and device.
#pragma once
#include "tm_weld.hpp"

#include <cmath>

namespace tmh {

constexpr int WB_SIDE_HUB = 4, WB_SIDE_SHROUD = 5;
constexpr int WB_MAX_NPF = 81;     // (8+1)^2 local nodes of a face at most (the measure takes quadrilaterals of any order a curve may have)
constexpr int WB_TERMS = 5;        // measure, normal x / y / z, moment

// One boundary segment of the plane mesh in face order (patch-major): where its faces go in the face list.  With layers the face of span
// element g is face0 + g * stride, stride = the segments of its patch.
struct WbSeg {
    int32_t block, side, e, patch;
    int32_t face0, stride;
};

// position along its side of the local node a (0 .. p) of segment e: counter-clockwise in index space, reversed for a block of orientation -1
TM_WELD_HD int wb_side_pos(uint32_t side, int p, int e, int a, int orientation) {
    const bool ascending = (side == TM_SIDE_I_MIN || side == TM_SIDE_J_MAX) == (orientation >= 0);
    return ascending ? e * p + a : (e + 1) * p - a;
}
// flat index inside its block of local node a of a segment
TM_WELD_HD int wb_seg_node(const WeldBlock& B, uint32_t side, int p, int e, int a, int orientation) {
    int i, j;
    weld_side_node(B.ni, B.nj, side, wb_side_pos(side, p, e, a, orientation), i, j);
    return j * B.ni + i;
}
// flat index inside its block of local node (a, b') of the cap face of element (e, f): hub a along j, shroud a along i; orientation -1 exchanges them
TM_WELD_HD int wb_cap_node(const WeldBlock& B, bool shroud, int p, int e, int f, int a, int bp, int orientation) {
    const bool a_along_i = shroud == (orientation >= 0);
    const int di = a_along_i ? a : bp, dj = a_along_i ? bp : a;
    return (f * p + dj) * B.ni + e * p + di;
}
// place in a VTK Lagrange curve of the node at parameter a
TM_WELD_HD int wb_curve_local(int p, int a) { return a == 0 ? 0 : a == p ? 1 : a + 1; }

// fine edge A -> B of a plane face: t = {length, n_x, n_y, 0, moment}
TM_WELD_HD void wb_edge_terms(double xa, double ya, double xb, double yb, double* t) {
    const double dx = xb - xa, dy = yb - ya;
    t[0] = sqrt(dx * dx + dy * dy);
    t[1] = dy;
    t[2] = -dx;
    t[3] = 0.0;
    t[4] = xa * yb - xb * ya;
}
// fine quadrilateral A, B, C, D in ring order: t = {|n|, n_x, n_y, n_z, centroid . n}, n = 0.5 * (C - A) x (D - B)
TM_WELD_HD void wb_quad_terms(const double* A, const double* B, const double* C, const double* D, double* t) {
    const double ux = C[0] - A[0], uy = C[1] - A[1], uz = C[2] - A[2];
    const double vx = D[0] - B[0], vy = D[1] - B[1], vz = D[2] - B[2];
    const double nx = 0.5 * (uy * vz - uz * vy), ny = 0.5 * (uz * vx - ux * vz), nz = 0.5 * (ux * vy - uy * vx);
    const double cx = 0.25 * (((A[0] + B[0]) + C[0]) + D[0]), cy = 0.25 * (((A[1] + B[1]) + C[1]) + D[1]), cz = 0.25 * (((A[2] + B[2]) + C[2]) + D[2]);
    t[0] = sqrt((nx * nx + ny * ny) + nz * nz);
    t[1] = nx;
    t[2] = ny;
    t[3] = nz;
    t[4] = (cx * nx + cy * ny) + cz * nz;
}

// The boundary of a description at one order and layer count: patches with their CSR, the boundary segments in face order, the counts.
struct WeldBoundaryPlan {
    int p = 1, npf = 2;
    int64_t Eg = 1;                 // span elements (1 for a plane mesh)
    bool layered = false;
    std::vector<tm_weld_patch> patches;
    std::vector<WbSeg> segs;        // plane boundary segments, patch-major
    std::vector<int64_t> cells_of;  // plane elements per block (prefix)
    int64_t lateral_faces = 0, cap_faces = 0, faces = 0;   // cap_faces: one cap
    int64_t hub_begin = 0, shroud_begin = 0;
    uint64_t loops = 0, irregular = 0;
};
// tm_ho_check / tm_ho3_check, the classification of every segment, the patch table (TM_E_MISMATCH for a condition off the element grid)
WeldBoundaryPlan weld_boundary_plan(const tm_mesh_desc* mesh, const WeldPlan& pl, int order, uint64_t nk);
// face_patch and origin of every face, either may be null: integers of the plan
void weld_boundary_labels(const WeldPlan& pl, const WeldBoundaryPlan& bp, int32_t* face_patch, int32_t* origin);
// place of local node (a, b) in VTK's Lagrange quadrilateral of order p: inv[b * (p+1) + a]
std::vector<int32_t> weld_quad_inverse(int p);
// argument checks of tm_weld_faces_measure (TM_E_ARG), before anything is read or launched; returns the nodes per face
int weld_measure_check(int dim, int order, uint64_t nfaces, const int32_t* faces, const int32_t* face_patch, uint64_t npatches, uint64_t npoints, int ncomp,
                       const double* const* points, const tm_weld_patch* patches);
void weld_boundary_faces_host(const WeldPlan& pl, const WeldBoundaryPlan& bp, const int32_t* map, int64_t nodes_out, uint64_t nk, const int32_t* orientation,
                              int32_t* faces);
void weld_faces_measure_host(int dim, int p, uint64_t nfaces, const int32_t* faces, const int32_t* face_patch, uint64_t npatches, const double* const* points,
                             tm_weld_patch* patches);

}  // namespace tmh
