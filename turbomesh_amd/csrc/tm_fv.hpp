// K21  faces, owners and finite-volume metrics of the welded mesh (include/tm_hip.h, "faces of the welded mesh"): what the kernels
// (tm_fv.hip) and the host definition (tm_fv_host.cpp) share -- the face a cell shows on a side, its neighbour across that side, the
// sorting network of the owned neighbours, and every expression of the metrics in its fixed order.  The translation units are compiled
// with contraction off (csrc/Makefile), so each value is bit-identical between host and device.
#pragma once
#include "tm_weld_boundary.hpp"

#include <cmath>

namespace tmh {

constexpr int FV_BOUNDARY = -1;               // "no neighbour" in the segment table and among a cell's neighbours
constexpr double FV_COS_70 = 0.3420201433256687;   // cos 70 degrees, the threshold of tm_fv_info.nonorthogonal_faces

// One segment of a block side: the plane cell behind its partner segment and the local side that cell shows, or FV_BOUNDARY.
struct FvSeg {
    int32_t block, side, seg;
};
// A block as the face kernels see it: WeldBlock, the first cell of the block (cells of tm_weld_cells at order 1, all layers), its first
// segment per side in the segment table, its orientation.
struct FvBlock {
    int32_t off, ni, nj, cell0, seg0[4], orientation;
};

// flat indices inside its block of the two nodes A -> B of side 0 .. 3 of cell (e, f): K19's rule for a block that is this one cell
TM_WELD_HD void fv_side_nodes(int ni, int e, int f, int side, int orientation, int& nA, int& nB) {
    const bool ascending = (side == TM_SIDE_I_MIN || side == TM_SIDE_J_MAX) == (orientation >= 0);
    if (side == TM_SIDE_I_MIN || side == TM_SIDE_I_MAX) {
        const int j = f + (side == TM_SIDE_I_MAX ? 1 : 0);
        nA = j * ni + (ascending ? e : e + 1);
        nB = j * ni + (ascending ? e + 1 : e);
    } else {
        const int i = e + (side == TM_SIDE_J_MAX ? 1 : 0);
        nA = (ascending ? f : f + 1) * ni + i;
        nB = (ascending ? f + 1 : f) * ni + i;
    }
}
// the ids of the face cell (e, f, g) of block B shows on local side 0 .. 5: 2 ids of a plane mesh, 4 of a stacked one
TM_WELD_HD void fv_cell_face(const FvBlock& B, int e, int f, int g, int side, bool layered, const int32_t* map, int nodes_out, int32_t* ids) {
    if (side < 4) {
        int nA, nB;
        fv_side_nodes(B.ni, e, f, side, B.orientation, nA, nB);
        const int a = map[B.off + nA], b = map[B.off + nB];
        if (!layered) {
            ids[0] = a;
            ids[1] = b;
        } else {
            ids[0] = g * nodes_out + a;
            ids[1] = g * nodes_out + b;
            ids[2] = (g + 1) * nodes_out + b;
            ids[3] = (g + 1) * nodes_out + a;
        }
        return;
    }
    const bool shroud = side == WB_SIDE_SHROUD, a_along_i = shroud == (B.orientation >= 0);
    const int layer = (shroud ? g + 1 : g) * nodes_out;
    const int ra[4] = {0, 1, 1, 0}, rb[4] = {0, 0, 1, 1};
    for (int q = 0; q < 4; ++q) {
        const int di = a_along_i ? ra[q] : rb[q], dj = a_along_i ? rb[q] : ra[q];
        ids[q] = layer + map[B.off + (f + dj) * B.ni + e + di];
    }
}
// plane cell (e, f) behind segment `seg` of side 0 .. 3 of a block of Ei x Ej cells
TM_WELD_HD void fv_seg_cell(int Ei, int Ej, int side, int seg, int& e, int& f) {
    switch (side) {
    case TM_SIDE_I_MIN: e = seg; f = 0; break;
    case TM_SIDE_I_MAX: e = seg; f = Ej - 1; break;
    case TM_SIDE_J_MIN: e = 0; f = seg; break;
    default: e = Ei - 1; f = seg; break;
    }
}
// Neighbour of cell (e, f, g) of block b across local side 0 .. 5 and the local side the neighbour shows back; FV_BOUNDARY when the side
// is a boundary face.  Eg = layers - 1 (1 for a plane mesh, which has no sides 4 and 5).
TM_WELD_HD int fv_neighbour(const FvBlock* blocks, const FvSeg* segs, int b, int e, int f, int g, int Eg, int side, int& back) {
    const FvBlock& B = blocks[b];
    const int Ei = B.ni - 1, Ej = B.nj - 1;
    const int self = B.cell0 + (g * Ej + f) * Ei + e;
    if (side == WB_SIDE_HUB) {
        back = WB_SIDE_SHROUD;
        return g > 0 ? self - Ei * Ej : FV_BOUNDARY;
    }
    if (side == WB_SIDE_SHROUD) {
        back = WB_SIDE_HUB;
        return g < Eg - 1 ? self + Ei * Ej : FV_BOUNDARY;
    }
    back = side ^ 1;
    if (side == TM_SIDE_I_MIN && f > 0) return self - Ei;
    if (side == TM_SIDE_I_MAX && f < Ej - 1) return self + Ei;
    if (side == TM_SIDE_J_MIN && e > 0) return self - 1;
    if (side == TM_SIDE_J_MAX && e < Ei - 1) return self + 1;
    const FvSeg s = segs[B.seg0[side] + (side == TM_SIDE_I_MIN || side == TM_SIDE_I_MAX ? e : f)];
    if (s.block < 0) return FV_BOUNDARY;
    const FvBlock& P = blocks[s.block];
    int pe, pf;
    fv_seg_cell(P.ni - 1, P.nj - 1, s.side, s.seg, pe, pf);
    back = s.side;
    return P.cell0 + (g * (P.nj - 1) + pf) * (P.ni - 1) + pe;
}
// cell -> (block, e, f, g): the last block whose first cell is <= cell
TM_WELD_HD void fv_cell_place(const FvBlock* blocks, int nblocks, int cell, int& b, int& e, int& f, int& g) {
    int lo = 0, hi = nblocks - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (blocks[mid].cell0 <= cell) lo = mid;
        else hi = mid - 1;
    }
    b = lo;
    const int Ei = blocks[b].ni - 1, Ej = blocks[b].nj - 1, l = cell - blocks[b].cell0, fg = l / Ei;
    e = l - fg * Ei;
    g = fg / Ej;
    f = fg - g * Ej;
}
// The neighbours above `cell` in upper-triangular order: key = neighbour, then the owner's side.  Fills nb[k], sd[k], bk[k] for the
// k-th owned face and returns their number.  A fixed network of compare-exchanges over 6 slots (empty slots carry the largest key).
TM_WELD_HD int fv_owned(const FvBlock* blocks, const FvSeg* segs, int b, int e, int f, int g, int Eg, int nsides, int cell, int* nb, int* sd, int* bk) {
    long long packed[6];   // neighbour << 6 | side << 3 | the side shown back: below 2^37
    int n = 0;
    for (int s = 0; s < 6; ++s) {
        packed[s] = 0x7fffffffffffffffll;
        if (s >= nsides) continue;
        int back = 0;
        const int v = fv_neighbour(blocks, segs, b, e, f, g, Eg, s, back);
        if (v > cell) {
            packed[s] = (static_cast<long long>(v) << 6) | (s << 3) | back;
            ++n;
        }
    }
    // the 12 compare-exchanges in 5 layers that sort 6 keys
    const int net[12][2] = {{0, 5}, {1, 3}, {2, 4}, {1, 2}, {3, 4}, {0, 3}, {2, 5}, {0, 1}, {2, 3}, {4, 5}, {1, 2}, {3, 4}};
    for (int k = 0; k < 12; ++k) {
        const int i = net[k][0], j = net[k][1];
        if (packed[j] < packed[i]) {
            const long long t = packed[i];
            packed[i] = packed[j];
            packed[j] = t;
        }
    }
    for (int k = 0; k < n; ++k) {
        bk[k] = static_cast<int>(packed[k] & 7);
        sd[k] = static_cast<int>((packed[k] >> 3) & 7);
        nb[k] = static_cast<int>(packed[k] >> 6);
    }
    return n;
}

// ------------------------------------------------------------------ metrics: every expression in its fixed order, nothing fused
// area vector S and centre Cf of a face from its nodes P[k][0 .. 2] (dim 2: A, B with z = 0; dim 3: the ring A, B, C, D)
TM_WELD_HD void fv_face_geometry(int dim, const double P[4][3], double* S, double* Cf) {
    if (dim == 2) {
        S[0] = P[1][1] - P[0][1];
        S[1] = -(P[1][0] - P[0][0]);
        S[2] = 0.0;
        Cf[0] = 0.5 * (P[0][0] + P[1][0]);
        Cf[1] = 0.5 * (P[0][1] + P[1][1]);
        Cf[2] = 0.0;
        return;
    }
    const double ux = P[2][0] - P[0][0], uy = P[2][1] - P[0][1], uz = P[2][2] - P[0][2];
    const double vx = P[3][0] - P[1][0], vy = P[3][1] - P[1][1], vz = P[3][2] - P[1][2];
    S[0] = 0.5 * (uy * vz - uz * vy);
    S[1] = 0.5 * (uz * vx - ux * vz);
    S[2] = 0.5 * (ux * vy - uy * vx);
    double m[3], r[4][3];
    for (int c = 0; c < 3; ++c) m[c] = 0.25 * (((P[0][c] + P[1][c]) + P[2][c]) + P[3][c]);
    for (int k = 0; k < 4; ++k)
        for (int c = 0; c < 3; ++c) r[k][c] = P[k][c] - m[c];
    double W = 0.0, acc[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < 4; ++k) {
        const double* a = r[k];
        const double* b = r[(k + 1) & 3];
        const double nx = 0.5 * (a[1] * b[2] - a[2] * b[1]), ny = 0.5 * (a[2] * b[0] - a[0] * b[2]), nz = 0.5 * (a[0] * b[1] - a[1] * b[0]);
        const double w = sqrt((nx * nx + ny * ny) + nz * nz);
        W += w;
        for (int c = 0; c < 3; ++c) acc[c] += w * ((a[c] + b[c]) / 3.0);   // the triangle's centroid relative to m
    }
    for (int c = 0; c < 3; ++c) Cf[c] = W > 0.0 ? m[c] + acc[c] / W : m[c];
}

struct FvCell {
    double volume, centre[3], closedness;
};
// nf = 4 or 6 faces in local side order: S[k], Cf[k] as fv_face_geometry gave them for the stored ring, sign[k] = +1 where the cell is the
// face's owner and -1 otherwise
TM_WELD_HD FvCell fv_cell_metrics(int dim, int nf, const double S[6][3], const double Cf[6][3], const double* sign) {
    FvCell out;
    double mean[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < nf; ++k)
        for (int c = 0; c < 3; ++c) mean[c] += Cf[k][c];
    for (int c = 0; c < 3; ++c) mean[c] = mean[c] / static_cast<double>(nf);
    double V = 0.0, mom[3] = {0.0, 0.0, 0.0}, net[3] = {0.0, 0.0, 0.0}, mag[3] = {0.0, 0.0, 0.0};
    const double base = dim == 2 ? 2.0 / 3.0 : 0.75;   // a pyramid's centroid lies this far from the apex towards the centre of its base
    for (int k = 0; k < nf; ++k) {
        double r[3];
        for (int c = 0; c < 3; ++c) r[c] = Cf[k][c] - mean[c];
        const double v = sign[k] * (((S[k][0] * r[0] + S[k][1] * r[1]) + S[k][2] * r[2]) / static_cast<double>(dim));
        V += v;
        for (int c = 0; c < 3; ++c) {
            mom[c] += v * (base * r[c]);
            net[c] += sign[k] * S[k][c];
            mag[c] += fabs(S[k][c]);
        }
    }
    out.volume = V;
    for (int c = 0; c < 3; ++c) out.centre[c] = V != 0.0 ? mean[c] + mom[c] / V : mean[c];
    double top = 0.0, bottom = 0.0;
    for (int c = 0; c < 3; ++c) {
        if (fabs(net[c]) > top) top = fabs(net[c]);
        if (mag[c] > bottom) bottom = mag[c];
    }
    out.closedness = bottom > 0.0 ? top / bottom : 0.0;
    return out;
}
// cos of the angle between d and S; d = C_nb - C_own (interior) or Cf - C_own (boundary)
TM_WELD_HD double fv_cos(const double* d, const double* S) {
    const double dS = (d[0] * S[0] + d[1] * S[1]) + d[2] * S[2];
    const double dd = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]), SS = sqrt((S[0] * S[0] + S[1] * S[1]) + S[2] * S[2]);
    return dS / (dd * SS);
}
// |Cf - C_own - ((S.(Cf - C_own)) / (S.d)) d| / |d| with d = C_nb - C_own
TM_WELD_HD double fv_skewness(const double* Cown, const double* Cnb, const double* Cf, const double* S) {
    double d[3], e[3], m[3];
    for (int c = 0; c < 3; ++c) {
        d[c] = Cnb[c] - Cown[c];
        e[c] = Cf[c] - Cown[c];
    }
    const double Se = (S[0] * e[0] + S[1] * e[1]) + S[2] * e[2], Sd = (S[0] * d[0] + S[1] * d[1]) + S[2] * d[2];
    const double r = Se / Sd;
    for (int c = 0; c < 3; ++c) m[c] = e[c] - r * d[c];
    return sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]) / sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
}

// The record as it is accumulated: counts, sums and extremes with the smallest index at a tie -- independent of the order of
// evaluation except for the rounding of total_volume.  An index of -1 says "none yet"; NaN values never win an extreme.
struct FvAcc {
    long long negative, first_negative, nonorth, inverted;
    long long min_v_cell, max_v_cell, closed_cell, cos_face, skew_face;
    double min_v, max_v, total_v, closed, min_cos, skew;
};
TM_WELD_HD void fv_acc_init(FvAcc& a) {
    a.negative = a.nonorth = a.inverted = 0;
    a.first_negative = a.min_v_cell = a.max_v_cell = a.closed_cell = a.cos_face = a.skew_face = -1;
    a.min_v = a.max_v = a.closed = a.min_cos = a.skew = 0.0;
    a.total_v = 0.0;
}
TM_WELD_HD void fv_take_min(double& best, long long& at, double v, long long i) {
    if (i < 0 || v != v) return;
    if (at < 0 || v < best || (v == best && i < at)) {
        best = v;
        at = i;
    }
}
TM_WELD_HD void fv_take_max(double& best, long long& at, double v, long long i) {
    if (i < 0 || v != v) return;
    if (at < 0 || v > best || (v == best && i < at)) {
        best = v;
        at = i;
    }
}
TM_WELD_HD void fv_acc_combine(FvAcc& a, const FvAcc& b) {
    a.negative += b.negative;
    a.nonorth += b.nonorth;
    a.inverted += b.inverted;
    if (b.first_negative >= 0 && (a.first_negative < 0 || b.first_negative < a.first_negative)) a.first_negative = b.first_negative;
    fv_take_min(a.min_v, a.min_v_cell, b.min_v, b.min_v_cell);
    fv_take_max(a.max_v, a.max_v_cell, b.max_v, b.max_v_cell);
    fv_take_max(a.closed, a.closed_cell, b.closed, b.closed_cell);
    fv_take_min(a.min_cos, a.cos_face, b.min_cos, b.cos_face);
    fv_take_max(a.skew, a.skew_face, b.skew, b.skew_face);
    a.total_v += b.total_v;
}
TM_WELD_HD void fv_acc_cell(FvAcc& a, long long cell, const FvCell& m) {
    if (m.volume <= 0.0) {
        a.negative += 1;
        if (a.first_negative < 0 || cell < a.first_negative) a.first_negative = cell;
    }
    fv_take_min(a.min_v, a.min_v_cell, m.volume, cell);
    fv_take_max(a.max_v, a.max_v_cell, m.volume, cell);
    fv_take_max(a.closed, a.closed_cell, m.closedness, cell);
    a.total_v += m.volume;
}
TM_WELD_HD void fv_acc_face(FvAcc& a, long long face, bool interior, double cosine, double skew) {
    if (interior && cosine < FV_COS_70) a.nonorth += 1;
    if (cosine <= 0.0) a.inverted += 1;
    fv_take_min(a.min_cos, a.cos_face, cosine, face);
    if (interior) fv_take_max(a.skew, a.skew_face, skew, face);
}

// The face-based view of a description at order 1: blocks, the segment table, counts.
struct FvPlan {
    std::vector<FvBlock> blocks;
    std::vector<FvSeg> segs;
    int64_t cells = 0, internal = 0, boundary = 0;
    int Eg = 1, npf = 2, fpc = 4;
    bool layered = false;
};
// sizes and counts only (closed form); TM_E_ARG when faces or cells do not fit int32_t
FvPlan fv_plan_counts(const tm_mesh_desc* mesh, const WeldPlan& pl, const WeldBoundaryPlan& bp, uint64_t nk);
// + the segment table and orientations; TM_E_MISMATCH for a cell that is its own neighbour or a connection whose two sides disagree
FvPlan fv_plan(const tm_mesh_desc* mesh, const WeldPlan& pl, const WeldBoundaryPlan& bp, uint64_t nk, const int32_t* orientation);
// owner and cell_faces slot of K19's boundary face t from its origin (block, side, e, g)
TM_WELD_HD int fv_origin_cell(const FvBlock* blocks, const int32_t* origin, int Eg) {
    const FvBlock& B = blocks[origin[0]];
    const int Ei = B.ni - 1, Ej = B.nj - 1, side = origin[1];
    int e, f;
    if (side >= 4) {
        f = origin[2] / Ei;
        e = origin[2] - f * Ei;
    } else {
        fv_seg_cell(Ei, Ej, side, origin[2], e, f);
    }
    return B.cell0 + (origin[3] * Ej + f) * Ei + e;
}
void fv_faces_host(const FvPlan& fp, const WeldBoundaryPlan& bp, const int32_t* map, int64_t nodes_out, const int32_t* boundary_faces, const int32_t* origin,
                   int32_t* faces, int32_t* owner, int32_t* neighbour, int32_t* cell_faces);

struct FvLists {
    int dim, npf, fpc;
    int64_t ncells, ninternal, nboundary, npoints;
    const int32_t *faces, *owner, *neighbour, *cell_faces;
};
// argument checks of tm_fv_metrics (TM_E_ARG), before anything is read or launched
FvLists fv_metrics_check(int dim, uint64_t ncells, uint64_t ninternal, uint64_t nboundary, const int32_t* faces, const int32_t* owner, const int32_t* neighbour,
                         const int32_t* cell_faces, uint64_t npoints, const double* const* points);
void fv_info_from(const FvLists& L, const FvAcc& a, tm_fv_info* info);

}  // namespace tmh
