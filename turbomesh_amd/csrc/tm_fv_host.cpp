// Host side of K21 (include/tm_hip.h, "faces of the welded mesh"): the plan -- counts in closed form, the table of the block-side
// segments with their partner cells -- and the host definition of the face lists and of the metrics.  No HIP call in this file: it works
// in a process without a device.
#include "tm_fv.hpp"
#include "tm_api_util.hpp"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

namespace tmh {

FvPlan fv_plan_counts(const tm_mesh_desc*, const WeldPlan& pl, const WeldBoundaryPlan& bp, uint64_t nk) {
    FvPlan fp;
    fp.layered = nk >= 2;
    fp.Eg = fp.layered ? static_cast<int>(nk - 1) : 1;
    fp.npf = fp.layered ? 4 : 2;
    fp.fpc = fp.layered ? 6 : 4;
    int64_t nseg = 0;
    for (const WeldBlock& b : pl.blocks) {
        FvBlock B{};
        B.off = b.off;
        B.ni = b.ni;
        B.nj = b.nj;
        B.orientation = 1;
        const int64_t here = static_cast<int64_t>(b.ni - 1) * (b.nj - 1) * fp.Eg;
        if (fp.cells + here > WELD_MAX_ID) throw TmError(TM_E_ARG, "more than 2^31 - 1 faces: face indices are int32_t");
        B.cell0 = static_cast<int32_t>(fp.cells);
        fp.cells += here;
        for (int s = 0; s < 4; ++s) {
            B.seg0[s] = static_cast<int32_t>(nseg);
            nseg += weld_side_length(b.ni, b.nj, s) - 1;
        }
        fp.blocks.push_back(B);
    }
    fp.boundary = bp.faces;
    fp.internal = (fp.fpc * fp.cells - fp.boundary) / 2;
    if (fp.internal + fp.boundary > WELD_MAX_ID) throw TmError(TM_E_ARG, "more than 2^31 - 1 faces: face indices are int32_t");
    fp.segs.assign(static_cast<size_t>(nseg), FvSeg{FV_BOUNDARY, -1, -1});
    return fp;
}

FvPlan fv_plan(const tm_mesh_desc* mesh, const WeldPlan& pl, const WeldBoundaryPlan& bp, uint64_t nk, const int32_t* orientation) {
    FvPlan fp = fv_plan_counts(mesh, pl, bp, nk);
    for (size_t b = 0; b < fp.blocks.size(); ++b) fp.blocks[b].orientation = orientation && orientation[b] < 0 ? -1 : 1;
    for (const tm_connection& c : pl.conns) {
        if (c.has_periodicity) continue;
        const int64_t len = weld_range_length(c.r[0].start, c.r[0].end);
        for (int s = 0; s < 2; ++s) {
            const tm_range &r = c.r[s], &q = c.r[1 - s];
            for (int64_t t = 0; t + 1 < len; ++t) {
                const int64_t seg = std::min(weld_range_pos(r.start, r.end, t), weld_range_pos(r.start, r.end, t + 1));
                const int64_t pseg = std::min(weld_range_pos(q.start, q.end, t), weld_range_pos(q.start, q.end, t + 1));
                FvSeg& slot = fp.segs[static_cast<size_t>(fp.blocks[r.block].seg0[r.side] + seg)];
                if (slot.block == FV_BOUNDARY) slot = FvSeg{static_cast<int32_t>(q.block), static_cast<int32_t>(q.side), static_cast<int32_t>(pseg)};
            }
        }
    }
    for (size_t b = 0; b < fp.blocks.size(); ++b) {
        const FvBlock& B = fp.blocks[b];
        for (int s = 0; s < 4; ++s) {
            const int n = weld_side_length(B.ni, B.nj, s) - 1;
            for (int k = 0; k < n; ++k) {
                const FvSeg& a = fp.segs[static_cast<size_t>(B.seg0[s] + k)];
                if (a.block == FV_BOUNDARY) continue;
                const std::string where = "block " + std::to_string(b) + ", side " + std::to_string(s) + ", segment " + std::to_string(k);
                const FvSeg& back = fp.segs[static_cast<size_t>(fp.blocks[a.block].seg0[a.side] + a.seg)];
                if (back.block != static_cast<int32_t>(b) || back.side != s || back.seg != k)
                    throw TmError(TM_E_MISMATCH, where + ": the segment behind it is connected elsewhere (overlapping connections)");
                int e, f, pe, pf;
                fv_seg_cell(B.ni - 1, B.nj - 1, s, k, e, f);
                fv_seg_cell(fp.blocks[a.block].ni - 1, fp.blocks[a.block].nj - 1, a.side, a.seg, pe, pf);
                if (a.block == static_cast<int32_t>(b) && pe == e && pf == f)
                    throw TmError(TM_E_MISMATCH, where + ": the cell is its own neighbour (a ring one cell around)");
            }
        }
    }
    return fp;
}

void fv_faces_host(const FvPlan& fp, const WeldBoundaryPlan&, const int32_t* map, int64_t nodes_out, const int32_t* boundary_faces, const int32_t* origin,
                   int32_t* faces, int32_t* owner, int32_t* neighbour, int32_t* cell_faces) {
    const int nb = static_cast<int>(fp.blocks.size()), npf = fp.npf, fpc = fp.fpc;
    int64_t at = 0;
    int nbr[6], sd[6], bk[6];
    for (int b = 0; b < nb; ++b) {
        const FvBlock& B = fp.blocks[b];
        const int Ei = B.ni - 1, Ej = B.nj - 1;
        for (int g = 0; g < fp.Eg; ++g)
            for (int f = 0; f < Ej; ++f)
                for (int e = 0; e < Ei; ++e) {
                    const int cell = B.cell0 + (g * Ej + f) * Ei + e;
                    const int n = fv_owned(fp.blocks.data(), fp.segs.data(), b, e, f, g, fp.Eg, fpc, cell, nbr, sd, bk);
                    if (at + n > fp.internal) throw TmError(TM_E_MISMATCH, "the connections yield more interior faces than the count of the plan");
                    for (int k = 0; k < n; ++k, ++at) {
                        owner[at] = cell;
                        neighbour[at] = nbr[k];
                        fv_cell_face(B, e, f, g, sd[k], fp.layered, map, static_cast<int>(nodes_out), faces + at * npf);
                        if (cell_faces) {
                            cell_faces[static_cast<size_t>(cell) * fpc + sd[k]] = static_cast<int32_t>(at);
                            cell_faces[static_cast<size_t>(nbr[k]) * fpc + bk[k]] = static_cast<int32_t>(at);
                        }
                    }
                }
    }
    if (at != fp.internal) throw TmError(TM_E_MISMATCH, "the connections yield fewer interior faces than the count of the plan");
    for (int64_t t = 0; t < fp.boundary; ++t) {
        const int64_t face = fp.internal + t;
        for (int q = 0; q < npf; ++q) faces[face * npf + q] = boundary_faces[t * npf + q];
        const int cell = fv_origin_cell(fp.blocks.data(), origin + 4 * t, fp.Eg);
        owner[face] = cell;
        if (cell_faces) cell_faces[static_cast<size_t>(cell) * fpc + origin[4 * t + 1]] = static_cast<int32_t>(face);
    }
}

FvLists fv_metrics_check(int dim, uint64_t ncells, uint64_t ninternal, uint64_t nboundary, const int32_t* faces, const int32_t* owner, const int32_t* neighbour,
                         const int32_t* cell_faces, uint64_t npoints, const double* const* points) {
    if (dim != 2 && dim != 3) throw TmError(TM_E_ARG, "dim: 2 (edges of a plane mesh) or 3 (quadrilaterals of a stacked one)");
    const uint64_t top = static_cast<uint64_t>(WELD_MAX_ID);
    if (ncells == 0 || ncells > top || ninternal > top || nboundary > top || ninternal + nboundary > top || npoints > top)
        throw TmError(TM_E_ARG, "no cells, or more than 2^31 - 1 cells, faces or points");
    if (!faces || !owner || (ninternal && !neighbour) || !cell_faces || !points) throw TmError(TM_E_ARG, "null argument");
    for (int c = 0; c < dim; ++c)
        if (!points[c]) throw TmError(TM_E_ARG, "null coordinate plane");
    FvLists L{dim, dim == 2 ? 2 : 4, dim == 2 ? 4 : 6, static_cast<int64_t>(ncells), static_cast<int64_t>(ninternal), static_cast<int64_t>(nboundary),
              static_cast<int64_t>(npoints), faces, owner, neighbour, cell_faces};
    const int64_t nfaces = L.ninternal + L.nboundary;
    const uint32_t plimit = static_cast<uint32_t>(npoints), climit = static_cast<uint32_t>(ncells), flimit = static_cast<uint32_t>(nfaces);
    for (int64_t k = 0; k < nfaces * L.npf; ++k)
        if (static_cast<uint32_t>(faces[k]) >= plimit) throw TmError(TM_E_ARG, "face " + std::to_string(k / L.npf) + " names point " + std::to_string(faces[k]) + " of " + std::to_string(npoints));
    int32_t last = 0;
    for (int64_t f = 0; f < nfaces; ++f) {
        if (static_cast<uint32_t>(owner[f]) >= climit) throw TmError(TM_E_ARG, "face " + std::to_string(f) + ": owner " + std::to_string(owner[f]) + " of " + std::to_string(ncells) + " cells");
        if (f >= L.ninternal) continue;
        if (owner[f] < last) throw TmError(TM_E_ARG, "face " + std::to_string(f) + ": the owners of the internal faces decrease");
        last = owner[f];
        if (static_cast<uint32_t>(neighbour[f]) >= climit || neighbour[f] <= owner[f])
            throw TmError(TM_E_ARG, "face " + std::to_string(f) + ": neighbour " + std::to_string(neighbour[f]) + " is not a cell above its owner");
    }
    for (int64_t c = 0; c < L.ncells; ++c)
        for (int k = 0; k < L.fpc; ++k) {
            const int32_t f = cell_faces[c * L.fpc + k];
            if (static_cast<uint32_t>(f) >= flimit || (owner[f] != c && !(f < L.ninternal && neighbour[f] == c)))
                throw TmError(TM_E_ARG, "cell " + std::to_string(c) + ", side " + std::to_string(k) + ": face " + std::to_string(f) + " is not a face of this cell");
        }
    return L;
}

void fv_info_from(const FvLists& L, const FvAcc& a, tm_fv_info* info) {
    if (!info) return;
    auto idx = [](long long v) { return v < 0 ? 0ull : static_cast<uint64_t>(v); };
    std::memset(info, 0, sizeof(*info));
    info->cells = static_cast<uint64_t>(L.ncells);
    info->internal_faces = static_cast<uint64_t>(L.ninternal);
    info->boundary_faces = static_cast<uint64_t>(L.nboundary);
    info->min_volume_cell = idx(a.min_v_cell);
    info->max_volume_cell = idx(a.max_v_cell);
    info->negative_cells = static_cast<uint64_t>(a.negative);
    info->first_negative_cell = idx(a.first_negative);
    info->max_closedness_cell = idx(a.closed_cell);
    info->min_cos_face = idx(a.cos_face);
    info->nonorthogonal_faces = static_cast<uint64_t>(a.nonorth);
    info->inverted_faces = static_cast<uint64_t>(a.inverted);
    info->max_skewness_face = idx(a.skew_face);
    info->min_volume = a.min_v;
    info->max_volume = a.max_v;
    info->total_volume = a.total_v;
    info->max_closedness = a.closed;
    info->min_cos = a.min_cos;
    info->max_skewness = a.skew;
}

namespace {

void face_points(const FvLists& L, const double* const* points, int64_t face, double P[4][3]) {
    for (int q = 0; q < L.npf; ++q) {
        const int32_t id = L.faces[face * L.npf + q];
        for (int c = 0; c < 3; ++c) P[q][c] = c < L.dim ? points[c][id] : 0.0;
    }
}

void metrics_host(const FvLists& L, const double* const* points, const tm_fv_fields* out, tm_fv_info* info) {
    const int64_t nfaces = L.ninternal + L.nboundary;
    std::vector<double> centre(static_cast<size_t>(L.ncells) * 3);
    FvAcc acc;
    fv_acc_init(acc);
    double P[4][3], S[6][3], Cf[6][3], sign[6];
    for (int64_t cell = 0; cell < L.ncells; ++cell) {
        for (int k = 0; k < L.fpc; ++k) {
            const int32_t face = L.cell_faces[cell * L.fpc + k];
            face_points(L, points, face, P);
            fv_face_geometry(L.dim, P, S[k], Cf[k]);
            sign[k] = L.owner[face] == cell ? 1.0 : -1.0;
        }
        const FvCell m = fv_cell_metrics(L.dim, L.fpc, S, Cf, sign);
        for (int c = 0; c < 3; ++c) centre[static_cast<size_t>(cell) * 3 + c] = m.centre[c];
        fv_acc_cell(acc, cell, m);
        if (out && out->volume) out->volume[cell] = m.volume;
        if (out && out->closedness) out->closedness[cell] = m.closedness;
        if (out && out->centre)
            for (int c = 0; c < L.dim; ++c) out->centre[static_cast<size_t>(c) * L.ncells + cell] = m.centre[c];
    }
    for (int64_t face = 0; face < nfaces; ++face) {
        double s[3], cf[3], d[3];
        face_points(L, points, face, P);
        fv_face_geometry(L.dim, P, s, cf);
        const double* Cown = centre.data() + static_cast<size_t>(L.owner[face]) * 3;
        const bool interior = face < L.ninternal;
        const double* Cnb = interior ? centre.data() + static_cast<size_t>(L.neighbour[face]) * 3 : cf;
        for (int c = 0; c < 3; ++c) d[c] = Cnb[c] - Cown[c];
        const double cosine = fv_cos(d, s), skew = interior ? fv_skewness(Cown, Cnb, cf, s) : 0.0;
        fv_acc_face(acc, face, interior, cosine, skew);
        if (out && out->cos) out->cos[face] = cosine;
        if (out && out->skewness && interior) out->skewness[face] = skew;
        for (int c = 0; c < L.dim; ++c) {
            if (out && out->area) out->area[static_cast<size_t>(c) * nfaces + face] = s[c];
            if (out && out->face_centre) out->face_centre[static_cast<size_t>(c) * nfaces + face] = cf[c];
        }
    }
    fv_info_from(L, acc, info);
}

}  // namespace

}  // namespace tmh

using namespace tmh;

extern "C" int tm_weld_faces_plan(const tm_mesh_desc* mesh, uint64_t nk, tm_fv_plan* plan) {
    return guarded([&]() {
        if (!plan) throw TmError(TM_E_ARG, "null argument");
        const WeldPlan pl = weld_plan(mesh);
        const WeldBoundaryPlan bp = weld_boundary_plan(mesh, pl, 1, nk);
        const FvPlan fp = fv_plan_counts(mesh, pl, bp, nk);
        plan->cells = static_cast<uint64_t>(fp.cells);
        plan->internal_faces = static_cast<uint64_t>(fp.internal);
        plan->boundary_faces = static_cast<uint64_t>(fp.boundary);
        plan->nodes_per_face = static_cast<uint64_t>(fp.npf);
        plan->faces_per_cell = static_cast<uint64_t>(fp.fpc);
        return TM_OK;
    });
}

extern "C" int tm_weld_faces_host(const tm_mesh_desc* mesh, const int32_t* map, uint64_t nodes_out, uint64_t nk, const int32_t* block_orientation,
                                  int32_t* faces, int32_t* owner, int32_t* neighbour, int32_t* cell_faces) {
    return guarded([&]() {
        weld_layers(nk, nodes_out);   // sizes first: nothing is read when the ids cannot be held
        const WeldPlan pl = weld_plan(mesh);
        const WeldBoundaryPlan bp = weld_boundary_plan(mesh, pl, 1, nk);
        const FvPlan fp = fv_plan(mesh, pl, bp, nk, block_orientation);
        if (!map || !faces || !owner || (!neighbour && fp.internal)) throw TmError(TM_E_ARG, "null argument");
        std::vector<int32_t> bfaces(static_cast<size_t>(bp.faces) * bp.npf), origin(static_cast<size_t>(bp.faces) * 4);
        weld_boundary_faces_host(pl, bp, map, static_cast<int64_t>(nodes_out), nk, block_orientation, bfaces.data());
        weld_boundary_labels(pl, bp, nullptr, origin.data());
        fv_faces_host(fp, bp, map, static_cast<int64_t>(nodes_out), bfaces.data(), origin.data(), faces, owner, neighbour, cell_faces);
        return TM_OK;
    });
}

extern "C" int tm_fv_metrics_host(int32_t dim, uint64_t ncells, uint64_t ninternal, uint64_t nboundary, const int32_t* faces, const int32_t* owner,
                                  const int32_t* neighbour, const int32_t* cell_faces, uint64_t npoints, const double* const* points,
                                  const tm_fv_fields* fields, tm_fv_info* info) {
    return guarded([&]() {
        const FvLists L = fv_metrics_check(dim, ncells, ninternal, nboundary, faces, owner, neighbour, cell_faces, npoints, points);
        metrics_host(L, points, fields, info);
        return TM_OK;
    });
}
