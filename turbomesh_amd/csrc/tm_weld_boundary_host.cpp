// Host side of K19 (include/tm_hip.h, "boundary of the welded mesh"): the plan -- every segment of every side classified by the ranges of
// the description, the patch table with its CSR, loops and irregular nodes of the plane boundary -- and the host definition of the face
// lists and of the measures.  No HIP call in this file: it works in a process without a device.
#include "tm_weld_boundary.hpp"
#include "tm_api_util.hpp"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

namespace tmh {

namespace {

struct SideSegs {   // the segments of one side of one block
    int first = 0, count = 0;
};
constexpr int SEG_INTERIOR = -2, SEG_FREE = -1;

std::string range_text(const tm_range& r) {
    return "(block " + std::to_string(r.block) + ", side " + std::to_string(r.side) + ", nodes " + std::to_string(r.start) + " .. " + std::to_string(r.end) + ")";
}

int find_root(std::vector<int32_t>& parent, int x) {
    int r = x;
    while (parent[r] != r) r = parent[r];
    while (parent[x] != r) {
        const int next = parent[x];
        parent[x] = r;
        x = next;
    }
    return r;
}
void unite(std::vector<int32_t>& parent, int a, int b) {
    a = find_root(parent, a);
    b = find_root(parent, b);
    if (a < b) parent[b] = a;
    else if (b < a) parent[a] = b;
}

}  // namespace

WeldBoundaryPlan weld_boundary_plan(const tm_mesh_desc* mesh, const WeldPlan& pl, int order, uint64_t nk) {
    WeldBoundaryPlan bp;
    weld_cells_plan(mesh, pl, order, nk, bp.cells_of);   // tm_ho_check / tm_ho3_check: the order, the sizes, the connection ranges
    if (mesh->nbcs && !mesh->bcs) throw TmError(TM_E_ARG, "null condition array");
    if (mesh->nbcs > 65535u) throw TmError(TM_E_ARG, "more than 65535 conditions");
    const int p = order, nb = pl.nblocks();
    bp.p = p;
    bp.layered = nk >= 2;
    bp.Eg = bp.layered ? static_cast<int64_t>(nk - 1) / p : 1;
    bp.npf = bp.layered ? (p + 1) * (p + 1) : p + 1;
    {   // cells_of counts span elements too: the caps want the plane elements
        bp.cells_of.assign(1, 0);
        for (const WeldBlock& b : pl.blocks) bp.cells_of.push_back(bp.cells_of.back() + static_cast<int64_t>((b.ni - 1) / p) * ((b.nj - 1) / p));
    }
    // the segment table: block, side 0 .. 3, e
    std::vector<SideSegs> sides(static_cast<size_t>(nb) * 4);
    int nseg = 0;
    for (int b = 0; b < nb; ++b)
        for (int s = 0; s < 4; ++s) {
            sides[b * 4 + s] = SideSegs{nseg, (weld_side_length(pl.blocks[b].ni, pl.blocks[b].nj, s) - 1) / p};
            nseg += sides[b * 4 + s].count;
        }
    std::vector<int32_t> owner(nseg, SEG_FREE);   // SEG_INTERIOR, SEG_FREE or the patch
    auto cover = [&](const tm_range& r, int value) {   // the segments a range covers take `value` unless they are taken
        const int64_t lo = static_cast<int64_t>(std::min(r.start, r.end)), hi = static_cast<int64_t>(std::max(r.start, r.end));
        const SideSegs& ss = sides[r.block * 4 + r.side];
        for (int64_t e = (lo + p - 1) / p; e < ss.count && (e + 1) * p <= hi; ++e)
            if (owner[ss.first + e] == SEG_FREE) owner[ss.first + e] = value;
    };
    const int nbcs = static_cast<int>(mesh->nbcs);
    for (int c = 0; c < nbcs; ++c) {   // conditions are not seen by weld_plan: the same checks
        const tm_range& r = mesh->bcs[c].range;
        if (r.block >= mesh->nblocks) throw TmError(TM_E_ARG, "condition " + std::to_string(c) + " names block " + std::to_string(r.block) + " past the mesh");
        if (r.side > TM_SIDE_J_MAX) throw TmError(TM_E_ARG, "condition " + std::to_string(c) + ": side " + std::to_string(r.side) + " does not exist");
        const uint64_t n = static_cast<uint64_t>(weld_side_length(pl.blocks[r.block].ni, pl.blocks[r.block].nj, r.side));
        if (r.start >= n || r.end >= n) throw TmError(TM_E_MISMATCH, "condition " + std::to_string(c) + " " + range_text(r) + " leaves its side of " + std::to_string(n) + " nodes");
        if (r.start != r.end && (r.start % p != 0 || r.end % p != 0))
            throw TmError(TM_E_MISMATCH, "condition " + std::to_string(c) + " " + range_text(r) + " covers a part of a segment only: it does not lie on the element grid of order " +
                                             std::to_string(p));
    }
    for (const tm_connection& c : pl.conns)
        if (!c.has_periodicity)
            for (int s = 0; s < 2; ++s) cover(c.r[s], SEG_INTERIOR);
    int nper = 0;
    for (const tm_connection& c : pl.conns)
        if (c.has_periodicity) {
            for (int s = 0; s < 2; ++s) cover(c.r[s], nbcs + 2 * nper + s);
            ++nper;
        }
    for (int c = 0; c < nbcs; ++c) cover(mesh->bcs[c].range, c);
    const int unassigned = nbcs + 2 * nper;
    for (int32_t& o : owner)
        if (o == SEG_FREE) o = unassigned;
    // the patches
    bp.patches.assign(static_cast<size_t>(unassigned + 1 + (bp.layered ? 2 : 0)), tm_weld_patch{});
    for (tm_weld_patch& q : bp.patches) q.source = q.partner = -1;
    for (int c = 0; c < nbcs; ++c) {
        bp.patches[c].kind = static_cast<int32_t>(mesh->bcs[c].kind);
        bp.patches[c].source = c;
    }
    {
        int k = 0;
        for (size_t c = 0; c < pl.conns.size(); ++c) {
            if (!pl.conns[c].has_periodicity) continue;
            for (int s = 0; s < 2; ++s) {
                tm_weld_patch& q = bp.patches[nbcs + 2 * k + s];
                q.kind = TM_PATCH_PERIODIC;
                q.source = static_cast<int32_t>(c);
                q.partner = nbcs + 2 * k + (1 - s);
                for (int d = 0; d < 2; ++d) q.translation[d] = s == 0 ? pl.conns[c].periodicity[d] : -pl.conns[c].periodicity[d];
            }
            ++k;
        }
    }
    bp.patches[unassigned].kind = TM_PATCH_UNASSIGNED;
    // segments in face order
    std::vector<std::vector<WbSeg>> of_patch(static_cast<size_t>(unassigned) + 1);
    std::vector<char> listed(nseg, 0);
    {
        int k = 0;
        for (const tm_connection& c : pl.conns) {   // periodic patches: along the connection's own pair order
            if (!c.has_periodicity) continue;
            const int64_t elements = (weld_range_length(c.r[0].start, c.r[0].end) - 1) / p;
            for (int s = 0; s < 2; ++s) {
                const tm_range& r = c.r[s];
                const SideSegs& ss = sides[r.block * 4 + r.side];
                const int q = nbcs + 2 * k + s;
                for (int64_t t = 0; t < elements; ++t) {
                    const int64_t e = std::min(weld_range_pos(r.start, r.end, t * p), weld_range_pos(r.start, r.end, (t + 1) * p)) / p;
                    if (owner[ss.first + e] != q || listed[ss.first + e]) continue;
                    listed[ss.first + e] = 1;
                    of_patch[q].push_back(WbSeg{static_cast<int32_t>(r.block), static_cast<int32_t>(r.side), static_cast<int32_t>(e), q, 0, 0});
                }
            }
            ++k;
        }
    }
    for (int b = 0; b < nb; ++b)
        for (int s = 0; s < 4; ++s) {
            const SideSegs& ss = sides[b * 4 + s];
            for (int e = 0; e < ss.count; ++e) {
                const int q = owner[ss.first + e];
                if (q == SEG_INTERIOR || bp.patches[q].kind == TM_PATCH_PERIODIC) continue;
                of_patch[q].push_back(WbSeg{b, s, e, q, 0, 0});
            }
        }
    int64_t at = 0;
    for (int q = 0; q <= unassigned; ++q) {
        const int64_t n = static_cast<int64_t>(of_patch[q].size());
        bp.patches[q].face_begin = static_cast<uint64_t>(at);
        bp.patches[q].faces = static_cast<uint64_t>(n * bp.Eg);
        for (int64_t k = 0; k < n; ++k) {
            WbSeg s = of_patch[q][k];
            if (at + n * bp.Eg > WELD_MAX_ID) throw TmError(TM_E_ARG, "more than 2^31 - 1 boundary faces");
            s.face0 = static_cast<int32_t>(at + k);
            s.stride = static_cast<int32_t>(n);
            bp.segs.push_back(s);
        }
        at += n * bp.Eg;
    }
    bp.lateral_faces = at;
    if (bp.layered) {
        bp.cap_faces = bp.cells_of.back();
        if (at + 2 * bp.cap_faces > WELD_MAX_ID) throw TmError(TM_E_ARG, "more than 2^31 - 1 boundary faces");
        bp.hub_begin = at;
        bp.shroud_begin = at + bp.cap_faces;
        tm_weld_patch& hub = bp.patches[unassigned + 1];
        tm_weld_patch& shroud = bp.patches[unassigned + 2];
        hub.kind = TM_PATCH_HUB;
        shroud.kind = TM_PATCH_SHROUD;
        hub.face_begin = static_cast<uint64_t>(bp.hub_begin);
        shroud.face_begin = static_cast<uint64_t>(bp.shroud_begin);
        hub.faces = shroud.faces = static_cast<uint64_t>(bp.cap_faces);
        at += 2 * bp.cap_faces;
    }
    bp.faces = at;
    // loops and irregular nodes of the plane boundary: welded nodes are the classes of the perimeter slots
    std::vector<int32_t> node(static_cast<size_t>(pl.slots));
    for (size_t s = 0; s < node.size(); ++s) node[s] = static_cast<int32_t>(s);
    for (const tm_connection& c : pl.conns) {
        if (c.has_periodicity) continue;
        const int64_t len = weld_range_length(c.r[0].start, c.r[0].end);
        for (int64_t t = 0; t < len; ++t) unite(node, pl.slot_of(c.r[0], t), pl.slot_of(c.r[1], t));
    }
    std::vector<int32_t> comp(node.size()), degree(node.size(), 0);
    for (size_t s = 0; s < comp.size(); ++s) comp[s] = static_cast<int32_t>(s);
    for (const WbSeg& s : bp.segs) {
        int end[2];
        for (int k = 0; k < 2; ++k) {
            const WeldBlock& B = pl.blocks[s.block];
            int i, j;
            weld_side_node(B.ni, B.nj, s.side, (s.e + k) * p, i, j);
            end[k] = find_root(node, B.slot0 + weld_slot(B.ni, B.nj, i, j));
            degree[end[k]] += 1;
        }
        unite(comp, end[0], end[1]);
    }
    for (size_t s = 0; s < degree.size(); ++s) {
        if (!degree[s]) continue;
        if (degree[s] != 2) bp.irregular += 1;
        if (find_root(comp, static_cast<int>(s)) == static_cast<int>(s)) bp.loops += 1;
    }
    return bp;
}

void weld_boundary_labels(const WeldPlan& pl, const WeldBoundaryPlan& bp, int32_t* face_patch, int32_t* origin) {
    for (const WbSeg& s : bp.segs)
        for (int64_t g = 0; g < bp.Eg; ++g) {
            const size_t f = static_cast<size_t>(s.face0 + g * s.stride);
            if (face_patch) face_patch[f] = s.patch;
            if (origin) {
                origin[4 * f + 0] = s.block;
                origin[4 * f + 1] = s.side;
                origin[4 * f + 2] = s.e;
                origin[4 * f + 3] = static_cast<int32_t>(g);
            }
        }
    if (!bp.layered) return;
    const int hub = static_cast<int>(bp.patches.size()) - 2;
    for (int cap = 0; cap < 2; ++cap)
        for (int b = 0; b < pl.nblocks(); ++b)
            for (int64_t el = 0; el < bp.cells_of[b + 1] - bp.cells_of[b]; ++el) {
                const size_t f = static_cast<size_t>((cap ? bp.shroud_begin : bp.hub_begin) + bp.cells_of[b] + el);
                if (face_patch) face_patch[f] = hub + cap;
                if (origin) {
                    origin[4 * f + 0] = b;
                    origin[4 * f + 1] = cap ? WB_SIDE_SHROUD : WB_SIDE_HUB;
                    origin[4 * f + 2] = static_cast<int32_t>(el);
                    origin[4 * f + 3] = cap ? static_cast<int32_t>(bp.Eg - 1) : 0;
                }
            }
}

std::vector<int32_t> weld_quad_inverse(int p) {
    const std::vector<int32_t> local = weld_local_order(p, false);
    std::vector<int32_t> inv(local.size());
    for (size_t q = 0; q < local.size(); ++q) inv[((local[q] >> 8) & 255) * (p + 1) + (local[q] & 255)] = static_cast<int32_t>(q);
    return inv;
}

void weld_boundary_faces_host(const WeldPlan& pl, const WeldBoundaryPlan& bp, const int32_t* map, int64_t nodes_out, uint64_t nk, const int32_t* orientation,
                              int32_t* faces) {
    const int p = bp.p, npf = bp.npf;
    auto o_of = [&](int b) { return orientation && orientation[b] < 0 ? -1 : 1; };
    const std::vector<int32_t> quad = weld_local_order(p, false);
    for (const WbSeg& s : bp.segs) {
        const WeldBlock& B = pl.blocks[s.block];
        for (int64_t g = 0; g < bp.Eg; ++g) {
            int32_t* out = faces + static_cast<size_t>(s.face0 + g * s.stride) * npf;
            if (!bp.layered) {
                for (int a = 0; a <= p; ++a) out[wb_curve_local(p, a)] = map[B.off + wb_seg_node(B, s.side, p, s.e, a, o_of(s.block))];
            } else {
                for (int q = 0; q < npf; ++q) {
                    const int a = quad[q] & 255, c = (quad[q] >> 8) & 255;
                    out[q] = static_cast<int32_t>((g * p + c) * nodes_out + map[B.off + wb_seg_node(B, s.side, p, s.e, a, o_of(s.block))]);
                }
            }
        }
    }
    if (!bp.layered) return;
    const int64_t top = static_cast<int64_t>(nk - 1) * nodes_out;
    for (int b = 0; b < pl.nblocks(); ++b) {
        const WeldBlock& B = pl.blocks[b];
        const int Ei = (B.ni - 1) / p, Ej = (B.nj - 1) / p;
        for (int f = 0; f < Ej; ++f)
            for (int e = 0; e < Ei; ++e) {
                const size_t el = static_cast<size_t>(bp.cells_of[b]) + static_cast<size_t>(f) * Ei + e;
                int32_t* hub = faces + (static_cast<size_t>(bp.hub_begin) + el) * npf;
                int32_t* shroud = faces + (static_cast<size_t>(bp.shroud_begin) + el) * npf;
                for (int q = 0; q < npf; ++q) {
                    const int a = quad[q] & 255, c = (quad[q] >> 8) & 255;
                    hub[q] = map[B.off + wb_cap_node(B, false, p, e, f, a, c, o_of(b))];
                    shroud[q] = static_cast<int32_t>(top + map[B.off + wb_cap_node(B, true, p, e, f, a, c, o_of(b))]);
                }
            }
    }
}

int weld_measure_check(int dim, int order, uint64_t nfaces, const int32_t* faces, const int32_t* face_patch, uint64_t npatches, uint64_t npoints, int ncomp,
                       const double* const* points, const tm_weld_patch* patches) {
    if (dim != 2 && dim != 3) throw TmError(TM_E_ARG, "dim: 2 (curves of a plane mesh) or 3 (quadrilaterals of a stacked one)");
    const int top = dim == 2 ? TM_HO_MAX_ORDER : TM_HO3_MAX_ORDER;
    if (order < 1 || order > top) throw TmError(TM_E_ARG, "order " + std::to_string(order) + ": 1 .. " + std::to_string(top));
    if (ncomp < dim || ncomp > 3) throw TmError(TM_E_ARG, "ncomp: " + std::to_string(dim) + " .. 3 coordinate planes");
    if (!patches || npatches == 0 || npatches > static_cast<uint64_t>(WELD_MAX_ID)) throw TmError(TM_E_ARG, "patches are needed");
    if (nfaces > static_cast<uint64_t>(WELD_MAX_ID) || npoints > static_cast<uint64_t>(WELD_MAX_ID)) throw TmError(TM_E_ARG, "more than 2^31 - 1 faces or points");
    if (!points || (nfaces && (!faces || !face_patch))) throw TmError(TM_E_ARG, "null argument");
    for (int c = 0; c < dim; ++c)
        if (!points[c]) throw TmError(TM_E_ARG, "null coordinate plane");
    const int npf = dim == 2 ? order + 1 : (order + 1) * (order + 1);
    int32_t last = 0;
    for (uint64_t f = 0; f < nfaces; ++f) {
        const int32_t q = face_patch[f];
        if (q < last || static_cast<uint64_t>(q) >= npatches) throw TmError(TM_E_ARG, "face " + std::to_string(f) + ": its patch " + std::to_string(q) + " decreases or is past the patches");
        last = q;
    }
    const size_t n = static_cast<size_t>(nfaces) * npf;
    const uint32_t limit = static_cast<uint32_t>(npoints);
    for (size_t k = 0; k < n; ++k)
        if (static_cast<uint32_t>(faces[k]) >= limit) throw TmError(TM_E_ARG, "face " + std::to_string(k / npf) + " names point " + std::to_string(faces[k]) + " of " + std::to_string(npoints));
    return npf;
}

void weld_faces_measure_host(int dim, int p, uint64_t nfaces, const int32_t* faces, const int32_t* face_patch, uint64_t npatches, const double* const* points,
                             tm_weld_patch* patches) {
    std::vector<double> acc(static_cast<size_t>(npatches) * WB_TERMS, 0.0);
    const int npf = dim == 2 ? p + 1 : (p + 1) * (p + 1), n1 = p + 1;
    const std::vector<int32_t> inv = dim == 3 ? weld_quad_inverse(p) : std::vector<int32_t>();
    double t[WB_TERMS];
    for (uint64_t f = 0; f < nfaces; ++f) {
        const int32_t* ids = faces + static_cast<size_t>(f) * npf;
        double* sum = acc.data() + static_cast<size_t>(face_patch[f]) * WB_TERMS;
        if (dim == 2) {
            for (int a = 0; a < p; ++a) {
                const int A = ids[wb_curve_local(p, a)], B = ids[wb_curve_local(p, a + 1)];
                wb_edge_terms(points[0][A], points[1][A], points[0][B], points[1][B], t);
                for (int k = 0; k < WB_TERMS; ++k) sum[k] += t[k];
            }
        } else {
            for (int c = 0; c < p; ++c)
                for (int a = 0; a < p; ++a) {
                    const int corner[4] = {ids[inv[c * n1 + a]], ids[inv[c * n1 + a + 1]], ids[inv[(c + 1) * n1 + a + 1]], ids[inv[(c + 1) * n1 + a]]};
                    double P[4][3];
                    for (int k = 0; k < 4; ++k)
                        for (int d = 0; d < 3; ++d) P[k][d] = points[d][corner[k]];
                    wb_quad_terms(P[0], P[1], P[2], P[3], t);
                    for (int k = 0; k < WB_TERMS; ++k) sum[k] += t[k];
                }
        }
    }
    for (uint64_t q = 0; q < npatches; ++q) {
        const double* s = acc.data() + q * WB_TERMS;
        patches[q].measure = s[0];
        patches[q].normal[0] = s[1];
        patches[q].normal[1] = s[2];
        patches[q].normal[2] = s[3];
        patches[q].moment = s[4];
    }
}

}  // namespace tmh

using namespace tmh;

extern "C" int tm_weld_boundary_plan(const tm_mesh_desc* mesh, int32_t order, uint64_t nk, tm_weld_boundary_info* info, tm_weld_patch* patches) {
    return guarded([&]() {
        const WeldPlan pl = weld_plan(mesh);
        const WeldBoundaryPlan bp = weld_boundary_plan(mesh, pl, order, nk);
        if (info) {
            info->patches = bp.patches.size();
            info->faces = static_cast<uint64_t>(bp.faces);
            info->nodes_per_face = static_cast<uint64_t>(bp.npf);
            info->lateral_faces = static_cast<uint64_t>(bp.lateral_faces);
            info->cap_faces = static_cast<uint64_t>(2 * bp.cap_faces);
            info->loops = bp.loops;
            info->irregular_nodes = bp.irregular;
        }
        if (patches) std::memcpy(patches, bp.patches.data(), sizeof(tm_weld_patch) * bp.patches.size());
        return TM_OK;
    });
}

extern "C" int tm_weld_boundary_faces_host(const tm_mesh_desc* mesh, const int32_t* map, uint64_t nodes_out, int32_t order, uint64_t nk,
                                           const int32_t* block_orientation, int32_t* faces, int32_t* face_patch, int32_t* origin) {
    return guarded([&]() {
        weld_layers(nk, nodes_out);   // sizes first: nothing is read when the ids cannot be held
        const WeldPlan pl = weld_plan(mesh);
        const WeldBoundaryPlan bp = weld_boundary_plan(mesh, pl, order, nk);
        if (!map || (!faces && bp.faces)) throw TmError(TM_E_ARG, "null argument");
        weld_boundary_faces_host(pl, bp, map, static_cast<int64_t>(nodes_out), nk, block_orientation, faces);
        weld_boundary_labels(pl, bp, face_patch, origin);
        return TM_OK;
    });
}

extern "C" int tm_weld_faces_measure_host(int32_t dim, int32_t order, uint64_t nfaces, const int32_t* faces, const int32_t* face_patch, uint64_t npatches,
                                          uint64_t npoints, int32_t ncomp, const double* const* points, tm_weld_patch* patches) {
    return guarded([&]() {
        weld_measure_check(dim, order, nfaces, faces, face_patch, npatches, npoints, ncomp, points, patches);
        weld_faces_measure_host(dim, order, nfaces, faces, face_patch, npatches, points, patches);
        return TM_OK;
    });
}
