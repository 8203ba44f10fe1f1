// Host side of K18 (include/tm_hip.h, "welded unstructured mesh"): validation of a mesh description, the local node orders of VTK's
// Lagrange cells, and the host definition of every stage -- classes by a sequential union-find on the perimeter slots, first-occurrence
// numbering, points of the owners, cells, periodic pairs.  No HIP call in this file: it works in a process without a device.
#include "tm_weld.hpp"
#include "tm_api_util.hpp"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace tmh {

WeldPlan weld_plan(const tm_mesh_desc* mesh) {
    if (!mesh || !mesh->blocks || mesh->nblocks == 0) throw TmError(TM_E_ARG, "mesh description without blocks");
    if (mesh->nconns && !mesh->conns) throw TmError(TM_E_ARG, "null connection array");
    if (mesh->nblocks > 65535u || mesh->nconns > 65535u) throw TmError(TM_E_ARG, "more than 65535 blocks or connections");
    WeldPlan pl;
    for (uint64_t b = 0; b < mesh->nblocks; ++b) {
        const uint64_t ni = mesh->blocks[b].ni, nj = mesh->blocks[b].nj;
        if (ni < 2 || nj < 2) throw TmError(TM_E_SIZE, "InconsistentSize: block " + std::to_string(b) + " has fewer than 2 nodes in a direction");
        if (ni > static_cast<uint64_t>(WELD_MAX_ID) || nj > static_cast<uint64_t>(WELD_MAX_ID) || ni * nj > static_cast<uint64_t>(WELD_MAX_ID - pl.nodes))
            throw TmError(TM_E_ARG, "the mesh has more than 2^31 - 1 nodes: welded ids are int32_t");
        pl.blocks.push_back(WeldBlock{static_cast<int32_t>(pl.nodes), static_cast<int32_t>(pl.slots), static_cast<int32_t>(ni), static_cast<int32_t>(nj)});
        pl.nodes += static_cast<int64_t>(ni * nj);
        pl.slots += weld_perimeter(static_cast<int>(ni), static_cast<int>(nj));
    }
    for (uint64_t c = 0; c < mesh->nconns; ++c) {
        const tm_connection& cn = mesh->conns[c];
        int64_t len[2];
        for (int s = 0; s < 2; ++s) {
            const tm_range& r = cn.r[s];
            if (r.block >= mesh->nblocks) throw TmError(TM_E_ARG, "connection " + std::to_string(c) + " names block " + std::to_string(r.block) + " past the mesh");
            if (r.side > TM_SIDE_J_MAX) throw TmError(TM_E_ARG, "connection " + std::to_string(c) + ": side " + std::to_string(r.side) + " does not exist");
            const uint64_t n = static_cast<uint64_t>(weld_side_length(pl.blocks[r.block].ni, pl.blocks[r.block].nj, r.side));
            if (r.start >= n || r.end >= n)
                throw TmError(TM_E_MISMATCH, "connection " + std::to_string(c) + " range " + std::to_string(s) + " (" + std::to_string(r.start) + " .. " + std::to_string(r.end) +
                                                 ") leaves its side of " + std::to_string(n) + " nodes");
            len[s] = weld_range_length(r.start, r.end);
        }
        if (len[0] != len[1])
            throw TmError(TM_E_MISMATCH, "connection " + std::to_string(c) + ": ranges of " + std::to_string(len[0]) + " and " + std::to_string(len[1]) + " nodes");
        if (cn.has_periodicity) pl.periodic_pairs += len[0];
        else if (len[0] > pl.max_pairs) pl.max_pairs = len[0];
        pl.conns.push_back(cn);
    }
    return pl;
}

int64_t weld_layers(uint64_t nk, uint64_t nodes_out) {
    const uint64_t layers = nk < 1 ? 1 : nk;
    if (nodes_out > static_cast<uint64_t>(WELD_MAX_ID) || layers > static_cast<uint64_t>(WELD_MAX_ID) || layers * nodes_out > static_cast<uint64_t>(WELD_MAX_ID))
        throw TmError(TM_E_ARG, std::to_string(layers) + " layers of " + std::to_string(nodes_out) + " welded nodes exceed 2^31 - 1: welded ids are int32_t");
    return static_cast<int64_t>(layers);
}

void weld_cells_plan(const tm_mesh_desc* mesh, const WeldPlan& pl, int order, uint64_t nk, std::vector<int64_t>& cells_of) {
    tm_ho_opt ho{};
    ho.order = order;
    ho.distribution = TM_HO_EQUIDISTANT;
    int rc;
    if (nk >= 2) {   // hexahedra: the size rule and the order limit of "high-order hexahedra of stacked blocks"
        tm_stack_opt st{};
        st.nlayers = nk;
        rc = tm_ho3_check(mesh, &st, &ho);
    } else {
        rc = tm_ho_check(mesh, &ho);
    }
    if (rc < 0) throw TmError(rc, g_last_error);
    const int64_t Eg = nk >= 2 ? static_cast<int64_t>(nk - 1) / order : 1;
    cells_of.assign(1, 0);
    for (const WeldBlock& b : pl.blocks) {
        const int64_t n = static_cast<int64_t>((b.ni - 1) / order) * ((b.nj - 1) / order) * Eg;
        if (n > WELD_MAX_ID) throw TmError(TM_E_ARG, "a block with more than 2^31 - 1 cells");
        cells_of.push_back(cells_of.back() + n);
    }
}

std::vector<int32_t> weld_local_order(int p, bool hex) {
    std::vector<int32_t> o;
    auto put = [&](int a, int b, int c) { o.push_back(a | (b << 8) | (c << 16)); };
    const int ring[4][2] = {{0, 0}, {p, 0}, {p, p}, {0, p}};
    if (!hex) {   // vtkLagrangeQuadrilateral::PointIndexFromIJK: corners, the edges b = 0, a = p, b = p, a = 0 ascending, the interior with a fastest
        for (auto& r : ring) put(r[0], r[1], 0);
        for (int a = 1; a < p; ++a) put(a, 0, 0);
        for (int b = 1; b < p; ++b) put(p, b, 0);
        for (int a = 1; a < p; ++a) put(a, p, 0);
        for (int b = 1; b < p; ++b) put(0, b, 0);
        for (int b = 1; b < p; ++b)
            for (int a = 1; a < p; ++a) put(a, b, 0);
        return o;
    }
    // vtkLagrangeHexahedron::PointIndexFromIJK (VTK >= 9): corners of c = 0 and c = p, the edges of c = 0 and of c = p in the order of the
    // quadrilateral, the vertical edges at the ring's corners, the faces a = 0, a = p (b fastest), b = 0, b = p, c = 0, c = p (a fastest), the interior
    const int cs[2] = {0, p};
    for (int c : cs)
        for (auto& r : ring) put(r[0], r[1], c);
    for (int c : cs) {
        for (int a = 1; a < p; ++a) put(a, 0, c);
        for (int b = 1; b < p; ++b) put(p, b, c);
        for (int a = 1; a < p; ++a) put(a, p, c);
        for (int b = 1; b < p; ++b) put(0, b, c);
    }
    for (auto& r : ring)
        for (int c = 1; c < p; ++c) put(r[0], r[1], c);
    for (int a : cs)
        for (int c = 1; c < p; ++c)
            for (int b = 1; b < p; ++b) put(a, b, c);
    for (int b : cs)
        for (int c = 1; c < p; ++c)
            for (int a = 1; a < p; ++a) put(a, b, c);
    for (int c : cs)
        for (int b = 1; b < p; ++b)
            for (int a = 1; a < p; ++a) put(a, b, c);
    for (int c = 1; c < p; ++c)
        for (int b = 1; b < p; ++b)
            for (int a = 1; a < p; ++a) put(a, b, c);
    return o;
}

static int find_root(std::vector<int32_t>& parent, int x) {
    int r = x;
    while (parent[r] != r) r = parent[r];
    while (parent[x] != r) {   // path compression
        const int next = parent[x];
        parent[x] = r;
        x = next;
    }
    return r;
}

void weld_map_host(const WeldPlan& pl, int32_t* map, tm_weld_info* info) {
    std::vector<int32_t> parent(static_cast<size_t>(pl.slots));
    for (size_t s = 0; s < parent.size(); ++s) parent[s] = static_cast<int32_t>(s);
    for (const tm_connection& c : pl.conns) {
        if (c.has_periodicity) continue;
        const int64_t len = weld_range_length(c.r[0].start, c.r[0].end);
        for (int64_t t = 0; t < len; ++t) {
            const int a = find_root(parent, pl.slot_of(c.r[0], t)), b = find_root(parent, pl.slot_of(c.r[1], t));
            if (a < b) parent[b] = a;   // the root is the smallest slot, that is, the smallest flat index
            else if (b < a) parent[a] = b;
        }
    }
    std::vector<int32_t> count(parent.size(), 0), id_of(parent.size(), -1);
    for (size_t s = 0; s < parent.size(); ++s) count[find_root(parent, static_cast<int>(s))] += 1;
    tm_weld_info out;
    std::memset(&out, 0, sizeof(out));
    out.nodes_in = static_cast<uint64_t>(pl.nodes);
    out.max_class = 1;
    out.periodic_pairs = static_cast<uint64_t>(pl.periodic_pairs);
    for (size_t s = 0; s < parent.size(); ++s) {
        if (parent[s] != static_cast<int32_t>(s) || count[s] < 2) continue;
        const uint64_t n = static_cast<uint64_t>(count[s]);
        (n == 2 ? out.classes_2 : n == 3 ? out.classes_3 : n == 4 ? out.classes_4 : out.classes_5_up) += 1;
        if (n > out.max_class) out.max_class = n;
    }
    int32_t next = 0;
    for (const WeldBlock& b : pl.blocks)
        for (int j = 0; j < b.nj; ++j)
            for (int i = 0; i < b.ni; ++i) {
                int32_t id;
                if (!weld_on_perimeter(b.ni, b.nj, i, j)) {
                    id = next++;
                } else {
                    const int s = b.slot0 + weld_slot(b.ni, b.nj, i, j), r = parent[s];
                    if (r == s) id_of[s] = next++;
                    id = id_of[r];   // r <= s: numbered already
                }
                if (map) map[b.off + j * b.ni + i] = id;
            }
    out.nodes_out = static_cast<uint64_t>(next);
    if (info) *info = out;
}

double weld_periodic_gap(const WeldPlan& pl, const int32_t* map, int ncomp, uint64_t layers, uint64_t nodes_out, const double* const* out) {
    double gap = 0.0;
    for (const tm_connection& c : pl.conns) {
        if (!c.has_periodicity) continue;
        const int64_t len = weld_range_length(c.r[0].start, c.r[0].end);
        for (uint64_t k = 0; k < layers; ++k)
            for (int64_t t = 0; t < len; ++t) {
                const size_t a = k * nodes_out + map[pl.flat_of(c.r[0], t)], b = k * nodes_out + map[pl.flat_of(c.r[1], t)];
                for (int d = 0; d < 2 && d < ncomp; ++d) {
                    const double g = std::fabs(out[d][a] + c.periodicity[d] - out[d][b]);
                    if (g > gap) gap = g;
                }
            }
    }
    return gap;
}

// info fields that follow from the map alone, for the calls that are handed a map
uint64_t weld_nodes_out(const WeldPlan& pl, const int32_t* map) {
    int32_t top = -1;
    for (int64_t n = 0; n < pl.nodes; ++n) {
        if (map[n] < 0) throw TmError(TM_E_ARG, "map holds a negative id");
        if (map[n] > top) top = map[n];
    }
    return static_cast<uint64_t>(top) + 1;
}

static void points_host(const WeldPlan& pl, const int32_t* map, int ncomp, uint64_t nk, const double* const* planes, double* const* out, tm_weld_info* info) {
    const uint64_t nodes_out = weld_nodes_out(pl, map), layers = static_cast<uint64_t>(weld_layers(nk, nodes_out)), N = static_cast<uint64_t>(pl.nodes);
    const int nb = pl.nblocks();
    std::vector<int32_t> owner(nodes_out, -1);   // first occurrence
    for (uint64_t n = 0; n < N; ++n)
        if (owner[map[n]] < 0) owner[map[n]] = static_cast<int32_t>(n);
    for (int32_t o : owner)
        if (o < 0) throw TmError(TM_E_ARG, "map leaves an id below its maximum unused");
    std::vector<int32_t> block_of(N);
    for (int b = 0; b < nb; ++b)
        for (int64_t l = 0; l < static_cast<int64_t>(pl.blocks[b].ni) * pl.blocks[b].nj; ++l) block_of[pl.blocks[b].off + l] = b;
    auto src = [&](int c, uint64_t k, uint64_t n) {
        const WeldBlock& B = pl.blocks[block_of[n]];
        return planes[static_cast<size_t>(c) * nb + block_of[n]][k * static_cast<uint64_t>(B.ni) * B.nj + (n - B.off)];
    };
    double max_gap = 0.0;
    uint64_t gap_node = 0;
    for (uint64_t k = 0; k < layers; ++k)
        for (uint64_t n = 0; n < N; ++n) {
            const uint64_t o = static_cast<uint64_t>(owner[map[n]]);
            if (o == n) {
                for (int c = 0; c < ncomp; ++c) out[c][k * nodes_out + map[n]] = src(c, k, n);
                continue;
            }
            double g = 0.0;
            for (int c = 0; c < ncomp; ++c) {
                const double d = std::fabs(src(c, k, n) - src(c, k, o));
                if (d > g) g = d;
            }
            if (g > max_gap) {
                max_gap = g;
                gap_node = k * N + n;
            }
        }
    if (info) {
        info->nodes_in = N;
        info->nodes_out = nodes_out;
        info->periodic_pairs = static_cast<uint64_t>(pl.periodic_pairs);
        info->max_gap = max_gap;
        info->gap_node = gap_node;
        info->periodic_gap = weld_periodic_gap(pl, map, ncomp, layers, nodes_out, out);
    }
}

void weld_points_check(const WeldPlan& pl, const int32_t* map, int32_t ncomp, const double* const* planes, double* const* out) {
    if (!map || !planes || !out) throw TmError(TM_E_ARG, "null argument");
    if (ncomp < 1 || ncomp > 3) throw TmError(TM_E_ARG, "ncomp: 1 .. 3 coordinate planes");
    for (int c = 0; c < ncomp; ++c) {
        if (!out[c]) throw TmError(TM_E_ARG, "null output plane");
        for (int b = 0; b < pl.nblocks(); ++b)
            if (!planes[static_cast<size_t>(c) * pl.nblocks() + b]) throw TmError(TM_E_ARG, "null source plane");
    }
}

static void cells_host(const WeldPlan& pl, const std::vector<int64_t>& cells_of, const int32_t* map, int64_t nodes_out, int p, uint64_t nk, int32_t* cells) {
    const bool hex = nk >= 2;
    const std::vector<int32_t> local = weld_local_order(p, hex);
    const int64_t Eg = hex ? static_cast<int64_t>(nk - 1) / p : 1;
    const size_t npe = local.size();
    for (int b = 0; b < pl.nblocks(); ++b) {
        const WeldBlock& B = pl.blocks[b];
        const int Ei = (B.ni - 1) / p, Ej = (B.nj - 1) / p;
        int32_t* out = cells + static_cast<size_t>(cells_of[b]) * npe;
        for (int64_t g = 0; g < Eg; ++g)
            for (int f = 0; f < Ej; ++f)
                for (int e = 0; e < Ei; ++e)
                    for (size_t q = 0; q < npe; ++q) {
                        const int a = local[q] & 255, bb = (local[q] >> 8) & 255, c = local[q] >> 16;
                        *out++ = static_cast<int32_t>((g * p + c) * nodes_out + map[B.off + (f * p + bb) * B.ni + e * p + a]);
                    }
    }
}

}  // namespace tmh

using namespace tmh;

extern "C" int tm_weld_map_host(const tm_mesh_desc* mesh, int32_t* map, tm_weld_info* info) {
    return guarded([&]() {
        const WeldPlan pl = weld_plan(mesh);
        weld_map_host(pl, map, info);
        return TM_OK;
    });
}

extern "C" int tm_weld_points_host(const tm_mesh_desc* mesh, const int32_t* map, int32_t ncomp, uint64_t nk, const double* const* planes, double* const* out,
                                   tm_weld_info* info) {
    return guarded([&]() {
        const WeldPlan pl = weld_plan(mesh);
        weld_points_check(pl, map, ncomp, planes, out);
        points_host(pl, map, ncomp, nk, planes, out, info);
        return TM_OK;
    });
}

extern "C" int tm_weld_cells_host(const tm_mesh_desc* mesh, const int32_t* map, uint64_t nodes_out, int32_t order, uint64_t nk, int32_t* cells) {
    return guarded([&]() {
        weld_layers(nk, nodes_out);   // sizes first: nothing is read when the ids cannot be held
        const WeldPlan pl = weld_plan(mesh);
        std::vector<int64_t> cells_of;
        weld_cells_plan(mesh, pl, order, nk, cells_of);
        if (!map || !cells) throw TmError(TM_E_ARG, "null argument");
        cells_host(pl, cells_of, map, static_cast<int64_t>(nodes_out), order, nk, cells);
        return TM_OK;
    });
}

extern "C" int tm_weld_periodic_pairs(const tm_mesh_desc* mesh, const int32_t* map, int32_t* pairs) {
    return guarded([&]() {
        const WeldPlan pl = weld_plan(mesh);
        if (!map || (!pairs && pl.periodic_pairs)) throw TmError(TM_E_ARG, "null argument");
        for (const tm_connection& c : pl.conns) {
            if (!c.has_periodicity) continue;
            const int64_t len = weld_range_length(c.r[0].start, c.r[0].end);
            for (int64_t t = 0; t < len; ++t) {
                *pairs++ = map[pl.flat_of(c.r[0], t)];
                *pairs++ = map[pl.flat_of(c.r[1], t)];
            }
        }
        return TM_OK;
    });
}
