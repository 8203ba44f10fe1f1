// K19 boundary of the welded mesh.  gfx950, wave64.  Definitions: include/tm_hip.h, "boundary of the welded mesh"; the index arithmetic and the
//     terms are tm_weld_boundary.hpp, shared with the host definition (tm_weld_boundary_host.cpp); the plan (which segment is a face of
//     which patch) is made on the host -- the perimeter is small.
//
// 1. k_weld_faces_lateral expands the host's segment table over span elements and local nodes: one id per lane, consecutive lanes on
//    consecutive ids of consecutive faces (the segments of a patch are consecutive faces).  Perimeter-sized; in a plane mesh it is all there is.
// 2. k_weld_faces_caps covers all plane elements of a block twice -- hub and shroud -- with k_weld_cells' store pattern: a workgroup takes
//    2048 / npf whole elements.  This is the launch with weight.
// 3. k_weld_faces_measure gathers the points of WB_TILE faces per workgroup through their ids, forms the terms of tm_weld_boundary.hpp and
//    reduces wave -> workgroup into one partial per (workgroup, patch).  Faces are patch-major, so a workgroup meets the patches of one
//    short run, which the host lists for it (part_begin / part_patch): nothing is sorted and no atomic is used.  k_weld_faces_final sums
//    the partials of a patch -- consecutive, since both orders ascend -- per lane in strides and then by a fixed tree: the result does not
//    depend on scheduling.
#include "tm_weld_boundary_dev.hpp"
#include "tm_stack_dev.hpp"
#include "tm_devutil.hpp"

#include <algorithm>
#include <cstring>

namespace tmh {

constexpr int WB_THREADS = 256, WB_WAVES = WB_THREADS / 64;
constexpr int WB_IDS = 2048;                                             // ids per workgroup of the caps pass
constexpr int WB_PER_THREAD = 4, WB_TILE = WB_THREADS * WB_PER_THREAD;   // faces per workgroup of the measure

// ------------------------------------------------------------------ 1. lateral faces
// local: a | c << 8 per local node (c = 0 in a plane mesh); total = nseg * Eg * npf ids
__global__ __launch_bounds__(WB_THREADS) void k_weld_faces_lateral(const WeldBlock* __restrict__ blocks, const int32_t* __restrict__ orientation,
                                                                   const WbSeg* __restrict__ segs, int nseg, long long total, int p, int npf,
                                                                   const int32_t* __restrict__ local, const int32_t* __restrict__ map, int nodes_out,
                                                                   int32_t* __restrict__ out) {
    __shared__ int32_t sh_local[WB_MAX_NPF];
    if (static_cast<int>(threadIdx.x) < npf) sh_local[threadIdx.x] = local[threadIdx.x];
    __syncthreads();
    const long long idx = static_cast<long long>(blockIdx.x) * WB_THREADS + threadIdx.x;
    if (idx >= total) return;
    const long long r = idx / npf;
    const int q = static_cast<int>(idx - r * npf), g = static_cast<int>(r / nseg), k = static_cast<int>(r - static_cast<long long>(g) * nseg);
    const WbSeg s = segs[k];
    const WeldBlock B = blocks[s.block];
    const int l = sh_local[q], a = l & 255, c = l >> 8;
    const long long face = s.face0 + static_cast<long long>(g) * s.stride;   // < faces <= 2^31 - 1 (weld_boundary_plan)
    out[face * npf + q] = (g * p + c) * nodes_out + map[B.off + wb_seg_node(B, s.side, p, s.e, a, orientation[s.block])];   // fits: weld_layers
}

// ------------------------------------------------------------------ 2. caps
// one block: a workgroup takes per_wg whole plane elements (per_wg * npf <= WB_IDS); hub / shroud: the block's first id in either patch
__global__ __launch_bounds__(WB_THREADS) void k_weld_faces_caps(const int32_t* __restrict__ map, WeldBlock B, int orientation, int p, int Ei, int ncells, int npf,
                                                                int per_wg, const int32_t* __restrict__ local, int top, int32_t* __restrict__ hub,
                                                                int32_t* __restrict__ shroud) {
    __shared__ int32_t sh_local[WB_MAX_NPF];
    if (static_cast<int>(threadIdx.x) < npf) sh_local[threadIdx.x] = local[threadIdx.x];
    __syncthreads();
    const int el0 = static_cast<int>(blockIdx.x) * per_wg;
    const int here = ncells - el0 < per_wg ? ncells - el0 : per_wg;   // >= 1 by the grid
    const size_t base = static_cast<size_t>(el0) * npf;
    for (int idx = threadIdx.x; idx < here * npf; idx += WB_THREADS) {
        const int k = idx / npf, q = idx - k * npf, el = el0 + k;
        const int f = el / Ei, e = el - f * Ei;
        const int l = sh_local[q], a = l & 255, b = l >> 8;
        hub[base + idx] = map[B.off + wb_cap_node(B, false, p, e, f, a, b, orientation)];
        shroud[base + idx] = top + map[B.off + wb_cap_node(B, true, p, e, f, a, b, orientation)];   // <= nk * nodes_out - 1: fits (weld_layers)
    }
}

// ------------------------------------------------------------------ 3. measures
__device__ __forceinline__ void wb_face_terms(int dim, int p, int npf, const int32_t* __restrict__ ids, const int32_t* inv, const double* __restrict__ px,
                                              const double* __restrict__ py, const double* __restrict__ pz, double* acc) {
    double t[WB_TERMS];
#pragma unroll
    for (int k = 0; k < WB_TERMS; ++k) acc[k] = 0.0;
    if (dim == 2) {
        for (int a = 0; a < p; ++a) {
            const int A = ids[wb_curve_local(p, a)], B = ids[wb_curve_local(p, a + 1)];
            wb_edge_terms(px[A], py[A], px[B], py[B], t);
#pragma unroll
            for (int k = 0; k < WB_TERMS; ++k) acc[k] += t[k];
        }
        return;
    }
    const int n1 = p + 1;
    for (int c = 0; c < p; ++c)
        for (int a = 0; a < p; ++a) {
            int corner[4];
            if (p == 1) {   // the ring itself: one 16-byte load
                const int4 v = *reinterpret_cast<const int4*>(ids);
                corner[0] = v.x;
                corner[1] = v.y;
                corner[2] = v.z;
                corner[3] = v.w;
            } else {
                corner[0] = ids[inv[c * n1 + a]];
                corner[1] = ids[inv[c * n1 + a + 1]];
                corner[2] = ids[inv[(c + 1) * n1 + a + 1]];
                corner[3] = ids[inv[(c + 1) * n1 + a]];
            }
            double P[4][3];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                P[k][0] = px[corner[k]];
                P[k][1] = py[corner[k]];
                P[k][2] = pz[corner[k]];
            }
            wb_quad_terms(P[0], P[1], P[2], P[3], t);
#pragma unroll
            for (int k = 0; k < WB_TERMS; ++k) acc[k] += t[k];
        }
}

// sum over the workgroup in a fixed order: shuffle tree inside the wave, then waves 0 .. 3 in order on lane 0 of wave 0
__device__ __forceinline__ double wb_block_sum(double v, double* sh) {   // sh[WB_WAVES]
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double total = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < WB_WAVES; ++w) total += sh[w];
    }
    __syncthreads();
    return total;
}

// ids were checked against npoints and face_patch against the partial table on the host before the launch (weld_measure_check)
__global__ __launch_bounds__(WB_THREADS) void k_weld_faces_measure(int dim, int p, int npf, int nfaces, const int32_t* __restrict__ faces,
                                                                   const int32_t* __restrict__ face_patch, const int32_t* __restrict__ inv,
                                                                   const double* __restrict__ px, const double* __restrict__ py, const double* __restrict__ pz,
                                                                   const int32_t* __restrict__ part_begin, const int32_t* __restrict__ part_patch,
                                                                   double* __restrict__ partials) {
    __shared__ int32_t sh_inv[WB_MAX_NPF];
    __shared__ double sh_sum[WB_WAVES];
    if (dim == 3 && static_cast<int>(threadIdx.x) < npf) sh_inv[threadIdx.x] = inv[threadIdx.x];
    __syncthreads();
    double t[WB_PER_THREAD][WB_TERMS];
    int pf[WB_PER_THREAD];
#pragma unroll
    for (int r = 0; r < WB_PER_THREAD; ++r) {
        const long long f = static_cast<long long>(blockIdx.x) * WB_TILE + r * WB_THREADS + threadIdx.x;
        pf[r] = -1;
        if (f < nfaces) {
            pf[r] = face_patch[f];
            wb_face_terms(dim, p, npf, faces + f * npf, sh_inv, px, py, pz, t[r]);
        }
    }
    for (int k = part_begin[blockIdx.x]; k < part_begin[blockIdx.x + 1]; ++k) {   // the same for every lane of the workgroup
        const int q = part_patch[k];
#pragma unroll
        for (int j = 0; j < WB_TERMS; ++j) {
            double v = 0.0;
#pragma unroll
            for (int r = 0; r < WB_PER_THREAD; ++r)
                if (pf[r] == q) v += t[r][j];
            const double total = wb_block_sum(v, sh_sum);
            if (threadIdx.x == 0) partials[static_cast<size_t>(k) * WB_TERMS + j] = total;
        }
    }
}

// grid.x = patch: its partials [patch_part[q], patch_part[q+1]) per lane in strides of the workgroup, then the fixed tree
__global__ __launch_bounds__(WB_THREADS) void k_weld_faces_final(const int32_t* __restrict__ patch_part, const double* __restrict__ partials, double* __restrict__ sums) {
    __shared__ double sh_sum[WB_WAVES];
    const int q = blockIdx.x, k0 = patch_part[q], k1 = patch_part[q + 1];
    for (int j = 0; j < WB_TERMS; ++j) {
        double v = 0.0;
        for (int k = k0 + static_cast<int>(threadIdx.x); k < k1; k += WB_THREADS) v += partials[static_cast<size_t>(k) * WB_TERMS + j];
        const double total = wb_block_sum(v, sh_sum);
        if (threadIdx.x == 0) sums[static_cast<size_t>(q) * WB_TERMS + j] = total;
    }
}

// ------------------------------------------------------------------ host driver
namespace {

unsigned groups(int64_t n, int per) { return static_cast<unsigned>((n + per - 1) / per); }

std::vector<int32_t> face_local_table(const WeldBoundaryPlan& bp) {   // a | c << 8 per local node
    if (bp.layered) return weld_local_order(bp.p, false);
    std::vector<int32_t> t(static_cast<size_t>(bp.p) + 1);
    for (int a = 0; a <= bp.p; ++a) t[wb_curve_local(bp.p, a)] = a;
    return t;
}

// the face ids of a plan on the device (asynchronous on st); d_map: the welded map on the device; d_faces: bp.faces * bp.npf ids
void faces_run(const WeldPlan& pl, const WeldBoundaryPlan& bp, hipStream_t st, const int32_t* d_map, int64_t nodes_out, uint64_t nk, const int32_t* orientation,
               int32_t* d_faces, FaceTables& keep) {
    const int nb = pl.nblocks(), p = bp.p, npf = bp.npf;
    std::vector<int32_t>& orient = keep.h_orient;
    orient.resize(nb);
    for (int b = 0; b < nb; ++b) orient[b] = orientation && orientation[b] < 0 ? -1 : 1;
    keep.h_local = face_local_table(bp);
    const std::vector<int32_t>& local = keep.h_local;
    const WeldBlock* d_blocks = keep.blocks.upload(pl.blocks.data(), pl.blocks.size(), st, "boundary block table");
    const int32_t* d_orient = keep.orient.upload(orient.data(), orient.size(), st, "boundary orientations");
    const WbSeg* d_segs = keep.segs.upload(bp.segs.data(), bp.segs.size(), st, "boundary segment table");
    const int32_t* d_local = keep.local.upload(local.data(), local.size(), st, "boundary local order");
    const int nseg = static_cast<int>(bp.segs.size());
    const long long total = static_cast<long long>(nseg) * bp.Eg * npf;
    if (total > 0) {
        if (groups(total, WB_THREADS) > 2147483647u) throw TmError(TM_E_ARG, "too many lateral faces for one launch");
        hipLaunchKernelGGL(k_weld_faces_lateral, dim3(groups(total, WB_THREADS)), dim3(WB_THREADS), 0, st, d_blocks, d_orient, d_segs, nseg, total, p, npf, d_local, d_map,
                           static_cast<int>(nodes_out), d_faces);
        HIPCHK(hipGetLastError());
    }
    if (!bp.layered) return;
    const int per_wg = WB_IDS / npf, top = static_cast<int>(static_cast<int64_t>(nk - 1) * nodes_out);
    for (int b = 0; b < nb; ++b) {
        const WeldBlock& B = pl.blocks[b];
        const int ncells = static_cast<int>(bp.cells_of[b + 1] - bp.cells_of[b]);
        if (ncells == 0) continue;
        hipLaunchKernelGGL(k_weld_faces_caps, dim3(groups(ncells, per_wg)), dim3(WB_THREADS), 0, st, d_map, B, orient[b], p, (B.ni - 1) / p, ncells, npf, per_wg, d_local,
                           top, d_faces + static_cast<size_t>(bp.hub_begin + bp.cells_of[b]) * npf, d_faces + static_cast<size_t>(bp.shroud_begin + bp.cells_of[b]) * npf);
        HIPCHK(hipGetLastError());
    }
}

// the measures of device faces over device planes into patches (synchronises); face_patch: host, checked already
void measure_run(hipStream_t st, int dim, int p, int npf, int64_t nfaces, const int32_t* d_faces, const int32_t* face_patch, int64_t npatches, const double* px,
                 const double* py, const double* pz, tm_weld_patch* patches) {
    // the partial table: per workgroup the patches of its tile (a run of the non-decreasing face_patch), per patch its partials
    const int nwg = static_cast<int>(groups(nfaces, WB_TILE));
    std::vector<int32_t> part_begin(static_cast<size_t>(nwg) + 1, 0), part_patch, patch_part(static_cast<size_t>(npatches) + 1, 0);
    for (int w = 0; w < nwg; ++w) {
        const int64_t f1 = std::min<int64_t>(nfaces, static_cast<int64_t>(w + 1) * WB_TILE);
        int32_t last = -1;
        for (int64_t f = static_cast<int64_t>(w) * WB_TILE; f < f1; ++f)
            if (face_patch[f] != last) {
                last = face_patch[f];
                part_patch.push_back(last);
                patch_part[static_cast<size_t>(last) + 1] += 1;
            }
        part_begin[static_cast<size_t>(w) + 1] = static_cast<int32_t>(part_patch.size());
    }
    for (int64_t q = 0; q < npatches; ++q) patch_part[static_cast<size_t>(q) + 1] += patch_part[static_cast<size_t>(q)];
    std::vector<double> sums(static_cast<size_t>(npatches) * WB_TERMS, 0.0);
    if (nfaces > 0) {
        const std::vector<int32_t> inv = dim == 3 ? weld_quad_inverse(p) : std::vector<int32_t>(1, 0);
        DevBuf b_fp, b_inv, b_pb, b_pp, b_qp, b_part, b_sums;
        const int32_t* d_fp = b_fp.upload(face_patch, static_cast<size_t>(nfaces), st, "face patches");
        const int32_t* d_inv = b_inv.upload(inv.data(), inv.size(), st, "face local order");
        const int32_t* d_pb = b_pb.upload(part_begin.data(), part_begin.size(), st, "partial table");
        const int32_t* d_pp = b_pp.upload(part_patch.data(), part_patch.size(), st, "partial table");
        const int32_t* d_qp = b_qp.upload(patch_part.data(), patch_part.size(), st, "partial table");
        b_part.grow(sizeof(double) * part_patch.size() * WB_TERMS, "boundary partials");
        b_sums.grow(sizeof(double) * sums.size(), "boundary sums");
        double* d_part = b_part.as<double>();
        double* d_sums = b_sums.as<double>();
        hipLaunchKernelGGL(k_weld_faces_measure, dim3(nwg), dim3(WB_THREADS), 0, st, dim, p, npf, static_cast<int>(nfaces), d_faces, d_fp, d_inv, px, py, pz, d_pb, d_pp,
                           d_part);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_weld_faces_final, dim3(static_cast<unsigned>(npatches)), dim3(WB_THREADS), 0, st, d_qp, d_part, d_sums);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(sums.data(), d_sums, sizeof(double) * sums.size(), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));   // the buffers go out of scope behind it
    }
    for (int64_t q = 0; q < npatches; ++q) {
        const double* s = sums.data() + static_cast<size_t>(q) * WB_TERMS;
        patches[q].measure = s[0];
        patches[q].normal[0] = s[1];
        patches[q].normal[1] = s[2];
        patches[q].normal[2] = s[3];
        patches[q].moment = s[4];
    }
}

}  // namespace

void weld_faces_run(const WeldPlan& pl, const WeldBoundaryPlan& bp, hipStream_t st, const int32_t* d_map, int64_t nodes_out, uint64_t nk, const int32_t* orientation,
                    int32_t* d_faces, FaceTables& keep) {
    faces_run(pl, bp, st, d_map, nodes_out, nk, orientation, d_faces, keep);
}

// ------------------------------------------------------------------ handle: the coordinates resident in X
void Smoother::weld_boundary_host(int order, const int32_t* block_orientation, int32_t* faces, int32_t* face_patch, tm_weld_patch* patches) {
    if (lp.nranks > 1) throw TmError(TM_E_UNSUPPORTED, "welding needs every block in one handle: not served with rank hooks");
    std::vector<tm_block> tb;
    std::vector<tm_connection> tc;
    std::vector<tm_condition> tq;
    std::vector<const double2*> blocks_x;
    weld_tables(tb, tc, tq, blocks_x);
    tm_mesh_desc desc{tb.data(), tb.size(), tc.data(), tc.size(), tq.data(), tq.size()};
    const WeldPlan pl = weld_plan(&desc);
    const WeldBoundaryPlan bp = weld_boundary_plan(&desc, pl, order, 0);
    std::vector<int32_t> orient(static_cast<size_t>(pl.nblocks()), 1);
    if (block_orientation) {
        orient.assign(block_orientation, block_orientation + pl.nblocks());
    } else {   // the rule of tm_smoother_quality
        std::vector<tm_quality> per(static_cast<size_t>(pl.nblocks()));
        quality_host(per.data(), nullptr);
        for (int b = 0; b < pl.nblocks(); ++b) orient[b] = per[b].orientation;
    }
    if (!welddev) welddev = new WeldDev();
    tm_weld_info rec;
    welddev->link(pl, stream);
    welddev->number(pl, stream);
    welddev->read_map(pl, stream, nullptr, &rec);
    const int64_t nodes_out = static_cast<int64_t>(rec.nodes_out);
    WeldGap gap{0.0, 0ull};
    welddev->points_resident(pl, stream, blocks_x, nodes_out, nullptr, nullptr, &gap);   // the welded planes stay in welddev->out
    FaceTables keep;
    const size_t nids = static_cast<size_t>(bp.faces) * bp.npf;
    DevBuf b_faces(sizeof(int32_t) * nids, "boundary faces");
    int32_t* d_faces = b_faces.as<int32_t>();
    faces_run(pl, bp, stream, static_cast<const int32_t*>(welddev->map.p), nodes_out, 0, orient.data(), d_faces, keep);
    if (faces && nids) HIPCHK(hipMemcpyAsync(faces, d_faces, sizeof(int32_t) * nids, hipMemcpyDeviceToHost, stream));
    std::vector<int32_t> own_patch;
    if (!face_patch) {
        own_patch.resize(static_cast<size_t>(bp.faces));
        face_patch = own_patch.data();
    }
    weld_boundary_labels(pl, bp, face_patch, nullptr);
    std::memcpy(patches, bp.patches.data(), sizeof(tm_weld_patch) * bp.patches.size());
    const double* ox = static_cast<const double*>(welddev->out.p);
    measure_run(stream, 2, bp.p, bp.npf, bp.faces, d_faces, face_patch, static_cast<int64_t>(bp.patches.size()), ox, ox + nodes_out, nullptr, patches);
    HIPCHK(hipStreamSynchronize(stream));
}

}  // namespace tmh

using namespace tmh;

extern "C" int tm_weld_boundary_faces(const tm_mesh_desc* mesh, const int32_t* map, uint64_t nodes_out, int32_t order, uint64_t nk,
                                      const int32_t* block_orientation, int32_t* faces, int32_t* face_patch, int32_t* origin) {
    return guarded([&]() {
        weld_layers(nk, nodes_out);   // sizes first: nothing is read when the ids cannot be held
        const WeldPlan pl = weld_plan(mesh);
        const WeldBoundaryPlan bp = weld_boundary_plan(mesh, pl, order, nk);
        if (!map || (!faces && bp.faces)) throw TmError(TM_E_ARG, "null argument");
        for (int64_t n = 0; n < pl.nodes; ++n)   // the kernels add layer offsets to these ids
            if (map[n] < 0 || static_cast<uint64_t>(map[n]) >= nodes_out) throw TmError(TM_E_ARG, "map holds an id outside 0 .. nodes_out - 1");
        require_gfx950();
        FaceTables keep;
        DevBuf b_map;
        const int32_t* d_map = b_map.upload(map, static_cast<size_t>(pl.nodes), nullptr, "weld map");
        const size_t nids = static_cast<size_t>(bp.faces) * bp.npf;
        DevBuf b_faces(sizeof(int32_t) * nids, "boundary faces");
        int32_t* d_faces = b_faces.as<int32_t>();
        faces_run(pl, bp, nullptr, d_map, static_cast<int64_t>(nodes_out), nk, block_orientation, d_faces, keep);
        if (nids) HIPCHK(hipMemcpyAsync(faces, d_faces, sizeof(int32_t) * nids, hipMemcpyDeviceToHost, nullptr));
        HIPCHK(hipStreamSynchronize(nullptr));
        weld_boundary_labels(pl, bp, face_patch, origin);
        return TM_OK;
    });
}

extern "C" int tm_weld_faces_measure(int32_t dim, int32_t order, uint64_t nfaces, const int32_t* faces, const int32_t* face_patch, uint64_t npatches,
                                     uint64_t npoints, int32_t ncomp, const double* const* points, tm_weld_patch* patches) {
    return guarded([&]() {
        const int npf = weld_measure_check(dim, order, nfaces, faces, face_patch, npatches, npoints, ncomp, points, patches);
        require_gfx950();
        DevBuf b_faces, b_pts(sizeof(double) * npoints * dim, "welded planes");
        const int32_t* d_faces = b_faces.upload(faces, static_cast<size_t>(nfaces) * npf, nullptr, "boundary faces");
        double* d_pts = b_pts.as<double>();
        for (int c = 0; c < dim; ++c)
            if (npoints) HIPCHK(hipMemcpyAsync(d_pts + static_cast<size_t>(c) * npoints, points[c], sizeof(double) * npoints, hipMemcpyHostToDevice, nullptr));
        measure_run(nullptr, dim, order, npf, static_cast<int64_t>(nfaces), d_faces, face_patch, static_cast<int64_t>(npatches), d_pts, d_pts + npoints,
                    dim == 3 ? d_pts + 2 * npoints : nullptr, patches);
        HIPCHK(hipStreamSynchronize(nullptr));
        return TM_OK;
    });
}

extern "C" int tm_smoother_weld_boundary(tm_smoother* s, int32_t order, const int32_t* block_orientation, int32_t* faces, int32_t* face_patch,
                                         tm_weld_patch* patches) {
    return guarded([&]() {
        if (!s || !smoother_is_live(s)) throw TmError(TM_E_ARG, "not a live handle");
        if (!patches) throw TmError(TM_E_ARG, "patches are needed");
        s->impl.weld_boundary_host(order, block_orientation, faces, face_patch, patches);
        return TM_OK;
    });
}
