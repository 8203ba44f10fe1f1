// K21 faces, owners and finite-volume metrics of the welded mesh.  gfx950, wave64.  Definitions: include/tm_hip.h, "faces of the welded
//     mesh"; the index arithmetic and every expression of the metrics are tm_fv.hpp, shared with the host definition (tm_fv_host.cpp); the
//     table of the block-side segments is made on the host -- the perimeter is small.
//
// 1. Face lists.  k_fv_count takes a cell per thread, forms its 4 (6) neighbours in closed form plus the segment table and counts those
//    above itself; WeldDev::exscan (K18's tile sums / scan / scan inside the tiles) turns the counts into the first face of every cell;
//    k_fv_interior forms the neighbours again, sorts the owned ones with the fixed network of tm_fv.hpp and writes owner, neighbour, the
//    ring and both cell_faces slots of the face: every address is written by exactly one thread, no atomics.  K19's kernels write the
//    boundary ids behind the interior faces; k_fv_boundary adds their owners and cell_faces slots from `origin`.
// 2. Metrics.  k_fv_cells: a cell per thread gathers its faces through cell_faces and their points through the ids, writes the centre
//    (and the optional fields) and accumulates the record; k_fv_faces: a face per thread reads the two centres.  Both walk tiles with a
//    grid stride, reduce thread -> workgroup through LDS in a fixed tree and leave one record per workgroup; k_fv_final combines them with
//    records_reduce_wave.  No floating-point atomics: the same bits from run to run.
#include "tm_fv.hpp"
#include "tm_weld_boundary_dev.hpp"
#include "tm_records.hpp"
#include "tm_stack.hpp"
#include "tm_api_util.hpp"

#include <algorithm>
#include <cstring>

namespace tmh {

constexpr int FV_THREADS = 256;
constexpr int FV_MAX_GRID = 512;   // workgroups of a metrics pass: each leaves one record

// ------------------------------------------------------------------ 1. face lists
__global__ __launch_bounds__(FV_THREADS) void k_fv_count(const FvBlock* __restrict__ blocks, int nblocks, const FvSeg* __restrict__ segs, int ncells, int Eg, int fpc,
                                                         int32_t* __restrict__ counts) {
    const long long cell = static_cast<long long>(blockIdx.x) * FV_THREADS + threadIdx.x;
    if (cell >= ncells) return;
    int b, e, f, g, n = 0;
    fv_cell_place(blocks, nblocks, static_cast<int>(cell), b, e, f, g);
    for (int s = 0; s < fpc; ++s) {
        int back;
        if (fv_neighbour(blocks, segs, b, e, f, g, Eg, s, back) > cell) ++n;
    }
    counts[cell] = n;
}

// first[cell]: the exclusive prefix of the counts.  A face index at or past ninternal (a plan and a table that disagree) is not written;
// the driver compares the total with the plan afterwards.
__global__ __launch_bounds__(FV_THREADS) void k_fv_interior(const FvBlock* __restrict__ blocks, int nblocks, const FvSeg* __restrict__ segs, int ncells, int Eg, int fpc,
                                                            int layered, const int32_t* __restrict__ map, int nodes_out, const int32_t* __restrict__ first,
                                                            int ninternal, int32_t* __restrict__ faces, int32_t* __restrict__ owner,
                                                            int32_t* __restrict__ neighbour, int32_t* __restrict__ cell_faces) {
    const long long cell = static_cast<long long>(blockIdx.x) * FV_THREADS + threadIdx.x;
    if (cell >= ncells) return;
    int b, e, f, g, nbr[6], sd[6], bk[6];
    fv_cell_place(blocks, nblocks, static_cast<int>(cell), b, e, f, g);
    const int n = fv_owned(blocks, segs, b, e, f, g, Eg, fpc, static_cast<int>(cell), nbr, sd, bk);
    const FvBlock B = blocks[b];
    const int npf = layered ? 4 : 2;
    const long long at = first[cell];
    for (int k = 0; k < n; ++k) {
        const long long face = at + k;
        if (face < 0 || face >= ninternal || nbr[k] >= ncells) return;
        int32_t ids[4];
        fv_cell_face(B, e, f, g, sd[k], layered != 0, map, nodes_out, ids);
        for (int q = 0; q < npf; ++q) faces[face * npf + q] = ids[q];
        owner[face] = static_cast<int32_t>(cell);
        neighbour[face] = nbr[k];
        cell_faces[cell * fpc + sd[k]] = static_cast<int32_t>(face);
        cell_faces[static_cast<long long>(nbr[k]) * fpc + bk[k]] = static_cast<int32_t>(face);
    }
}

__global__ __launch_bounds__(FV_THREADS) void k_fv_boundary(const FvBlock* __restrict__ blocks, const int32_t* __restrict__ origin, int nboundary, int ninternal, int ncells,
                                                            int Eg, int fpc, int32_t* __restrict__ owner, int32_t* __restrict__ cell_faces) {
    const long long t = static_cast<long long>(blockIdx.x) * FV_THREADS + threadIdx.x;
    if (t >= nboundary) return;
    const int cell = fv_origin_cell(blocks, origin + 4 * t, Eg), side = origin[4 * t + 1];
    if (cell < 0 || cell >= ncells || side < 0 || side >= fpc) return;   // origin is the host's own table: never taken
    owner[ninternal + t] = cell;
    cell_faces[static_cast<long long>(cell) * fpc + side] = static_cast<int32_t>(ninternal + t);
}

// ------------------------------------------------------------------ 2. metrics
struct FvDev {   // the lists and the welded planes on the device, checked on the host or made by stage 1
    int dim, npf, fpc;
    long long ncells, ninternal, nboundary;
    const int32_t *faces, *owner, *neighbour, *cell_faces;
    const double *px, *py, *pz;
};
struct FvOut {   // optional fields on the device, any may be null
    double *volume, *centre, *closedness, *area, *face_centre, *cos, *skewness;
};

// DIM is a template parameter of the metrics kernels: the loops over faces, nodes and components unroll and the small arrays stay in registers
template <int DIM>
__device__ __forceinline__ void fv_dev_face_points(const FvDev& L, long long face, double P[4][3]) {
    constexpr int NPF = DIM == 2 ? 2 : 4;
    int id[NPF];
    if constexpr (DIM == 2) {
        const int2 v = *reinterpret_cast<const int2*>(L.faces + face * 2);   // 8-byte aligned: hipMalloc'ed base, even offset
        id[0] = v.x, id[1] = v.y;
    } else {
        const int4 v = *reinterpret_cast<const int4*>(L.faces + face * 4);
        id[0] = v.x, id[1] = v.y, id[2] = v.z, id[3] = v.w;
    }
#pragma unroll
    for (int q = 0; q < NPF; ++q) {
        P[q][0] = L.px[id[q]];
        P[q][1] = L.py[id[q]];
        P[q][2] = DIM == 3 ? L.pz[id[q]] : 0.0;
    }
}

// thread -> workgroup in a fixed tree through LDS; sh[FV_THREADS]
__device__ __forceinline__ void fv_block_reduce(const FvAcc& a, FvAcc* sh, FvAcc* out) {
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int off = FV_THREADS / 2; off > 0; off >>= 1) {
        if (static_cast<int>(threadIdx.x) < off) fv_acc_combine(sh[threadIdx.x], sh[threadIdx.x + off]);
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = sh[0];
}

// centre: 3 doubles per cell (the face pass reads them)
template <int DIM>
__global__ __launch_bounds__(FV_THREADS) void k_fv_cells(FvDev L, FvOut out, double* __restrict__ centre, FvAcc* __restrict__ partials) {
    constexpr int FPC = 2 * DIM;
    __shared__ FvAcc sh[FV_THREADS];
    FvAcc acc;
    fv_acc_init(acc);
    for (long long cell = static_cast<long long>(blockIdx.x) * FV_THREADS + threadIdx.x; cell < L.ncells; cell += static_cast<long long>(gridDim.x) * FV_THREADS) {
        double P[4][3], S[6][3], Cf[6][3], sign[6];
#pragma unroll
        for (int k = 0; k < FPC; ++k) {
            const int face = L.cell_faces[cell * FPC + k];
            fv_dev_face_points<DIM>(L, face, P);
            fv_face_geometry(DIM, P, S[k], Cf[k]);
            sign[k] = L.owner[face] == cell ? 1.0 : -1.0;
        }
        const FvCell m = fv_cell_metrics(DIM, FPC, S, Cf, sign);
        for (int c = 0; c < 3; ++c) centre[cell * 3 + c] = m.centre[c];
        fv_acc_cell(acc, cell, m);
        if (out.volume) out.volume[cell] = m.volume;
        if (out.closedness) out.closedness[cell] = m.closedness;
        if (out.centre)
            for (int c = 0; c < DIM; ++c) out.centre[c * L.ncells + cell] = m.centre[c];
    }
    fv_block_reduce(acc, sh, partials + blockIdx.x);
}

template <int DIM>
__global__ __launch_bounds__(FV_THREADS) void k_fv_faces(FvDev L, FvOut out, const double* __restrict__ centre, FvAcc* __restrict__ partials) {
    __shared__ FvAcc sh[FV_THREADS];
    FvAcc acc;
    fv_acc_init(acc);
    const long long nfaces = L.ninternal + L.nboundary;
    for (long long face = static_cast<long long>(blockIdx.x) * FV_THREADS + threadIdx.x; face < nfaces; face += static_cast<long long>(gridDim.x) * FV_THREADS) {
        double P[4][3], s[3], cf[3], d[3], Cown[3], Cnb[3];
        fv_dev_face_points<DIM>(L, face, P);
        fv_face_geometry(DIM, P, s, cf);
        const bool interior = face < L.ninternal;
        const long long o = L.owner[face], n = interior ? L.neighbour[face] : 0;
        for (int c = 0; c < 3; ++c) {
            Cown[c] = centre[o * 3 + c];
            Cnb[c] = interior ? centre[n * 3 + c] : cf[c];
            d[c] = Cnb[c] - Cown[c];
        }
        const double cosine = fv_cos(d, s), skew = interior ? fv_skewness(Cown, Cnb, cf, s) : 0.0;
        fv_acc_face(acc, face, interior, cosine, skew);
        if (out.cos) out.cos[face] = cosine;
        if (out.skewness && interior) out.skewness[face] = skew;
        for (int c = 0; c < DIM; ++c) {
            if (out.area) out.area[c * nfaces + face] = s[c];
            if (out.face_centre) out.face_centre[c * nfaces + face] = cf[c];
        }
    }
    fv_block_reduce(acc, sh, partials + blockIdx.x);
}

__global__ __launch_bounds__(64) void k_fv_final(const FvAcc* __restrict__ partials, int n, FvAcc* __restrict__ out) {
    __shared__ FvAcc sh[64];
    records_reduce_wave<FvAcc, fv_acc_init, fv_acc_combine>(partials, 0, n, sh);
    if (threadIdx.x == 0) out[0] = sh[0];
}

// ------------------------------------------------------------------ host driver
namespace {

unsigned groups(int64_t n, int per) { return static_cast<unsigned>(std::max<int64_t>(1, (n + per - 1) / per)); }

// the lists of a plan on the device
struct FvListBufs {
    DevBuf blocks, segs, origin, counts, first, faces, owner, neighbour, cell_faces;
    FaceTables keep;
    std::vector<int32_t> h_origin;
};

// stage 1 (synchronises once to compare the number of owned faces with the plan); d_map: the welded map on the device
void faces_run(const WeldPlan& pl, const WeldBoundaryPlan& bp, const FvPlan& fp, hipStream_t st, WeldDev& wd, const int32_t* d_map, int64_t nodes_out, uint64_t nk,
               const int32_t* orientation, FvListBufs& B) {
    const int ncells = static_cast<int>(fp.cells), ninternal = static_cast<int>(fp.internal), nboundary = static_cast<int>(fp.boundary), nb = static_cast<int>(fp.blocks.size());
    const size_t nfaces = static_cast<size_t>(fp.internal + fp.boundary);
    const FvBlock* d_blocks = B.blocks.upload(fp.blocks.data(), fp.blocks.size(), st, "face block table");
    const FvSeg* d_segs = B.segs.upload(fp.segs.data(), fp.segs.size(), st, "face segment table");
    B.counts.grow(sizeof(int32_t) * fp.cells, "owned faces per cell");
    B.first.grow(sizeof(int32_t) * fp.cells, "first face per cell");
    B.faces.grow(sizeof(int32_t) * nfaces * fp.npf, "faces");
    B.owner.grow(sizeof(int32_t) * nfaces, "face owners");
    B.neighbour.grow(sizeof(int32_t) * static_cast<size_t>(fp.internal), "face neighbours");
    B.cell_faces.grow(sizeof(int32_t) * static_cast<size_t>(fp.cells) * fp.fpc, "faces of the cells");
    const dim3 wg(FV_THREADS), over_cells(groups(ncells, FV_THREADS));
    hipLaunchKernelGGL(k_fv_count, over_cells, wg, 0, st, d_blocks, nb, d_segs, ncells, fp.Eg, fp.fpc, B.counts.as<int32_t>());
    HIPCHK(hipGetLastError());
    wd.exscan(st, B.counts.as<int32_t>(), ncells, B.first.as<int32_t>());
    int32_t last[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(&last[0], B.first.as<int32_t>() + (ncells - 1), sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&last[1], B.counts.as<int32_t>() + (ncells - 1), sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (static_cast<int64_t>(last[0]) + last[1] != fp.internal) throw TmError(TM_E_MISMATCH, "the connections do not yield the interior faces of the plan");
    hipLaunchKernelGGL(k_fv_interior, over_cells, wg, 0, st, d_blocks, nb, d_segs, ncells, fp.Eg, fp.fpc, fp.layered ? 1 : 0, d_map, static_cast<int>(nodes_out),
                       static_cast<const int32_t*>(B.first.as<int32_t>()), ninternal, B.faces.as<int32_t>(), B.owner.as<int32_t>(), B.neighbour.as<int32_t>(),
                       B.cell_faces.as<int32_t>());
    HIPCHK(hipGetLastError());
    if (nboundary) {
        weld_faces_run(pl, bp, st, d_map, nodes_out, nk, orientation, B.faces.as<int32_t>() + static_cast<size_t>(fp.internal) * fp.npf, B.keep);
        B.h_origin.resize(static_cast<size_t>(nboundary) * 4);
        weld_boundary_labels(pl, bp, nullptr, B.h_origin.data());
        const int32_t* d_origin = B.origin.upload(B.h_origin.data(), B.h_origin.size(), st, "boundary face origins");
        hipLaunchKernelGGL(k_fv_boundary, dim3(groups(nboundary, FV_THREADS)), wg, 0, st, d_blocks, d_origin, nboundary, ninternal, ncells, fp.Eg, fp.fpc,
                           B.owner.as<int32_t>(), B.cell_faces.as<int32_t>());
        HIPCHK(hipGetLastError());
    }
}

// stage 2 on device lists and planes; fields to the host where asked for (synchronises)
void metrics_run(hipStream_t st, const FvDev& L, const tm_fv_fields* fields, FvAcc* rec) {
    const int64_t nfaces = L.ninternal + L.nboundary;
    const int gc = static_cast<int>(std::min<int64_t>(FV_MAX_GRID, groups(L.ncells, FV_THREADS))), gf = static_cast<int>(std::min<int64_t>(FV_MAX_GRID, groups(nfaces, FV_THREADS)));
    DevBuf b_centre(sizeof(double) * 3 * static_cast<size_t>(L.ncells), "cell centres"), b_part(sizeof(FvAcc) * (static_cast<size_t>(gc) + gf + 1), "finite-volume records");
    DevBuf b_vol, b_cen, b_clo, b_area, b_fc, b_cos, b_skew;
    FvOut out{};
    const size_t nc = static_cast<size_t>(L.ncells), nf = static_cast<size_t>(nfaces), ni = static_cast<size_t>(L.ninternal), dim = static_cast<size_t>(L.dim);
    auto want = [&](double* host, DevBuf& b, size_t n, const char* what) -> double* {
        if (!host) return nullptr;
        b.grow(sizeof(double) * n, what);
        return b.as<double>();
    };
    if (fields) {
        out.volume = want(fields->volume, b_vol, nc, "cell volumes");
        out.centre = want(fields->centre, b_cen, dim * nc, "cell centre planes");
        out.closedness = want(fields->closedness, b_clo, nc, "cell closedness");
        out.area = want(fields->area, b_area, dim * nf, "face area vectors");
        out.face_centre = want(fields->face_centre, b_fc, dim * nf, "face centres");
        out.cos = want(fields->cos, b_cos, nf, "face cosines");
        out.skewness = want(fields->skewness, b_skew, ni, "face skewness");
    }
    FvAcc* d_part = b_part.as<FvAcc>();
    const double* d_centre = b_centre.as<double>();
    if (L.dim == 2) {
        hipLaunchKernelGGL(k_fv_cells<2>, dim3(gc), dim3(FV_THREADS), 0, st, L, out, b_centre.as<double>(), d_part);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_fv_faces<2>, dim3(gf), dim3(FV_THREADS), 0, st, L, out, d_centre, d_part + gc);
    } else {
        hipLaunchKernelGGL(k_fv_cells<3>, dim3(gc), dim3(FV_THREADS), 0, st, L, out, b_centre.as<double>(), d_part);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_fv_faces<3>, dim3(gf), dim3(FV_THREADS), 0, st, L, out, d_centre, d_part + gc);
    }
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_fv_final, dim3(1), dim3(64), 0, st, static_cast<const FvAcc*>(d_part), gc + gf, d_part + gc + gf);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(rec, d_part + gc + gf, sizeof(FvAcc), hipMemcpyDeviceToHost, st));
    auto back = [&](double* host, const double* dev, size_t n) {
        if (host && n) HIPCHK(hipMemcpyAsync(host, dev, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    };
    if (fields) {
        back(fields->volume, out.volume, nc);
        back(fields->centre, out.centre, dim * nc);
        back(fields->closedness, out.closedness, nc);
        back(fields->area, out.area, dim * nf);
        back(fields->face_centre, out.face_centre, dim * nf);
        back(fields->cos, out.cos, nf);
        back(fields->skewness, out.skewness, ni);
    }
    HIPCHK(hipStreamSynchronize(st));   // the buffers go out of scope behind it
}

}  // namespace

// ------------------------------------------------------------------ handle: the coordinates resident in X
void Smoother::fv_report_host(const int32_t* block_orientation, tm_fv_info* info) {
    if (lp.nranks > 1) throw TmError(TM_E_UNSUPPORTED, "welding needs every block in one handle: not served with rank hooks");
    std::vector<tm_block> tb;
    std::vector<tm_connection> tc;
    std::vector<tm_condition> tq;
    std::vector<const double2*> blocks_x;
    weld_tables(tb, tc, tq, blocks_x);
    tm_mesh_desc desc{tb.data(), tb.size(), tc.data(), tc.size(), tq.data(), tq.size()};
    const WeldPlan pl = weld_plan(&desc);
    const WeldBoundaryPlan bp = weld_boundary_plan(&desc, pl, 1, 0);
    std::vector<int32_t> orient(static_cast<size_t>(pl.nblocks()), 1);
    if (block_orientation) {
        orient.assign(block_orientation, block_orientation + pl.nblocks());
    } else {   // the rule of tm_smoother_quality
        std::vector<tm_quality> per(static_cast<size_t>(pl.nblocks()));
        quality_host(per.data(), nullptr);
        for (int b = 0; b < pl.nblocks(); ++b) orient[b] = per[b].orientation;
    }
    const FvPlan fp = fv_plan(&desc, pl, bp, 0, orient.data());
    if (!welddev) welddev = new WeldDev();
    tm_weld_info rec;
    welddev->link(pl, stream);
    welddev->number(pl, stream);
    welddev->read_map(pl, stream, nullptr, &rec);
    const int64_t nodes_out = static_cast<int64_t>(rec.nodes_out);
    WeldGap gap{0.0, 0ull};
    welddev->points_resident(pl, stream, blocks_x, nodes_out, nullptr, nullptr, &gap);   // the welded planes stay in welddev->out
    FvListBufs B;
    faces_run(pl, bp, fp, stream, *welddev, static_cast<const int32_t*>(welddev->map.p), nodes_out, 0, orient.data(), B);
    const double* ox = static_cast<const double*>(welddev->out.p);
    const FvDev L{2, 2, 4, fp.cells, fp.internal, fp.boundary, B.faces.as<int32_t>(), B.owner.as<int32_t>(), B.neighbour.as<int32_t>(), B.cell_faces.as<int32_t>(), ox,
                  ox + nodes_out, nullptr};
    FvAcc acc;
    metrics_run(stream, L, nullptr, &acc);
    const FvLists lists{2, 2, 4, fp.cells, fp.internal, fp.boundary, nodes_out, nullptr, nullptr, nullptr, nullptr};
    fv_info_from(lists, acc, info);
}

}  // namespace tmh

using namespace tmh;

extern "C" int tm_weld_faces(const tm_mesh_desc* mesh, const int32_t* map, uint64_t nodes_out, uint64_t nk, const int32_t* block_orientation, int32_t* faces,
                             int32_t* owner, int32_t* neighbour, int32_t* cell_faces) {
    return guarded([&]() {
        weld_layers(nk, nodes_out);   // sizes first: nothing is read when the ids cannot be held
        const WeldPlan pl = weld_plan(mesh);
        const WeldBoundaryPlan bp = weld_boundary_plan(mesh, pl, 1, nk);
        const FvPlan fp = fv_plan(mesh, pl, bp, nk, block_orientation);
        if (!map || !faces || !owner || (!neighbour && fp.internal)) throw TmError(TM_E_ARG, "null argument");
        for (int64_t n = 0; n < pl.nodes; ++n)   // the kernels add layer offsets to these ids
            if (map[n] < 0 || static_cast<uint64_t>(map[n]) >= nodes_out) throw TmError(TM_E_ARG, "map holds an id outside 0 .. nodes_out - 1");
        require_gfx950();
        WeldDev wd;
        wd.upload_map(pl, nullptr, map);
        FvListBufs B;
        faces_run(pl, bp, fp, nullptr, wd, static_cast<const int32_t*>(wd.map.p), static_cast<int64_t>(nodes_out), nk, block_orientation, B);
        const size_t nfaces = static_cast<size_t>(fp.internal + fp.boundary);
        HIPCHK(hipMemcpyAsync(faces, B.faces.p, sizeof(int32_t) * nfaces * fp.npf, hipMemcpyDeviceToHost, nullptr));
        HIPCHK(hipMemcpyAsync(owner, B.owner.p, sizeof(int32_t) * nfaces, hipMemcpyDeviceToHost, nullptr));
        if (fp.internal) HIPCHK(hipMemcpyAsync(neighbour, B.neighbour.p, sizeof(int32_t) * static_cast<size_t>(fp.internal), hipMemcpyDeviceToHost, nullptr));
        if (cell_faces) HIPCHK(hipMemcpyAsync(cell_faces, B.cell_faces.p, sizeof(int32_t) * static_cast<size_t>(fp.cells) * fp.fpc, hipMemcpyDeviceToHost, nullptr));
        HIPCHK(hipStreamSynchronize(nullptr));
        return TM_OK;
    });
}

extern "C" int tm_fv_metrics(int32_t dim, uint64_t ncells, uint64_t ninternal, uint64_t nboundary, const int32_t* faces, const int32_t* owner,
                             const int32_t* neighbour, const int32_t* cell_faces, uint64_t npoints, const double* const* points, const tm_fv_fields* fields,
                             tm_fv_info* info) {
    return guarded([&]() {
        const FvLists H = fv_metrics_check(dim, ncells, ninternal, nboundary, faces, owner, neighbour, cell_faces, npoints, points);
        require_gfx950();
        const size_t nfaces = static_cast<size_t>(H.ninternal + H.nboundary);
        DevBuf b_faces, b_owner, b_nb, b_cf, b_pts(sizeof(double) * npoints * dim, "welded planes");
        const int32_t* d_faces = b_faces.upload(faces, nfaces * H.npf, nullptr, "faces");
        const int32_t* d_owner = b_owner.upload(owner, nfaces, nullptr, "face owners");
        const int32_t* d_nb = b_nb.upload(neighbour, static_cast<size_t>(H.ninternal), nullptr, "face neighbours");
        const int32_t* d_cf = b_cf.upload(cell_faces, static_cast<size_t>(H.ncells) * H.fpc, nullptr, "faces of the cells");
        double* d_pts = b_pts.as<double>();
        for (int c = 0; c < dim; ++c)
            if (npoints) HIPCHK(hipMemcpyAsync(d_pts + static_cast<size_t>(c) * npoints, points[c], sizeof(double) * npoints, hipMemcpyHostToDevice, nullptr));
        const FvDev L{H.dim, H.npf, H.fpc, H.ncells, H.ninternal, H.nboundary, d_faces, d_owner, d_nb, d_cf, d_pts, d_pts + npoints, dim == 3 ? d_pts + 2 * npoints : nullptr};
        FvAcc acc;
        metrics_run(nullptr, L, fields, &acc);
        fv_info_from(H, acc, info);
        return TM_OK;
    });
}

extern "C" int tm_smoother_fv_report(tm_smoother* s, const int32_t* block_orientation, tm_fv_info* info) {
    return guarded([&]() {
        if (!s || !smoother_is_live(s)) throw TmError(TM_E_ARG, "not a live handle");
        if (!info) throw TmError(TM_E_ARG, "info is needed");
        s->impl.fv_report_host(block_orientation, info);
        return TM_OK;
    });
}
