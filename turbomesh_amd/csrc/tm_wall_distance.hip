// K20 wall distance of the welded mesh.  gfx950, wave64.  Definitions: include/tm_hip.h, "wall distance of the welded mesh"; the arithmetic
//     is tm_wall_distance.hpp, shared with the host twin (tm_wall_distance_host.cpp).
//
// 1. k_wall_table: one wave per group of WD_GROUP consecutive primitives.  A lane gathers the nodes of its primitive through the ids and
//    writes the record of tm_wall_distance.hpp (edges, 1 / L, the compensated normal); the wave reduces the group's box, its longest
//    squared edge and keeps one vertex.  Minima and maxima only: the table does not depend on scheduling.
//    k_wall_chunks does the same over the WD_CHUNK groups of a chunk, so that the distance pass can rule out 4096 primitives by one box.
// 2. k_wall_distance: one point per lane, WD_THREADS per workgroup, points in id order; a workgroup walks tiles of WD_THREADS points.
//    The group records travel through LDS in chunks of WD_CHUNK.  A first pass over them seeds the lane's upper bound with the squared
//    distance to one vertex per group; the second pass tests the box of every group and image per lane and evaluates the group when ANY
//    lane of the wave cannot rule it out; a chunk is not even loaded when no lane of the workgroup needs it.  The loop over groups and
//    primitives is wave-uniform, so a primitive's record is read at a wave-uniform address.  The seed and the boxes only steer: the
//    outputs come from evaluated primitives alone.
// 3. k_wall_final: one wave combines the per-workgroup records with records_reduce_wave: integer sums and a maximum with the smallest
//    id, the same on every run.
#include "tm_wall_distance.hpp"
#include "tm_weld_boundary_dev.hpp"
#include "tm_records.hpp"
#include "tm_stack.hpp"
#include "tm_api_util.hpp"

#include <algorithm>
#include <cstring>
#include <limits>

namespace tmh {

constexpr int WD_THREADS = 256, WD_WAVES = WD_THREADS / 64;
constexpr int WD_MAX_GRID = 2048;   // workgroups of the distance launch: each leaves one record

struct WdImages {
    tm_wall_image m[WD_MAX_IMAGES];
};
struct WdAcc {   // 48 bytes
    unsigned long long on_wall, nan_points, via_image, pairs, max_point;
    double max_d;   // -1: no point yet
};
__host__ __device__ inline void wd_init(WdAcc& a) {
    a.on_wall = a.nan_points = a.via_image = a.pairs = a.max_point = 0ull;
    a.max_d = -1.0;
}
__host__ __device__ inline void wd_combine(WdAcc& a, const WdAcc& b) {
    a.on_wall += b.on_wall;
    a.nan_points += b.nan_points;
    a.via_image += b.via_image;
    a.pairs += b.pairs;
    if (b.max_d > a.max_d || (b.max_d == a.max_d && b.max_point < a.max_point)) {
        a.max_d = b.max_d;
        a.max_point = b.max_point;
    }
}

template <int DIM>
struct WdPrim;
template <>
struct WdPrim<2> {
    using type = WdSeg;
};
template <>
struct WdPrim<3> {
    using type = WdTri;
};

// ------------------------------------------------------------------ 1. primitive table and group boxes
__device__ __forceinline__ double wd_wave_min(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(v, off, 64);
        if (o < v) v = o;
    }
    return v;
}
__device__ __forceinline__ double wd_wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(v, off, 64);
        if (o > v) v = o;
    }
    return v;
}

// ids were checked against npoints on the host before the launch (wall_check); grid.x = groups, 64 lanes
template <int DIM>
__global__ __launch_bounds__(64) void k_wall_table(int nprims, const int32_t* __restrict__ faces, const double* __restrict__ px, const double* __restrict__ py,
                                                   const double* __restrict__ pz, typename WdPrim<DIM>::type* __restrict__ prims, WdGroup* __restrict__ groups) {
    const int lane = threadIdx.x, k = static_cast<int>(blockIdx.x) * WD_GROUP + lane;
    const bool own = k < nprims;
    const double inf = __builtin_huge_val();
    double lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf}, E2 = 0.0, first[3] = {0.0, 0.0, 0.0};
    bool open = false;   // a sliver: its group is never culled
    if (own) {
        constexpr int NV = DIM == 2 ? 2 : 3;
        double V[NV][3];
        if constexpr (DIM == 2) {
            const int a = faces[2 * k], b = faces[2 * k + 1];
            V[0][0] = px[a], V[0][1] = py[a], V[0][2] = 0.0;
            V[1][0] = px[b], V[1][1] = py[b], V[1][2] = 0.0;
            const WdSeg s = wd_build_seg(V[0], V[1]);
            prims[k] = s;
            E2 = s.L;
        } else {
            const int f = k >> 1, second = k & 1;
            const int id[3] = {faces[4 * f], faces[4 * f + 1 + second], faces[4 * f + 2 + second]};
#pragma unroll
            for (int v = 0; v < 3; ++v) V[v][0] = px[id[v]], V[v][1] = py[id[v]], V[v][2] = pz[id[v]];
            const WdTri t = wd_build_tri(V[0], V[1], V[2], &E2);
            prims[k] = t;
            open = wd_tri_sliver(t);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            first[c] = V[0][c];
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                if (V[v][c] < lo[c]) lo[c] = V[v][c];
                if (V[v][c] > hi[c]) hi[c] = V[v][c];
            }
        }
    }
    const bool any_open = __any(open ? 1 : 0) != 0;
    WdGroup g;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        g.lo[c] = any_open ? -inf : wd_wave_min(lo[c]);
        g.hi[c] = any_open ? inf : wd_wave_max(hi[c]);
        g.seed[c] = __shfl(first[c], 0, 64);   // lane 0 always owns a primitive: a vertex of the group's first one (as given, or its longest edge's)
    }
    g.E2 = wd_wave_max(E2);
    if (lane == 0) groups[blockIdx.x] = g;
}

// the box of the WD_CHUNK groups of a chunk, their longest squared edge, the first group's vertex: grid.x = chunks, 64 lanes
__global__ __launch_bounds__(64) void k_wall_chunks(int ngroups, const WdGroup* __restrict__ groups, WdGroup* __restrict__ chunks) {
    static_assert(WD_CHUNK == 64, "one lane per group of the chunk");
    const int lane = threadIdx.x, g = static_cast<int>(blockIdx.x) * WD_CHUNK + lane;
    const double inf = __builtin_huge_val();
    WdGroup r;
#pragma unroll
    for (int c = 0; c < 3; ++c) r.lo[c] = inf, r.hi[c] = -inf, r.seed[c] = 0.0;
    r.E2 = 0.0;
    if (g < ngroups) r = groups[g];
    WdGroup out;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        out.lo[c] = wd_wave_min(r.lo[c]);
        out.hi[c] = wd_wave_max(r.hi[c]);
        out.seed[c] = __shfl(r.seed[c], 0, 64);
    }
    out.E2 = wd_wave_max(r.E2);
    if (lane == 0) chunks[blockIdx.x] = out;
}

// ------------------------------------------------------------------ 2. distance
template <int DIM>
__device__ __forceinline__ double wd_prim_d2(const typename WdPrim<DIM>::type& p, const double* Q) {
    if constexpr (DIM == 2) return wd_seg_d2(p, Q);
    else return wd_tri_d2(p, Q);
}

// lb: the squared distance from Q to the box, below every exact d2 of what the box holds; far: the squared distance to its farthest
// corner, which with the longest squared edge bounds rho2 of every pair of the lane and the box
template <int DIM>
__device__ __forceinline__ void wd_box(const WdGroup& b, const double* Q, double& lb, double& far) {
    lb = 0.0;
    far = 0.0;
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
        const double below = b.lo[c] - Q[c], above = Q[c] - b.hi[c];
        double out = 0.0;
        if (below > out) out = below;
        if (above > out) out = above;
        lb += out * out;
        const double reach = below < above ? -below : -above;   // the larger of Q - lo and hi - Q
        far += reach * reach;
    }
}

template <int DIM>
__global__ __launch_bounds__(WD_THREADS) void k_wall_distance(const typename WdPrim<DIM>::type* __restrict__ prims, int nprims, const WdGroup* __restrict__ groups,
                                                              int ngroups, const WdGroup* __restrict__ chunks, WdImages images, int nimages, const double* __restrict__ px,
                                                              const double* __restrict__ py, const double* __restrict__ pz, long long npoints, int cull,
                                                              double* __restrict__ distance, int32_t* __restrict__ face, int32_t* __restrict__ image,
                                                              WdAcc* __restrict__ partials) {
    __shared__ WdGroup sh_g[WD_CHUNK];
    __shared__ WdAcc sh_acc[WD_WAVES];
    constexpr int GW = sizeof(WdGroup) / sizeof(double);
    const double inf = __builtin_huge_val();
    WdAcc acc;
    wd_init(acc);
    const long long ntiles = (npoints + WD_THREADS - 1) / WD_THREADS;
    auto load_chunk = [&](int c0, int cnt) {   // the whole workgroup; sh_g is free behind the first barrier and full behind the second
        __syncthreads();
        const double* src = reinterpret_cast<const double*>(groups + c0);
        double* dst = reinterpret_cast<double*>(sh_g);
        for (int w = threadIdx.x; w < cnt * GW; w += WD_THREADS) dst[w] = src[w];
        __syncthreads();
    };
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long idx = tile * WD_THREADS + threadIdx.x;
        const bool valid = idx < npoints;
        double P[3] = {0.0, 0.0, 0.0};
        if (valid) {
            P[0] = px[idx];
            P[1] = py[idx];
            if constexpr (DIM == 3) P[2] = pz[idx];
        }
        const bool active = valid && !(P[0] != P[0] || P[1] != P[1] || P[2] != P[2]);
        // the seed: the squared distance to one vertex per group and image bounds the final key from above (plus the error of that
        // primitive's own evaluation: four guards of the seed and the longest edge cover it)
        double bound0 = inf;
        if (cull) {
            double seed = inf, E2 = 0.0;   // E2: the longest squared edge of the group the seed vertex is from
            for (int c0 = 0; c0 < ngroups; c0 += WD_CHUNK) {
                const int cnt = ngroups - c0 < WD_CHUNK ? ngroups - c0 : WD_CHUNK;
                // a chunk whose box lies farther than the seed cannot improve it; leaving one out only loosens the seed
                int want = 0;
                if (active)
                    for (int m = 0; m < nimages; ++m) {
                        double Q[3], lb, far;
                        wd_image_point(DIM, images.m[m], P, Q);
                        wd_box<DIM>(chunks[c0 / WD_CHUNK], Q, lb, far);
                        if (!(lb > seed)) want = 1;
                    }
                if (!__syncthreads_or(want)) continue;
                load_chunk(c0, cnt);
                for (int m = 0; m < nimages; ++m) {
                    double Q[3];
                    wd_image_point(DIM, images.m[m], P, Q);
                    for (int g = 0; g < cnt; ++g) {
                        double d = 0.0;
#pragma unroll
                        for (int c = 0; c < DIM; ++c) {
                            const double v = Q[c] - sh_g[g].seed[c];
                            d += v * v;
                        }
                        if (d < seed) {
                            seed = d;
                            E2 = sh_g[g].E2;
                        }
                    }
                }
            }
            bound0 = seed + 4.0 * WD_GUARD * (seed + E2);
        }
        WdKey best{inf, -1, -1};
        unsigned long long pairs = 0ull;
        for (int c0 = 0; c0 < ngroups; c0 += WD_CHUNK) {
            const int cnt = ngroups - c0 < WD_CHUNK ? ngroups - c0 : WD_CHUNK;
            if (cull) {   // the same test on the box of the whole chunk: it is loaded when any lane of the workgroup cannot rule it out
                int want = 0;
                if (active) {
                    const double bound = best.d2 < bound0 ? best.d2 : bound0;
                    for (int m = 0; m < nimages; ++m) {
                        double Q[3], lb, far;
                        wd_image_point(DIM, images.m[m], P, Q);
                        wd_box<DIM>(chunks[c0 / WD_CHUNK], Q, lb, far);
                        if (!(lb > bound + WD_GUARD * (far + chunks[c0 / WD_CHUNK].E2))) want = 1;
                    }
                }
                if (!__syncthreads_or(want)) continue;
            }
            load_chunk(c0, cnt);
            for (int m = 0; m < nimages; ++m) {
                double Q[3];
                wd_image_point(DIM, images.m[m], P, Q);
                for (int g = 0; g < cnt; ++g) {
                    bool need = active;
                    if (cull) {
                        double lb, far;
                        wd_box<DIM>(sh_g[g], Q, lb, far);
                        const double bound = best.d2 < bound0 ? best.d2 : bound0;
                        if (lb > bound + WD_GUARD * (far + sh_g[g].E2)) need = false;   // a NaN anywhere keeps the group
                    }
                    if (__any(need ? 1 : 0) == 0) continue;
                    const int base = __builtin_amdgcn_readfirstlane((c0 + g) * WD_GROUP);
                    const int n = nprims - base < WD_GROUP ? nprims - base : WD_GROUP;
                    if (active) {
                        for (int k = 0; k < n; ++k) {
                            const double d2 = wd_prim_d2<DIM>(prims[base + k], Q);
                            wd_take(best, d2, DIM == 2 ? base + k : (base + k) >> 1, m);
                        }
                        pairs += static_cast<unsigned long long>(n);
                    }
                }
            }
        }
        if (valid) {
            const bool served = best.face >= 0;
            const double d = served ? sqrt(best.d2) : __builtin_nan("");
            distance[idx] = d;
            if (face) face[idx] = best.face;
            if (image) image[idx] = served ? best.image : -1;
            acc.pairs += pairs;
            if (!served) {
                acc.nan_points += 1ull;
            } else {
                if (d == 0.0) acc.on_wall += 1ull;
                if (best.image != 0) acc.via_image += 1ull;
                if (d > acc.max_d) {   // tiles ascend: the first point at a maximum is the smallest id
                    acc.max_d = d;
                    acc.max_point = static_cast<unsigned long long>(idx);
                }
            }
        }
    }
    // wave, then workgroup, in fixed order
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        WdAcc o;
        o.on_wall = __shfl_down(acc.on_wall, off, 64);
        o.nan_points = __shfl_down(acc.nan_points, off, 64);
        o.via_image = __shfl_down(acc.via_image, off, 64);
        o.pairs = __shfl_down(acc.pairs, off, 64);
        o.max_point = __shfl_down(acc.max_point, off, 64);
        o.max_d = __shfl_down(acc.max_d, off, 64);
        if ((threadIdx.x & 63) + off < 64) wd_combine(acc, o);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh_acc[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        WdAcc t = sh_acc[0];
        for (int w = 1; w < WD_WAVES; ++w) wd_combine(t, sh_acc[w]);
        partials[blockIdx.x] = t;
    }
}

// ------------------------------------------------------------------ 3. the record
__global__ __launch_bounds__(64) void k_wall_final(const WdAcc* __restrict__ partials, int nwg, WdAcc* __restrict__ out) {
    __shared__ WdAcc sh[64];
    records_reduce_wave<WdAcc, wd_init, wd_combine>(partials, 0, nwg, sh);
    if (threadIdx.x == 0) out[0] = sh[0];
}

// ------------------------------------------------------------------ host driver
namespace {

// d_faces: the wall faces on the device, checked; d_p*: npoints doubles per component on the device; outputs to the host (synchronises)
template <int DIM>
void wall_run(hipStream_t st, int64_t nfaces, const int32_t* d_faces, int64_t npoints, const double* d_px, const double* d_py, const double* d_pz, int nimages,
              const tm_wall_image* images, uint32_t flags, double* distance, int32_t* face, int32_t* image, tm_wall_info* info) {
    using Prim = typename WdPrim<DIM>::type;
    const int64_t nprims = nfaces * (DIM == 2 ? 1 : 2);
    const int ngroups = static_cast<int>((nprims + WD_GROUP - 1) / WD_GROUP);
    const int64_t ntiles = (npoints + WD_THREADS - 1) / WD_THREADS;
    const int nwg = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(ntiles, WD_MAX_GRID)));
    const int nchunks = (ngroups + WD_CHUNK - 1) / WD_CHUNK;
    DevBuf b_prims(sizeof(Prim) * static_cast<size_t>(nprims), "wall primitives"), b_groups(sizeof(WdGroup) * static_cast<size_t>(ngroups), "wall groups");
    DevBuf b_chunks(sizeof(WdGroup) * static_cast<size_t>(nchunks), "wall chunks");
    DevBuf b_dist(sizeof(double) * static_cast<size_t>(npoints), "wall distance"), b_face(sizeof(int32_t) * static_cast<size_t>(npoints), "nearest faces");
    DevBuf b_image(sizeof(int32_t) * static_cast<size_t>(npoints), "nearest images"), b_part(sizeof(WdAcc) * (static_cast<size_t>(nwg) + 1), "wall records");
    WdImages im;
    std::memset(&im, 0, sizeof(im));
    for (int m = 0; m < nimages; ++m) im.m[m] = images[m];
    hipLaunchKernelGGL(k_wall_table<DIM>, dim3(static_cast<unsigned>(ngroups)), dim3(64), 0, st, static_cast<int>(nprims), d_faces, d_px, d_py, d_pz, b_prims.as<Prim>(),
                       b_groups.as<WdGroup>());
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_wall_chunks, dim3(static_cast<unsigned>(nchunks)), dim3(64), 0, st, ngroups, b_groups.as<WdGroup>(), b_chunks.as<WdGroup>());
    HIPCHK(hipGetLastError());
    WdAcc* d_part = b_part.as<WdAcc>();
    hipLaunchKernelGGL(k_wall_distance<DIM>, dim3(static_cast<unsigned>(nwg)), dim3(WD_THREADS), 0, st, b_prims.as<Prim>(), static_cast<int>(nprims), b_groups.as<WdGroup>(),
                       ngroups, b_chunks.as<WdGroup>(), im, nimages, d_px, d_py, d_pz, static_cast<long long>(npoints), (flags & TM_WALL_NO_CULL) ? 0 : 1, b_dist.as<double>(),
                       b_face.as<int32_t>(), b_image.as<int32_t>(), d_part);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_wall_final, dim3(1), dim3(64), 0, st, d_part, nwg, d_part + nwg);
    HIPCHK(hipGetLastError());
    WdAcc rec;
    HIPCHK(hipMemcpyAsync(&rec, d_part + nwg, sizeof(WdAcc), hipMemcpyDeviceToHost, st));
    if (npoints) {
        HIPCHK(hipMemcpyAsync(distance, b_dist.p, sizeof(double) * static_cast<size_t>(npoints), hipMemcpyDeviceToHost, st));
        if (face) HIPCHK(hipMemcpyAsync(face, b_face.p, sizeof(int32_t) * static_cast<size_t>(npoints), hipMemcpyDeviceToHost, st));
        if (image) HIPCHK(hipMemcpyAsync(image, b_image.p, sizeof(int32_t) * static_cast<size_t>(npoints), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));   // the buffers go out of scope behind it
    if (info) {
        wall_info_sizes(DIM, static_cast<uint64_t>(nfaces), static_cast<uint64_t>(npoints), static_cast<uint64_t>(nimages), info);
        info->on_wall = rec.on_wall;
        info->nan_points = rec.nan_points;
        info->nearest_via_image = rec.via_image;
        info->pairs_evaluated = rec.pairs;
        info->max_distance = rec.max_d < 0.0 ? 0.0 : rec.max_d;
        info->max_point = rec.max_d < 0.0 ? 0ull : rec.max_point;
    }
}

}  // namespace

// ------------------------------------------------------------------ handle: the coordinates resident in X
void Smoother::wall_distance_host(uint32_t kinds_mask, uint32_t flags, const int32_t* block_orientation, double* distance, int32_t* face, int32_t* image,
                                  tm_wall_info* info) {
    if (lp.nranks > 1) throw TmError(TM_E_UNSUPPORTED, "welding needs every block in one handle: not served with rank hooks");
    std::vector<tm_block> tb;
    std::vector<tm_connection> tc;
    std::vector<tm_condition> tq;
    std::vector<const double2*> blocks_x;
    weld_tables(tb, tc, tq, blocks_x);
    tm_mesh_desc desc{tb.data(), tb.size(), tc.data(), tc.size(), tq.data(), tq.size()};
    const WeldPlan pl = weld_plan(&desc);
    const WeldBoundaryPlan bp = weld_boundary_plan(&desc, pl, 1, 0);
    std::vector<int32_t> index;
    std::vector<tm_wall_image> images;
    wall_select(bp, kinds_mask, index, images);
    if (index.empty()) throw TmError(TM_E_ARG, "no face of the boundary has one of the kinds asked for");
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
    weld_faces_run(pl, bp, stream, static_cast<const int32_t*>(welddev->map.p), nodes_out, 0, orient.data(), b_faces.as<int32_t>(), keep);
    // the perimeter is small: the selected faces are gathered on the host (ids of a welded map: inside 0 .. nodes_out - 1)
    std::vector<int32_t> all(nids), wall(index.size() * 2);
    HIPCHK(hipMemcpyAsync(all.data(), b_faces.p, sizeof(int32_t) * nids, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    for (size_t f = 0; f < index.size(); ++f)
        for (int k = 0; k < 2; ++k) {
            const int32_t id = all[static_cast<size_t>(index[f]) * 2 + k];
            if (id < 0 || id >= nodes_out) throw TmError(TM_E_OVERFLOW, "a boundary face names a node outside the weld");
            wall[2 * f + k] = id;
        }
    DevBuf b_wall;
    const int32_t* d_wall = b_wall.upload(wall.data(), wall.size(), stream, "wall faces");
    const double* ox = static_cast<const double*>(welddev->out.p);
    wall_run<2>(stream, static_cast<int64_t>(index.size()), d_wall, nodes_out, ox, ox + nodes_out, nullptr, static_cast<int>(images.size()), images.data(), flags, distance,
                face, image, info);
    if (face)
        for (int64_t n = 0; n < nodes_out; ++n)
            if (face[n] >= 0) face[n] = index[static_cast<size_t>(face[n])];
}

}  // namespace tmh

using namespace tmh;

extern "C" int tm_wall_distance(int32_t dim, uint64_t nfaces, const int32_t* faces, uint64_t npoints, const double* const* points, uint64_t nimages,
                                const tm_wall_image* images, uint32_t flags, double* distance, int32_t* face, int32_t* image, tm_wall_info* info) {
    return guarded([&]() {
        wall_check(dim, nfaces, faces, npoints, points, nimages, images, distance);
        require_gfx950();
        DevBuf b_faces, b_pts(sizeof(double) * npoints * dim, "welded planes");
        const int32_t* d_faces = b_faces.upload(faces, static_cast<size_t>(nfaces) * (dim == 2 ? 2 : 4), nullptr, "wall faces");
        double* d_pts = b_pts.as<double>();
        for (int c = 0; c < dim; ++c)
            if (npoints) HIPCHK(hipMemcpyAsync(d_pts + static_cast<size_t>(c) * npoints, points[c], sizeof(double) * npoints, hipMemcpyHostToDevice, nullptr));
        if (dim == 2)
            wall_run<2>(nullptr, static_cast<int64_t>(nfaces), d_faces, static_cast<int64_t>(npoints), d_pts, d_pts + npoints, nullptr, static_cast<int>(nimages), images, flags,
                        distance, face, image, info);
        else
            wall_run<3>(nullptr, static_cast<int64_t>(nfaces), d_faces, static_cast<int64_t>(npoints), d_pts, d_pts + npoints, d_pts + 2 * npoints, static_cast<int>(nimages),
                        images, flags, distance, face, image, info);
        return TM_OK;
    });
}

extern "C" int tm_smoother_wall_distance(tm_smoother* s, uint32_t kinds_mask, uint32_t flags, const int32_t* block_orientation, double* distance, int32_t* face,
                                         int32_t* image, tm_wall_info* info) {
    return guarded([&]() {
        if (!s || !smoother_is_live(s)) throw TmError(TM_E_ARG, "not a live handle");
        if (!distance) throw TmError(TM_E_ARG, "distance is needed");
        s->impl.wall_distance_host(kinds_mask, flags, block_orientation, distance, face, image, info);
        return TM_OK;
    });
}
