// Host side of K20 (include/tm_hip.h, "wall distance of the welded mesh"): the argument checks, the selection of wall faces and images
// from a boundary plan, and the host twin -- plain loops over all pairs through the definitions of tm_wall_distance.hpp.  No HIP call in
// this file: it works in a process without a device.
#include "tm_wall_distance.hpp"
#include "tm_weld_boundary.hpp"
#include "tm_api_util.hpp"

#include <algorithm>
#include <cmath>
#include <limits>
#include <string>
#include <vector>

namespace tmh {

int64_t wall_check(int dim, uint64_t nfaces, const int32_t* faces, uint64_t npoints, const double* const* points, uint64_t nimages, const tm_wall_image* images,
                   const double* distance) {
    if (dim != 2 && dim != 3) throw TmError(TM_E_ARG, "dim: 2 (edges of a plane mesh) or 3 (quadrilaterals of a stacked one)");
    if (!faces || !points || !images || !distance) throw TmError(TM_E_ARG, "null argument");
    for (int c = 0; c < dim; ++c)
        if (!points[c]) throw TmError(TM_E_ARG, "null coordinate plane");
    if (nfaces == 0) throw TmError(TM_E_ARG, "no wall face");
    if (nfaces > static_cast<uint64_t>(WELD_MAX_ID) || npoints > static_cast<uint64_t>(WELD_MAX_ID)) throw TmError(TM_E_ARG, "more than 2^31 - 1 faces or points");
    if (nimages < 1 || nimages > static_cast<uint64_t>(WD_MAX_IMAGES)) throw TmError(TM_E_ARG, "images: 1 .. 16, image 0 the identity");
    const tm_wall_image& id = images[0];
    if (!(id.t[0] == 0.0 && id.t[1] == 0.0 && id.t[2] == 0.0 && id.c == 1.0 && id.s == 0.0)) throw TmError(TM_E_ARG, "image 0 must be the identity {0, 0, 0, 1, 0}");
    if (dim == 2)
        for (uint64_t m = 0; m < nimages; ++m)
            if (images[m].c != 1.0) throw TmError(TM_E_ARG, "image " + std::to_string(m) + ": c must be 1 in a plane mesh");
    const int npf = dim == 2 ? 2 : 4;
    const size_t n = static_cast<size_t>(nfaces) * npf;
    const uint32_t limit = static_cast<uint32_t>(npoints);
    for (size_t k = 0; k < n; ++k)
        if (static_cast<uint32_t>(faces[k]) >= limit) throw TmError(TM_E_ARG, "face " + std::to_string(k / npf) + " names point " + std::to_string(faces[k]) + " of " + std::to_string(npoints));
    return static_cast<int64_t>(nfaces) * (dim == 2 ? 1 : 2);
}

void wall_info_sizes(int dim, uint64_t nfaces, uint64_t npoints, uint64_t nimages, tm_wall_info* info) {
    info->points = npoints;
    info->faces = nfaces;
    info->primitives = nfaces * (dim == 2 ? 1 : 2);
    info->images = nimages;
    info->groups = (info->primitives + WD_GROUP - 1) / WD_GROUP;
}

void wall_distance_host(int dim, uint64_t nfaces, const int32_t* faces, uint64_t npoints, const double* const* points, uint64_t nimages, const tm_wall_image* images,
                        double* distance, int32_t* face, int32_t* image, tm_wall_info* info) {
    std::vector<WdSeg> segs;
    std::vector<WdTri> tris;
    auto node = [&](int32_t id, double* P) {
        for (int c = 0; c < 3; ++c) P[c] = c < dim ? points[c][id] : 0.0;
    };
    for (uint64_t f = 0; f < nfaces; ++f) {
        double P[4][3];
        for (int k = 0; k < (dim == 2 ? 2 : 4); ++k) node(faces[f * (dim == 2 ? 2 : 4) + k], P[k]);
        if (dim == 2) {
            segs.push_back(wd_build_seg(P[0], P[1]));
        } else {
            double longest;
            tris.push_back(wd_build_tri(P[0], P[1], P[2], &longest));
            tris.push_back(wd_build_tri(P[0], P[2], P[3], &longest));
        }
    }
    tm_wall_info rec{};
    wall_info_sizes(dim, nfaces, npoints, nimages, &rec);
    rec.pairs_evaluated = npoints * rec.primitives * nimages;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    bool any = false;
    for (uint64_t i = 0; i < npoints; ++i) {
        double P[3], Q[3];
        node(static_cast<int32_t>(i), P);
        WdKey best{inf, -1, -1};
        if (!(std::isnan(P[0]) || std::isnan(P[1]) || std::isnan(P[2])))
            for (uint64_t m = 0; m < nimages; ++m) {
                wd_image_point(dim, images[m], P, Q);
                if (dim == 2)
                    for (size_t k = 0; k < segs.size(); ++k) wd_take(best, wd_seg_d2(segs[k], Q), static_cast<int32_t>(k), static_cast<int32_t>(m));
                else
                    for (size_t k = 0; k < tris.size(); ++k) wd_take(best, wd_tri_d2(tris[k], Q), static_cast<int32_t>(k >> 1), static_cast<int32_t>(m));
            }
        const double d = best.face < 0 ? nan : sqrt(best.d2);
        distance[i] = d;
        if (face) face[i] = best.face;
        if (image) image[i] = best.face < 0 ? -1 : best.image;
        if (best.face < 0) {
            rec.nan_points += 1;
            continue;
        }
        if (d == 0.0) rec.on_wall += 1;
        if (best.image != 0) rec.nearest_via_image += 1;
        if (!any || d > rec.max_distance) {
            any = true;
            rec.max_distance = d;
            rec.max_point = i;
        }
    }
    if (info) *info = rec;
}

void wall_select(const WeldBoundaryPlan& bp, uint32_t kinds_mask, std::vector<int32_t>& face_index, std::vector<tm_wall_image>& images) {
    face_index.clear();
    images.assign(1, tm_wall_image{{0.0, 0.0, 0.0}, 1.0, 0.0});
    for (size_t q = 0; q < bp.patches.size(); ++q) {
        const tm_weld_patch& r = bp.patches[q];
        if (r.kind >= 0 && r.kind < 32 && ((kinds_mask >> r.kind) & 1u))
            for (uint64_t f = 0; f < r.faces; ++f) face_index.push_back(static_cast<int32_t>(r.face_begin + f));
        if (r.kind != TM_PATCH_PERIODIC || r.partner < static_cast<int32_t>(q)) continue;
        const double tx = r.translation[0], ty = r.translation[1];
        bool seen = false;
        for (size_t m = 1; m < images.size(); ++m) seen = seen || (images[m].t[0] == tx && images[m].t[1] == ty) || (images[m].t[0] == -tx && images[m].t[1] == -ty);
        if (seen) continue;
        images.push_back(tm_wall_image{{tx, ty, 0.0}, 1.0, 0.0});
        images.push_back(tm_wall_image{{-tx, -ty, 0.0}, 1.0, 0.0});
    }
    if (images.size() > static_cast<size_t>(WD_MAX_IMAGES)) throw TmError(TM_E_ARG, "more than 7 distinct periodic translations: at most 16 images");
}

}  // namespace tmh

using namespace tmh;

extern "C" int tm_wall_distance_host(int32_t dim, uint64_t nfaces, const int32_t* faces, uint64_t npoints, const double* const* points, uint64_t nimages,
                                     const tm_wall_image* images, uint32_t, double* distance, int32_t* face, int32_t* image, tm_wall_info* info) {
    return guarded([&]() {
        wall_check(dim, nfaces, faces, npoints, points, nimages, images, distance);
        wall_distance_host(dim, nfaces, faces, npoints, points, nimages, images, distance, face, image, info);
        return TM_OK;
    });
}

extern "C" int tm_wall_select(const tm_mesh_desc* mesh, uint64_t nk, uint32_t kinds_mask, uint64_t* nfaces, int32_t* face_index, uint64_t* nimages,
                              tm_wall_image* images) {
    return guarded([&]() {
        if (!nfaces || !nimages) throw TmError(TM_E_ARG, "null argument");
        const WeldPlan pl = weld_plan(mesh);
        const WeldBoundaryPlan bp = weld_boundary_plan(mesh, pl, 1, nk);
        std::vector<int32_t> idx;
        std::vector<tm_wall_image> im;
        wall_select(bp, kinds_mask, idx, im);
        *nfaces = idx.size();
        *nimages = im.size();
        if (face_index) std::copy(idx.begin(), idx.end(), face_index);
        if (images) std::copy(im.begin(), im.end(), images);
        return TM_OK;
    });
}
