// What the device entry points over K cuts share (tm_stack.hip: K11, tm_stack_quality.hip: K12, K16, K17): the kernels' argument block,
// RAII events, the preambles of the entry points (plan, cuts to the device or resolved from K handles behind their pending work) and
// the weight table.
#pragma once
#include "tm_stack.hpp"
#include "tm_stack_surface.hpp"
#include "tm_api_util.hpp"
#include "tm_devbuf.hpp"

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace tmh {

struct StackCuts {
    const double2* xy[TM_STACK_MAX_CUTS];   // the block in each cut, node (i,j) at i*nj + j
    double radius[TM_STACK_MAX_CUTS];       // z[c] (cylindrical mapping)
};

// the meridional tables of a TM_STACK_REVOLUTION call on the device (K15); null pointers with the other mappings.  The reference radii
// travel in StackCuts::radius.
struct StackSurf {
    const double* knots;   // u, cut after cut
    const double* coef;    // 8 per interval, cut after cut
    int first[TM_STACK_MAX_CUTS];    // index of cut c's first knot; its first coefficient is (first[c] - c) * 8
    int nknots[TM_STACK_MAX_CUTS];   // 2 .. TM_STACK_MAX_KNOTS
};

struct StackEvent {
    hipEvent_t e = nullptr;
    StackEvent() { HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); }
    ~StackEvent() { (void)hipEventDestroy(e); }
    StackEvent(const StackEvent&) = delete;
    StackEvent& operator=(const StackEvent&) = delete;
};

// radius[] from the plan, unused entries neutral
inline void stack_fill_radii(const StackPlan& p, StackCuts& cuts) {
    for (int c = 0; c < TM_STACK_MAX_CUTS; ++c) {
        cuts.radius[c] = c < p.ncuts ? p.span[c] : 1.0;
        if (c >= p.ncuts) cuts.xy[c] = nullptr;
    }
}

// K15, one cut.  Staging: every thread t < TM_STACK_MAX_KNOTS of the workgroup writes one entry of `sh_u`, knot t of the cut up to
// N-2 and +inf behind it (surf_locate_padded); the caller's barrier follows.
__device__ __forceinline__ void stack_surf_stage(double* sh_u, const StackSurf& surf, int c, int t) {
    if (t < TM_STACK_MAX_KNOTS) sh_u[t] = t < surf.nknots[c] - 1 ? surf.knots[surf.first[c] + t] : __builtin_huge_val();
}
// Search and evaluation on the lane's node: the knots from LDS, the table's last knot under a wave-uniform address, the 64 bytes of the
// interval's coefficients gathered from the table (L2).  Returns whether u lies outside the table.
__device__ __forceinline__ bool stack_surf_node(const double* sh_u, const StackSurf& surf, int c, double un, double* x, double* r) {
    const int N = surf.nknots[c];
    const int n = surf_locate_padded(sh_u, surf_first_step(N), un);   // <= N-2: inside the cut's table
    const double4* __restrict__ q = reinterpret_cast<const double4*>(surf.coef + (static_cast<size_t>(surf.first[c] - c) + n) * SURF_COEF);
    const double4 qx = q[0], qr = q[1];
    const double cf[SURF_COEF] = {qx.x, qx.y, qx.z, qx.w, qr.x, qr.y, qr.z, qr.w};
    double xs, rs;
    surf_eval(cf, un - sh_u[n], &xs, &rs);
    // the two values are wanted HERE: left to itself the scheduler carries the 16 registers of coefficients of every cut past the next
    // barrier and evaluates late, which costs 12 registers per cut
    asm volatile("" : "+v"(xs), "+v"(rs));
    *x = xs;
    *r = rs;
    return surf_outside(sh_u[0], surf.knots[surf.first[c] + N - 1], un);
}

// The tables of `sf` into one device buffer on `st` (`host` must live until st has been synchronised); reference radii into cuts.radius.
struct StackSurfDev {
    std::vector<double> host;
    DevBuf dev;
    StackSurf surf{};
};
void stack_surf_upload(const StackPlan& p, const SurfPlan& sf, StackCuts& cuts, StackSurfDev& d, hipStream_t st);
// K11 on `st`: nk layers of the block into the device planes X, Y, Z; table: per layer K weights followed by s[k] (tm_stack.hip)
hipError_t launch_stack_planes(int K, const StackCuts& cuts, const StackSurf& surf, int mapping, const double* table, int nk, int ni, int nj, double* X, double* Y,
                               double* Z, unsigned long long* outside, hipStream_t st);

// The plan of an entry point that may come with meridional tables: TM_E_ARG for null options or tables without TM_STACK_REVOLUTION;
// *used = &sf (filled) with TM_STACK_REVOLUTION, null otherwise.
StackPlan stack_plan_any(const tm_stack_opt* opt, const tm_stack_surfaces* surfaces, SurfPlan& sf, const SurfPlan** used);
// Block `block` of K host descriptions (checked already: ni x nj nodes each) into `in`, cut after cut, and their addresses into dc; makes
// the gfx950 check first.
void stack_upload_cuts(const tm_mesh_desc* const* cuts, int ncuts, uint64_t block, uint64_t ni, uint64_t nj, DevBuf& in, StackCuts& dc);
// Layers [k_begin, k_begin + k_count) of the plan as the kernels read them: per layer K weights followed by s[k]; `extra` doubles of room
// behind the rows for a caller's own tables.
std::vector<double> stack_weight_table(const StackPlan& p, uint64_t k_begin, uint64_t k_count, size_t extra = 0);
// Block `block` of K live handles: TM_E_ARG / TM_E_SIZE as include/tm_hip.h says for tm_stack_smoothers; the device pointers into dc and
// the block's size into ni, nj.
void stack_resident_cuts(tm_smoother* const* cuts, const StackPlan& p, uint64_t block, StackCuts& dc, uint64_t* ni, uint64_t* nj);
// Behind the pending work of every handle: the first handle's stream (returned) waits for an event recorded on each of the other
// streams (the same stream twice is harmless).  The events live in `events` until the caller has synchronised.
hipStream_t stack_order_behind(tm_smoother* const* cuts, int ncuts, std::vector<std::unique_ptr<StackEvent>>& events);

}  // namespace tmh
