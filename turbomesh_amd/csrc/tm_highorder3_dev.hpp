// Device side of the high-order hexahedra (K16): the tile constants, the kernel's argument block and the per-order launchers.  The
// kernel template is tm_highorder3_kernel.hpp; each order is instantiated in a translation unit of its own (tm_highorder3_p1.hip ..
// tm_highorder3_p4.hip: 45 kernels each, K = 2 .. 16 times three mappings), the driver and the entry points are tm_highorder3.hip.
#pragma once
#include "tm_highorder3.hpp"
#include "tm_highorder_dev.hpp"
#include "tm_stack_dev.hpp"

namespace tmh {

constexpr int HO3_THREADS = 256, HO3_WAVES = HO3_THREADS / 64;
// whole elements of a tile along i and j: (EI*p + 1) * (EJ*p + 1) nodes <= HO3_THREADS, one thread per node
constexpr int ho3_tile_ei(int p) { return p == 3 ? 5 : 16 / p; }
constexpr int ho3_tile_ej(int p) { return p == 3 ? 5 : 14 / p; }

struct Ho3Launch {
    StackCuts cuts;
    StackSurf surf;
    const double* table;   // per layer K weights and s[k]
    const double* tab;     // T then D
    int mapping, ni, nj, Ei, Ej, g0, g1, gs0, gsn, identity;
    double *X, *Y, *Z;
    double2* pairs;
    HoAcc* partials;
    unsigned long long* outside;
};

template <int P>
hipError_t ho3_launch(int K, const Ho3Launch& a, hipStream_t st);

// Tables up, K16 and the finalize on `st`, planes / record / pairs back; returns when they have arrived.  The sizes have been checked.
// pairs_dev (may be null; then sj must be null): the (Jmin, Jmax) pairs of the whole block stay on the device in the caller's buffer (K17).
void ho3_run(const StackPlan& p, const HoPlan& pl, StackCuts& cuts, uint64_t block, uint64_t ni, uint64_t nj, uint64_t g_begin, uint64_t g_count, double* x,
             double* y, double* z, tm_ho3_quality* q, double* sj, hipStream_t st, const SurfPlan* sf, uint64_t* outside, double2* pairs_dev = nullptr);

}  // namespace tmh
