// What the device entry points over K cuts share (tm_stack.hip: K11, tm_stack_quality.hip: K12): the kernels' argument block, RAII
// buffers and events, the gfx950 check, and the K handles of a call resolved to device pointers behind their pending work.
#pragma once
#include "tm_stack.hpp"
#include "tm_api_util.hpp"
#include "tm_smoother.hpp"

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

struct StackBuf {   // RAII device buffer
    void* p = nullptr;
    explicit StackBuf(size_t bytes, const char* what) {
        if (hipMalloc(&p, bytes ? bytes : 256) != hipSuccess) throw TmError(TM_E_MEMORY, std::string("hipMalloc failed (") + what + ")");
    }
    ~StackBuf() { (void)hipFree(p); }
    StackBuf(const StackBuf&) = delete;
    StackBuf& operator=(const StackBuf&) = delete;
    template <class T>
    T* as() { return static_cast<T*>(p); }
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

inline void require_gfx950_stack() {
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, dev));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        throw TmError(TM_E_HIP, std::string("libtm_hip is built for gfx950 (MI355X) only, found ") + prop.gcnArchName);
}

// Block `block` of K live handles: TM_E_ARG / TM_E_SIZE as include/tm_hip.h says for tm_stack_smoothers; the device pointers into dc and
// the block's size into ni, nj.
void stack_resident_cuts(tm_smoother* const* cuts, const StackPlan& p, uint64_t block, StackCuts& dc, uint64_t* ni, uint64_t* nj);
// Behind the pending work of every handle: the first handle's stream (returned) waits for an event recorded on each of the other
// streams (the same stream twice is harmless).  The events live in `events` until the caller has synchronised.
hipStream_t stack_order_behind(tm_smoother* const* cuts, int ncuts, std::vector<std::unique_ptr<StackEvent>>& events);

}  // namespace tmh
