// The library's one RAII device buffer, and the gfx950 check every entry point that brings its own device memory makes first.
#pragma once
#include "tm_smoother.hpp"

#include <cstring>
#include <string>

namespace tmh {

// hipMalloc'ed on demand, grown when short, freed with the owner.  A request for 0 bytes allocates 256, so `p` is never null behind a
// successful grow().
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;   // bytes
    DevBuf() = default;
    DevBuf(size_t bytes, const char* what) { grow(bytes, what); }
    ~DevBuf() { (void)hipFree(p); }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    // at least `bytes` behind the call; the contents are NOT kept when the buffer is reallocated
    void grow(size_t bytes, const char* what) {
        if (bytes == 0) bytes = 256;
        if (cap >= bytes) return;
        release();
        if (hipMalloc(&p, bytes) != hipSuccess) {
            p = nullptr;
            throw TmError(TM_E_MEMORY, std::string("hipMalloc failed (") + what + ")");
        }
        cap = bytes;
    }
    void release() {
        (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
    // n elements of `host` into the buffer on `st` (asynchronous: `host` must live until st has been synchronised)
    template <class T>
    T* upload(const T* host, size_t n, hipStream_t st, const char* what) {
        grow(sizeof(T) * n, what);
        if (n) hip_check(hipMemcpyAsync(p, host, sizeof(T) * n, hipMemcpyHostToDevice, st), "hipMemcpyAsync (upload)");
        return as<T>();
    }
};

inline void require_gfx950() {
    static int checked = 0;
    if (checked) return;
    int dev = 0;
    hip_check(hipGetDevice(&dev), "hipGetDevice(&dev)");
    hipDeviceProp_t prop;
    hip_check(hipGetDeviceProperties(&prop, dev), "hipGetDeviceProperties(&prop, dev)");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        throw TmError(TM_E_HIP, std::string("libtm_hip is built for gfx950 (MI355X) only, found ") + prop.gcnArchName);
    checked = 1;
}

}  // namespace tmh
