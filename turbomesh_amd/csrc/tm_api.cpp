// extern "C" surface of libtm_hip.so (declared in include/tm_hip.h; measurement / diagnostic entry points in include/tm_hip_diag.h).
#include "tm_smoother.hpp"
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>

using namespace tmh;

#include "tm_api_util.hpp"
#include "tm_devbuf.hpp"
#include "tm_ilu.hpp"
#include "tm_refine.hpp"
#include "tm_quality_dev.hpp"
#include "tm_stack.hpp"

#include <mutex>
#include <set>

// the handles tm_smoother_create has handed out and tm_smoother_destroy has not taken back: what lets a call that takes a LIST of handles
// (tm_stack_smoothers) refuse a destroyed one without touching its memory
static std::mutex g_live_mutex;
static std::set<const tm_smoother*> g_live_handles;
bool tmh::smoother_is_live(const tm_smoother* s) {
    std::lock_guard<std::mutex> lock(g_live_mutex);
    return g_live_handles.count(s) != 0;
}

static bool close2(const double* a, const double* b, double tol) { return std::fabs(a[0] - b[0]) <= tol && std::fabs(a[1] - b[1]) <= tol; }

template <class T>
static T* dup(const std::vector<T>& v) {
    T* p = static_cast<T*>(std::malloc(sizeof(T) * (v.empty() ? 1 : v.size())));
    if (!p) throw TmError(TM_E_MEMORY, "out of host memory");
    if (!v.empty()) std::memcpy(p, v.data(), sizeof(T) * v.size());
    return p;
}

extern "C" {

const char* tm_last_error(void) { return g_last_error.c_str(); }
int tm_abi_version(void) { return TM_HIP_ABI_VERSION; }
void tm_set_log(tm_log_fn sink, void* ctx) {
    g_log_sink = sink;
    g_log_ctx = ctx;
}

#ifdef TM_DEBUG_EXPORTS   // measurement build only (libtm_hip_dbg.so, tools/): not in include/tm_hip.h
// one ILU(0) application M^-1 r on a caller-assembled system, timed with an event pair per repeat (tools/reference_solve_timing.py):
// packed != 0 the level-packed substitution kernels, 0 the level-by-level kernels; ms_out[repeats]; *levels = forward + backward levels
int tm_debug_ilu0_apply_ms(uint64_t n64, const int32_t* Ap, const int32_t* Ai, const double* Ax, int packed, int repeats, double* ms_out, int32_t* levels) {
    return guarded([&]() {
        if (!Ap || !Ai || !Ax || !ms_out || repeats < 1) throw TmError(TM_E_ARG, "null argument");
        if (n64 == 0 || n64 >= (uint64_t{1} << 31)) throw TmError(TM_E_SIZE, "system size out of range");
        require_gfx950();
        const int n = static_cast<int>(n64);
        const size_t nnz = static_cast<size_t>(Ap[n]);
        for (size_t k = 0; k < nnz; ++k)
            if (Ai[k] < 0 || Ai[k] >= n) throw TmError(TM_E_ARG, "InvalidMatrix: column index out of range");
        DevBuf d_p(sizeof(int32_t) * (static_cast<size_t>(n) + 1), "csr p"), d_i(sizeof(int32_t) * nnz, "csr i"), d_v(sizeof(double) * nnz, "csr v"), d_r(sizeof(double2) * static_cast<size_t>(n), "csr r"),
            d_z(sizeof(double2) * static_cast<size_t>(n), "csr z");
        HIPCHK(hipMemcpy(d_p.p, Ap, sizeof(int32_t) * (static_cast<size_t>(n) + 1), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_i.p, Ai, sizeof(int32_t) * nnz, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_v.p, Ax, sizeof(double) * nnz, hipMemcpyHostToDevice));
        std::vector<double2> r(static_cast<size_t>(n));
        for (int k = 0; k < n; ++k) r[k] = make_double2(1.0 + 1e-3 * (k % 97), 1.0 - 1e-3 * (k % 89));
        HIPCHK(hipMemcpy(d_r.p, r.data(), sizeof(double2) * r.size(), hipMemcpyHostToDevice));
        IluState ilu(n, Ap, Ai, nnz, false, packed ? 1 : 0);
        if (packed && !ilu.packed) throw TmError(TM_E_UNSUPPORTED, "this pattern has no packed form (a row with more than 16 entries on one side of the diagonal)");
        if (levels) *levels = static_cast<int32_t>(ilu.L.ptr.size() + ilu.U.ptr.size()) - 2;
        ilu.factor(n, d_p.as<int32_t>(), d_i.as<int32_t>(), d_v.as<double>(), nullptr, nnz, nullptr, nullptr);
        ilu.apply(d_r.as<double2>(), d_z.as<double2>(), nullptr, false);   // warm-up
        HIPCHK(hipDeviceSynchronize());
        hipEvent_t e0, e1;
        HIPCHK(hipEventCreate(&e0));
        HIPCHK(hipEventCreate(&e1));
        for (int q = 0; q < repeats; ++q) {
            HIPCHK(hipEventRecord(e0, nullptr));
            ilu.apply(d_r.as<double2>(), d_z.as<double2>(), nullptr, false);
            HIPCHK(hipEventRecord(e1, nullptr));
            HIPCHK(hipEventSynchronize(e1));
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, e0, e1));
            ms_out[q] = ms;
        }
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        return TM_OK;
    });
}
// the double-double residual kernel (which != 0: k_csr_residual_dd) or the fp64 one it is measured against (0: k_csr_apply<true, DOT_NONE>) on a
// caller-assembled system, both components, an event pair per repeat after a warm-up (tools/refine_timing.py); ms_out[repeats]
int tm_debug_csr_residual_ms(uint64_t n64, const int32_t* Ap, const int32_t* Ai, const double* Ax, int which, int repeats, double* ms_out) {
    return guarded([&]() {
        if (!Ap || !Ai || !Ax || !ms_out || repeats < 1) throw TmError(TM_E_ARG, "null argument");
        if (n64 == 0 || n64 >= (uint64_t{1} << 31)) throw TmError(TM_E_SIZE, "system size out of range");
        require_gfx950();
        const int n = static_cast<int>(n64);
        const size_t nnz = static_cast<size_t>(Ap[n]);
        for (size_t k = 0; k < nnz; ++k)
            if (Ai[k] < 0 || Ai[k] >= n) throw TmError(TM_E_ARG, "InvalidMatrix: column index out of range");
        const size_t vb = sizeof(double2) * static_cast<size_t>(n);
        DevBuf d_p(sizeof(int32_t) * (static_cast<size_t>(n) + 1), "csr p"), d_i(sizeof(int32_t) * nnz, "csr i"), d_v(sizeof(double) * nnz, "csr v"), d_x(vb, "csr x"), d_b(vb, "csr b"), d_r(vb, "csr r"), d_dinv(vb, "csr dinv");
        HIPCHK(hipMemcpy(d_p.p, Ap, sizeof(int32_t) * (static_cast<size_t>(n) + 1), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_i.p, Ai, sizeof(int32_t) * nnz, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_v.p, Ax, sizeof(double) * nnz, hipMemcpyHostToDevice));
        std::vector<double2> w(static_cast<size_t>(n));
        for (int k = 0; k < n; ++k) w[k] = make_double2(1.0 + 1e-3 * (k % 97), 1.0 - 1e-3 * (k % 89));
        HIPCHK(hipMemcpy(d_x.p, w.data(), vb, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_b.p, w.data(), vb, hipMemcpyHostToDevice));
        HIPCHK(launch_csr_dinv(n, d_p.as<int32_t>(), d_i.as<int32_t>(), d_v.as<double>(), d_v.as<double>(), d_dinv.as<double2>(), nullptr));
        auto run = [&]() {
            if (which)
                HIPCHK(launch_csr_residual_dd(n, d_p.as<int32_t>(), d_i.as<int32_t>(), d_v.as<double>(), d_v.as<double>(), d_x.as<double2>(), d_b.as<double2>(),
                                              d_r.as<double2>(), nullptr));
            else
                HIPCHK(launch_csr_scaled_residual_plain(n, d_p.as<int32_t>(), d_i.as<int32_t>(), d_v.as<double>(), d_v.as<double>(), d_dinv.as<double2>(), d_x.as<double2>(),
                                                        d_b.as<double2>(), d_r.as<double2>(), nullptr));
        };
        run();   // warm-up
        HIPCHK(hipDeviceSynchronize());
        hipEvent_t e0, e1;
        HIPCHK(hipEventCreate(&e0));
        HIPCHK(hipEventCreate(&e1));
        for (int q = 0; q < repeats; ++q) {
            HIPCHK(hipEventRecord(e0, nullptr));
            run();
            HIPCHK(hipEventRecord(e1, nullptr));
            HIPCHK(hipEventSynchronize(e1));
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, e0, e1));
            ms_out[q] = ms;
        }
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        return TM_OK;
    });
}
// internal tuning knob used by the benchmark sweeps (not part of the drop-in surface)
int tm_tune_apply(int rows_per_chunk, int unroll, int pipe, int nt) {
    tune_apply(rows_per_chunk, unroll, pipe, nt);
    return TM_OK;
}

int tm_tune_fuse(int rows_per_chunk) {
    tune_fuse_rows(rows_per_chunk);
    return TM_OK;
}
// diagnostic: K2 with the same tiling / data movement but reduced arithmetic (mode 4 = copy, 5 = 9-point sum)
int tm_diag_apply(const double* d_in, double* d_out, uint64_t ni, uint64_t nj, int mode, void* stream) {
    return guarded([&]() {
        ApplyBlock a;
        a.in = reinterpret_cast<const double2*>(d_in);
        a.xk = a.in;
        a.pq = nullptr;
        a.aux = nullptr;
        a.out = reinterpret_cast<double2*>(d_out);
        a.ni = static_cast<int>(ni);
        a.nj = static_cast<int>(nj);
        a.omega = 1.0;
        a.partials = nullptr;
        HIPCHK(launch_apply_block(a, mode, DOT_NONE, static_cast<hipStream_t>(stream)));
        return TM_OK;
    });
}
#endif   // TM_DEBUG_EXPORTS

// ------------------------------------------------------------------ TFI (tfi.zig:112-208)
// diagnostic (include/tm_hip_diag.h): what this GPU sustains on a plain copy / triad of `bytes` per array, vector-kernel access pattern.
// Runs on a private non-blocking stream (the legacy null stream would synchronise with every blocking stream of the process, and a
// multi-rank job calls this on rank 0 while the other ranks move on); stream and events are released on every path.
namespace {
struct ProbeStream {
    hipStream_t s = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ProbeStream() {
        HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        HIPCHK(hipEventCreate(&e0));
        HIPCHK(hipEventCreate(&e1));
    }
    ~ProbeStream() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        if (s) {
            (void)hipStreamSynchronize(s);
            (void)hipStreamDestroy(s);
        }
    }
    ProbeStream(const ProbeStream&) = delete;
    ProbeStream& operator=(const ProbeStream&) = delete;
};
}  // namespace
int tm_stream_probe(uint64_t bytes, int32_t iters, double* copy_GBps, double* triad_GBps) {
    return guarded([&]() {
        if (bytes < 4096 || iters < 1 || !copy_GBps || !triad_GBps) throw TmError(TM_E_ARG, "bad argument");
        require_gfx950();
        const int64_t n = static_cast<int64_t>(bytes / sizeof(double2));
        DevBuf a(sizeof(double2) * n, "entry point a"), b(sizeof(double2) * n, "entry point b"), c(sizeof(double2) * n, "entry point c");
        ProbeStream ps;
        HIPCHK(hipMemsetAsync(a.p, 0, sizeof(double2) * n, ps.s));
        HIPCHK(hipMemsetAsync(b.p, 0, sizeof(double2) * n, ps.s));
        HIPCHK(hipMemsetAsync(c.p, 0, sizeof(double2) * n, ps.s));
        double out[2] = {0.0, 0.0};
        for (int kind = 0; kind < 2; ++kind) {
            // the direction alternates (a <- b, b <- a, ...), like the two fields of a relaxation sweep: a source that no launch ever writes
            // would be served from the 256 MB Infinity Cache and read as "8.5 TB/s" (tools/ubench/stream.hip)
            auto once = [&](int k) {
                double2* v[3] = {a.as<double2>(), b.as<double2>(), c.as<double2>()};
                if (kind == 0) return launch_stream(0, v[k & 1], v[(k & 1) ^ 1], v[2], 0.5, n, ps.s);
                return launch_stream(1, v[k % 3], v[(k + 1) % 3], v[(k + 2) % 3], 0.5, n, ps.s);   // the three arrays rotate
            };
            for (int w = 0; w < 4; ++w) HIPCHK(once(w));
            HIPCHK(hipEventRecord(ps.e0, ps.s));
            for (int k = 0; k < iters; ++k) HIPCHK(once(k));
            HIPCHK(hipEventRecord(ps.e1, ps.s));
            HIPCHK(hipEventSynchronize(ps.e1));
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, ps.e0, ps.e1));
            out[kind] = static_cast<double>(kind == 1 ? 3 : 2) * sizeof(double2) * n * iters / (1e-3 * ms) / 1e9;
        }
        *copy_GBps = out[0];
        *triad_GBps = out[1];
        return TM_OK;
    });
}

// diagnostic (include/tm_hip_diag.h, tests/test_gpu_refmath.py): acos(x[i]) and atan2(y[i], x[i]) as the device's White kernels evaluate
// them (tm_refmath.h), host arrays in and out
int tm_white_math_probe(const double* x, const double* y, uint64_t n, double* out_acos, double* out_atan2) {
    return guarded([&]() {
        if (!x || !y || !out_acos || !out_atan2) throw TmError(TM_E_ARG, "null argument");
        require_gfx950();
        const size_t nb = sizeof(double) * n;
        DevBuf dx(nb, "entry point dx"), dy(nb, "entry point dy"), da(nb, "entry point da"), dt(nb, "entry point dt");
        HIPCHK(hipMemcpy(dx.p, x, nb, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(dy.p, y, nb, hipMemcpyHostToDevice));
        HIPCHK(launch_debug_white_math(dx.as<double>(), dy.as<double>(), n, da.as<double>(), dt.as<double>(), nullptr));
        HIPCHK(hipMemcpy(out_acos, da.p, nb, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(out_atan2, dt.p, nb, hipMemcpyDeviceToHost));
        return TM_OK;
    });
}

// diagnostic (include/tm_hip_diag.h, tests/test_gpu_mg_operator.py): one stand-alone multigrid transfer kernel on host arrays, through the
// launch_mg_* functions the cycle uses
int tm_mg_transfer_probe(int32_t kind, uint64_t nif64, uint64_t njf64, int32_t ci, int32_t cj, const double* in, const double* x_coarse, double scale_x,
                         double scale_y, double* out) {
    return guarded([&]() {
        if (!in || !out || (kind == 1 && !x_coarse)) throw TmError(TM_E_ARG, "null argument");
        if (kind < 0 || kind > 3) throw TmError(TM_E_ARG, "kind must be 0 (inject), 1 (restrict), 2 (prolong-add) or 3 (scale)");
        if (nif64 < 3 || njf64 < 3 || nif64 * njf64 >= (uint64_t{1} << 31)) throw TmError(TM_E_SIZE, "a level needs at least 3 x 3 nodes (and fewer than 2^31)");
        require_gfx950();
        MgPair g;
        g.nif = static_cast<int>(nif64);
        g.njf = static_cast<int>(njf64);
        g.ci = (kind != 3 && ci) ? 1 : 0;
        g.cj = (kind != 3 && cj) ? 1 : 0;
        g.nic = g.ci ? g.nif / 2 + 1 : g.nif;
        g.njc = g.cj ? g.njf / 2 + 1 : g.njf;
        const size_t nf = sizeof(double2) * static_cast<size_t>(g.nif) * g.njf, nc = sizeof(double2) * static_cast<size_t>(g.nic) * g.njc;
        const bool in_fine = kind != 2, out_fine = kind >= 2;
        DevBuf din(in_fine ? nf : nc, "entry point din"), dout(out_fine ? nf : nc, "entry point dout"), dx(kind == 1 ? nc : 0, "entry point dx");
        HIPCHK(hipMemcpy(din.p, in, in_fine ? nf : nc, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(dout.p, out, out_fine ? nf : nc, hipMemcpyHostToDevice));   // (what a kernel leaves alone comes back as it went in)
        if (kind == 1) HIPCHK(hipMemcpy(dx.p, x_coarse, nc, hipMemcpyHostToDevice));
        if (kind == 0) HIPCHK(launch_mg_inject(din.as<double2>(), dout.as<double2>(), g, scale_x, scale_y, nullptr));
        else if (kind == 1) HIPCHK(launch_mg_restrict(din.as<double2>(), dx.as<double2>(), dout.as<double2>(), g, nullptr));
        else if (kind == 2) HIPCHK(launch_mg_prolong_add(din.as<double2>(), dout.as<double2>(), g, nullptr));
        else HIPCHK(launch_mg_scale(din.as<double2>(), dout.as<double2>(), g.nif, g.njf, scale_x, nullptr));
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(out, dout.p, out_fine ? nf : nc, hipMemcpyDeviceToHost));
        return TM_OK;
    });
}

int tm_tfi_block(double* xy_out, uint64_t ni, uint64_t nj, const double* x_i_min, const double* x_i_max, const double* x_j_min,
                 const double* x_j_max, const double* s1, const double* s2, const double* t1, const double* t2) {
    return guarded([&]() {
        if (!xy_out || !x_i_min || !x_i_max || !x_j_min || !x_j_max || !s1 || !s2 || !t1 || !t2) throw TmError(TM_E_ARG, "null argument");
        if (ni < 2 || nj < 2 || ni * nj >= (uint64_t{1} << 31)) throw TmError(TM_E_SIZE, "InconsistentSize: block must be at least 2 x 2 and below 2^31 nodes");
        // the reference's debug asserts (tfi.zig:135-162) become error codes
        if (s1[0] != 0 || s1[ni - 1] != 1.0 || s2[0] != 0 || s2[ni - 1] != 1.0 || t1[0] != 0 || t1[nj - 1] != 1.0 || t2[0] != 0 ||
            t2[nj - 1] != 1.0)
            throw TmError(TM_E_ARG, "clusterings must start at 0 and end at exactly 1 (tfi.zig:135-145)");
        const double tol = 1e-10;
        if (!close2(x_i_min, x_j_min, tol) || !close2(x_i_min + 2 * (ni - 1), x_j_max, tol) || !close2(x_j_min + 2 * (nj - 1), x_i_max, tol) ||
            !close2(x_i_max + 2 * (ni - 1), x_j_max + 2 * (nj - 1), tol))
            throw TmError(TM_E_MISMATCH, "edge end points do not meet at the block corners (tfi.zig:150-162)");
        require_gfx950();
        const size_t ei = sizeof(double) * 2 * ni, ej = sizeof(double) * 2 * nj;
        DevBuf out(sizeof(double) * 2 * ni * nj, "entry point out"), a(ei, "entry point a"), b(ei, "entry point b"), c(ej, "entry point c"), d(ej, "entry point d"), ds1(ei / 2, "entry point ds1"), ds2(ei / 2, "entry point ds2"), dt1(ej / 2, "entry point dt1"), dt2(ej / 2, "entry point dt2");
        HIPCHK(hipMemcpy(a.p, x_i_min, ei, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(b.p, x_i_max, ei, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(c.p, x_j_min, ej, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d.p, x_j_max, ej, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(ds1.p, s1, ei / 2, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(ds2.p, s2, ei / 2, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(dt1.p, t1, ej / 2, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(dt2.p, t2, ej / 2, hipMemcpyHostToDevice));
        HIPCHK(launch_tfi_block(out.as<double2>(), static_cast<int>(ni), static_cast<int>(nj), a.as<double2>(), b.as<double2>(), c.as<double2>(),
                                d.as<double2>(), ds1.as<double>(), ds2.as<double>(), dt1.as<double>(), dt2.as<double>(), nullptr));
        HIPCHK(hipMemcpy(xy_out, out.p, sizeof(double) * 2 * ni * nj, hipMemcpyDeviceToHost));
        return TM_OK;
    });
}

int tm_tfi_linear2d(double* xy_out, uint64_t ni, uint64_t nj, const double* e_i_min, const double* e_i_max, const double* e_j_min,
                    const double* e_j_max) {
    return guarded([&]() {
        if (!xy_out || !e_i_min || !e_i_max || !e_j_min || !e_j_max) throw TmError(TM_E_ARG, "null argument");
        if (ni < 2 || nj < 2 || ni * nj >= (uint64_t{1} << 31)) throw TmError(TM_E_SIZE, "InconsistentSize (tfi.zig:30)");
        require_gfx950();
        const size_t ei = sizeof(double) * 2 * ni, ej = sizeof(double) * 2 * nj;
        DevBuf out(sizeof(double) * 2 * ni * nj, "entry point out"), a(ei, "entry point a"), b(ei, "entry point b"), c(ej, "entry point c"), d(ej, "entry point d");
        HIPCHK(hipMemcpy(a.p, e_i_min, ei, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(b.p, e_i_max, ei, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(c.p, e_j_min, ej, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d.p, e_j_max, ej, hipMemcpyHostToDevice));
        HIPCHK(launch_tfi_linear2d(out.as<double2>(), static_cast<int>(ni), static_cast<int>(nj), a.as<double2>(), b.as<double2>(), c.as<double2>(),
                                   d.as<double2>(), nullptr));
        HIPCHK(hipMemcpy(xy_out, out.p, sizeof(double) * 2 * ni * nj, hipMemcpyDeviceToHost));
        return TM_OK;
    });
}

int tm_dev_tfi_block(double* d_xy, uint64_t ni, uint64_t nj, const double* a, const double* b, const double* c, const double* d,
                     const double* s1, const double* s2, const double* t1, const double* t2, void* stream) {
    return guarded([&]() {
        if (ni < 2 || nj < 2 || ni * nj >= (uint64_t{1} << 31)) throw TmError(TM_E_SIZE, "InconsistentSize");
        HIPCHK(launch_tfi_block(reinterpret_cast<double2*>(d_xy), static_cast<int>(ni), static_cast<int>(nj), reinterpret_cast<const double2*>(a),
                                reinterpret_cast<const double2*>(b), reinterpret_cast<const double2*>(c), reinterpret_cast<const double2*>(d), s1, s2,
                                t1, t2, static_cast<hipStream_t>(stream)));
        return TM_OK;
    });
}

uint64_t tm_dev_relax_partials_needed(uint64_t ni, uint64_t nj) {
    if (ni < 3 || nj < 3) return 0;
    return static_cast<uint64_t>(apply_block_nwg(static_cast<int>(ni), static_cast<int>(nj))) * MAX_PARTIALS;
}

int tm_dev_relax_sweep(const double* d_in, double* d_out, uint64_t ni, uint64_t nj, double omega, double* d_partials,
                       uint64_t partials_capacity, uint64_t* nwg, void* stream) {
    return guarded([&]() {
        if (ni < 3 || nj < 3 || ni * nj >= (uint64_t{1} << 31)) throw TmError(TM_E_SIZE, "block must be at least 3 x 3");
        if (d_in == d_out) throw TmError(TM_E_ARG, "a Jacobi sweep cannot run in place");
        const uint64_t need = tm_dev_relax_partials_needed(ni, nj);
        if (d_partials && partials_capacity < need) throw TmError(TM_E_ARG, "partials buffer too small");
        ApplyBlock a;
        a.in = reinterpret_cast<const double2*>(d_in);
        a.xk = a.in;
        a.pq = nullptr;
        a.aux = nullptr;
        a.out = reinterpret_cast<double2*>(d_out);
        a.ni = static_cast<int>(ni);
        a.nj = static_cast<int>(nj);
        a.omega = omega;
        a.partials = d_partials;
        hipStream_t st = static_cast<hipStream_t>(stream);
        HIPCHK(launch_apply_block(a, MODE_RELAX, d_partials ? DOT_DELTA : DOT_NONE, st));
        HIPCHK(launch_copy_perimeter(a.in, a.out, a.ni, a.nj, st));
        if (nwg) *nwg = need / MAX_PARTIALS;
        return TM_OK;
    });
}

// ------------------------------------------------------------------ handle
int tm_smoother_create(const tm_mesh_desc* mesh, const tm_solver_opt* opt, const tm_control_fn* cf, const tm_comm_hooks* hooks, void* stream,
                       tm_smoother** out) {
    return guarded([&]() {
        if (!out) throw TmError(TM_E_ARG, "null output handle");
        *out = nullptr;
        require_gfx950();
        auto h = std::make_unique<tm_smoother>();
        h->impl.create(mesh, opt, cf, hooks, stream, false);
        *out = h.release();
        {
            std::lock_guard<std::mutex> lock(g_live_mutex);
            g_live_handles.insert(*out);
        }
        return TM_OK;
    });
}
int tm_smoother_workspace_bytes(const tm_mesh_desc* mesh, const tm_solver_opt* opt, const tm_control_fn* cf, const tm_comm_hooks* hooks,
                                uint64_t* bytes) {
    return guarded([&]() {
        if (!bytes) throw TmError(TM_E_ARG, "null output");
        tm_smoother tmp;
        tmp.impl.create(mesh, opt, cf, hooks, nullptr, true);
        *bytes = tmp.impl.arena.used() + 4096;
        return TM_OK;
    });
}
void tm_smoother_destroy(tm_smoother* s) {
    {
        std::lock_guard<std::mutex> lock(g_live_mutex);
        g_live_handles.erase(s);
    }
    delete s;   // ~Smoother releases the pinned buffers, events, side stream and scratch
}
int tm_smoother_iterate(tm_smoother* s, uint64_t iterations, tm_stats* stats) {
    return guarded([&]() {
        if (!s) throw TmError(TM_E_ARG, "null handle");
        tm_stats st;
        s->impl.iterate(iterations, &st);
        if (stats) *stats = st;
        return st.not_converged ? TM_W_NOT_CONVERGED : TM_OK;
    });
}
int tm_smoother_iterate_until(tm_smoother* s, uint64_t max_iterations, double scaled_residual_tol, tm_stats* stats) {
    return guarded([&]() {
        if (!s) throw TmError(TM_E_ARG, "null handle");
        if (!(scaled_residual_tol > 0.0)) throw TmError(TM_E_ARG, "the residual tolerance must be positive");
        tm_stats st;
        const bool reached = s->impl.iterate_until(max_iterations, scaled_residual_tol, &st);
        if (stats) *stats = st;
        return (reached && !st.not_converged) ? TM_OK : TM_W_NOT_CONVERGED;
    });
}
int tm_smoother_iterate_until_update(tm_smoother* s, uint64_t max_iterations, double update_rms_tol, tm_stats* stats) {
    return guarded([&]() {
        if (!s) throw TmError(TM_E_ARG, "null handle");
        if (!(update_rms_tol > 0.0)) throw TmError(TM_E_ARG, "the update tolerance must be positive");
        tm_stats st;
        const bool reached = s->impl.iterate_until_update(max_iterations, update_rms_tol, &st);
        if (stats) *stats = st;
        return (reached && !st.not_converged) ? TM_OK : TM_W_NOT_CONVERGED;
    });
}
int tm_smoother_download(tm_smoother* s, const tm_mesh_desc* mesh) {
    return guarded([&]() {
        if (!s) throw TmError(TM_E_ARG, "null handle");
        s->impl.download(mesh);
        return TM_OK;
    });
}
int tm_smoother_upload(tm_smoother* s, const tm_mesh_desc* mesh) {
    return guarded([&]() {
        if (!s) throw TmError(TM_E_ARG, "null handle");
        s->impl.upload(mesh);
        s->impl.outer_done = 0;
        if (s->impl.white) {
            HIPCHK(hipMemsetAsync(s->impl.PQ, 0, sizeof(double2) * s->impl.n_local, s->impl.stream));
            s->impl.white_launch(0);
            s->impl.sync();
        }
        if (s->impl.thomas_middlecoff()) {   // the field belongs to the coordinates it was evaluated from
            s->impl.tm_field_launch();
            s->impl.sync();
        }
        return TM_OK;
    });
}
int tm_smoother_set_control_function(tm_smoother* s, const double* pq) {
    return guarded([&]() {
        if (!s || !pq) throw TmError(TM_E_ARG, "null argument");
        s->impl.set_control_function_host(pq);
        return TM_OK;
    });
}
int tm_smoother_update_control_function(tm_smoother* s) {
    return guarded([&]() {
        if (!s) throw TmError(TM_E_ARG, "null handle");
        s->impl.update_control_function();
        return TM_OK;
    });
}
int tm_smoother_exchange_plan(const tm_smoother* s, int32_t* npeers, const int32_t** peer_rank, const int64_t** send_offset,
                              const int64_t** send_count, const int64_t** recv_offset, const int64_t** recv_count) {
    return guarded([&]() {
        if (!s || !npeers) throw TmError(TM_E_ARG, "null argument");
        const LocalPlan& lp = s->impl.lp;
        *npeers = static_cast<int32_t>(lp.peer_rank.size());
        if (peer_rank) *peer_rank = lp.peer_rank.data();
        if (send_offset) *send_offset = lp.direct_send ? lp.send_first.data() : lp.send_off.data();
        if (send_count) *send_count = lp.send_cnt.data();
        if (recv_offset) *recv_offset = lp.recv_off.data();
        if (recv_count) *recv_count = lp.recv_cnt.data();
        return TM_OK;
    });
}
int tm_smoother_apply(tm_smoother* s, const double* in_xy, double* out_xy, int scaled) {
    return guarded([&]() {
        if (!s || !in_xy || !out_xy) throw TmError(TM_E_ARG, "null argument");
        s->impl.apply_host(in_xy, out_xy, scaled);
        return TM_OK;
    });
}
int tm_smoother_assemble_csr(tm_smoother* s, int32_t* Ap, int32_t* Ai, double* Ax_x, double* Ax_y, uint64_t nnz_capacity, uint64_t* nnz) {
    return guarded([&]() {
        if (!s) throw TmError(TM_E_ARG, "null handle");
        const uint64_t n = s->impl.assemble_csr_host(Ap, Ai, Ax_x, Ax_y, nnz_capacity);
        if (nnz) *nnz = n;
        return TM_OK;
    });
}
int tm_smoother_apply_reference_order(tm_smoother* s, const double* in_xy, double* out_xy) {
    return guarded([&]() {
        if (!s || !in_xy || !out_xy) throw TmError(TM_E_ARG, "null argument");
        s->impl.apply_reference_host(in_xy, out_xy);
        return TM_OK;
    });
}
int tm_smoother_rhs(tm_smoother* s, double* rhs_xy) {
    return guarded([&]() {
        if (!s || !rhs_xy) throw TmError(TM_E_ARG, "null argument");
        s->impl.rhs_host(rhs_xy);
        return TM_OK;
    });
}
int tm_smoother_residual(tm_smoother* s, const double* xy, double* r_xy) {
    return guarded([&]() {
        if (!s || !r_xy) throw TmError(TM_E_ARG, "null argument");
        s->impl.residual_host(xy, r_xy);
        return TM_OK;
    });
}
int tm_smoother_refine_report(const tm_smoother* s, uint32_t* steps_x_y, double* last_update_rel, uint64_t* correction_iterations) {
    return guarded([&]() {
        if (!s) throw TmError(TM_E_ARG, "null handle");
        if (!s->impl.refine()) throw TmError(TM_E_UNSUPPORTED, "the handle was created without TM_OPT_REFINE");
        for (int c = 0; c < 2; ++c) {
            if (steps_x_y) steps_x_y[c] = s->impl.refine_steps;
            if (last_update_rel) last_update_rel[c] = s->impl.refine_rel[c];
        }
        if (correction_iterations) *correction_iterations = s->impl.refine_iterations;
        return TM_OK;
    });
}
int tm_smoother_row_kinds(const tm_smoother* s, int32_t* kinds) {
    return guarded([&]() {
        if (!s || !kinds) throw TmError(TM_E_ARG, "null argument");
        for (int64_t i = 0; i < s->impl.topo.dof; ++i) kinds[i] = -1;
        for (const PlanRow& r : s->impl.all_rows) kinds[r.gid] = r.kind;
        return TM_OK;
    });
}
uint64_t tm_smoother_dof(const tm_smoother* s) { return s ? static_cast<uint64_t>(s->impl.topo.dof) : 0; }
int tm_smoother_control_function(tm_smoother* s, double* pq) {
    return guarded([&]() {
        if (!s || !pq) throw TmError(TM_E_ARG, "null argument");
        s->impl.control_function_host(pq);
        return TM_OK;
    });
}

int tm_smoother_export_soa(tm_smoother* s, uint64_t block, double* x, double* y, double* p, double* q) {
    return guarded([&]() {
        if (!s || !x || !y || ((p == nullptr) != (q == nullptr))) throw TmError(TM_E_ARG, "null argument (p and q come together)");
        s->impl.export_soa_host(static_cast<int64_t>(block), x, y, p, q);
        return TM_OK;
    });
}

int tm_export_soa(const double* xy, uint64_t ni, uint64_t nj, double* x_out, double* y_out) {
    return guarded([&]() {
        if (!xy || !x_out || !y_out) throw TmError(TM_E_ARG, "null argument");
        if (ni < 1 || nj < 1 || ni * nj >= (uint64_t{1} << 31)) throw TmError(TM_E_SIZE, "block size out of range");
        require_gfx950();
        const size_t n = static_cast<size_t>(ni) * nj;
        DevBuf in(sizeof(double) * 2 * n, "entry point in"), out(sizeof(double) * 2 * n, "entry point out");
        HIPCHK(hipMemcpy(in.p, xy, sizeof(double) * 2 * n, hipMemcpyHostToDevice));
        HIPCHK(launch_soa_planes(in.as<double2>(), out.as<double>(), out.as<double>() + n, static_cast<int>(ni), static_cast<int>(nj), nullptr));
        HIPCHK(hipMemcpy(x_out, out.p, sizeof(double) * n, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(y_out, out.as<double>() + n, sizeof(double) * n, hipMemcpyDeviceToHost));
        return TM_OK;
    });
}

// ------------------------------------------------------------------ mesh quality (tm_quality.hip; tm_mesh_quality_host: tm_quality_host.cpp)
int tm_mesh_quality(const tm_mesh_desc* mesh, tm_quality* per_block, tm_quality* total) {
    return guarded([&]() {
        if (!mesh || !mesh->blocks || mesh->nblocks == 0) throw TmError(TM_E_ARG, "mesh description without blocks");
        size_t bytes = 0;
        for (uint64_t b = 0; b < mesh->nblocks; ++b) {
            const tm_block& k = mesh->blocks[b];
            if (!k.xy) throw TmError(TM_E_ARG, "block without coordinates");
            if (k.ni < 2 || k.nj < 2 || k.ni * k.nj >= (uint64_t{1} << 31)) throw TmError(TM_E_SIZE, "InconsistentSize: a block needs at least 2 x 2 nodes (and fewer than 2^31)");
            bytes += sizeof(double2) * k.ni * k.nj;
        }
        require_gfx950();
        DevBuf xy(bytes, "entry point xy");
        std::vector<QualityBlock> blocks;
        size_t off = 0;
        for (uint64_t b = 0; b < mesh->nblocks; ++b) {
            const tm_block& k = mesh->blocks[b];
            HIPCHK(hipMemcpy(xy.as<double2>() + off, k.xy, sizeof(double2) * k.ni * k.nj, hipMemcpyHostToDevice));
            blocks.push_back(QualityBlock{xy.as<double2>() + off, static_cast<int>(k.ni), static_cast<int>(k.nj), b});
            off += k.ni * k.nj;
        }
        QualityDev dev;
        std::vector<tm_quality> rec(blocks.size());
        dev.run(blocks, nullptr, rec.data());
        if (per_block) std::memcpy(per_block, rec.data(), sizeof(tm_quality) * rec.size());
        if (total) quality_total(rec.data(), rec.size(), total);
        return TM_OK;
    });
}
int tm_smoother_quality(tm_smoother* s, tm_quality* per_block, tm_quality* total) {
    return guarded([&]() {
        if (!s) throw TmError(TM_E_ARG, "null handle");
        s->impl.quality_host(per_block, total);
        return TM_OK;
    });
}
int tm_smoother_quality_field(tm_smoother* s, uint64_t block, double* min_scaled_jacobian) {
    return guarded([&]() {
        if (!s || !min_scaled_jacobian) throw TmError(TM_E_ARG, "null argument");
        s->impl.quality_field_host(static_cast<int64_t>(block), min_scaled_jacobian);
        return TM_OK;
    });
}

int tm_smoother_profile(tm_smoother* s, int enable) {
    return guarded([&]() {
        if (!s) throw TmError(TM_E_ARG, "null handle");
        s->impl.profile = enable > 0 ? enable : 0;
        s->impl.ev_used = 0;
        s->impl.prof_launches = 0;
        s->impl.prof_timed = 0;
        s->impl.prof_phase = 0;
        s->impl.prof_open = 0;
        return TM_OK;
    });
}
int tm_smoother_profile_read(tm_smoother* s, double* k2_ms_total, uint64_t* k2_launches_timed, uint64_t* k2_launches) {
    return guarded([&]() {
        if (!s) throw TmError(TM_E_ARG, "null handle");
        s->impl.profile_read(k2_ms_total, k2_launches, k2_launches_timed);
        return TM_OK;
    });
}

int tm_smoother_inner(const tm_smoother* s) { return s ? s->impl.opt.inner : static_cast<int>(TM_E_ARG); }
int tm_smoother_inner_counts(const tm_smoother* s, uint64_t* x_iterations, uint64_t* y_iterations) {
    return guarded([&]() {
        if (!s || !x_iterations || !y_iterations) throw TmError(TM_E_ARG, "null argument");
        *x_iterations = s->impl.inner_counts[0];
        *y_iterations = s->impl.inner_counts[1];
        return TM_OK;
    });
}

// the multigrid preconditioner as an operator (include/tm_hip_diag.h)
int tm_smoother_mg_levels(const tm_smoother* s, uint64_t block, int32_t* nlevels, int32_t* shape, uint32_t capacity, int32_t* cycle, double* omega) {
    return guarded([&]() {
        if (!s || !nlevels) throw TmError(TM_E_ARG, "null argument");
        const Smoother& m = s->impl;
        if (!m.use_mg) throw TmError(TM_E_UNSUPPORTED, "tm_smoother_mg_levels needs a handle created with TM_INNER_MG_BICGSTAB");
        const auto it = std::lower_bound(m.lp.owned_blocks.begin(), m.lp.owned_blocks.end(), static_cast<int64_t>(block));
        if (it == m.lp.owned_blocks.end() || *it != static_cast<int64_t>(block)) throw TmError(TM_E_ARG, "block is not owned by this rank");
        const BlockMG& h = m.mg[static_cast<size_t>(it - m.lp.owned_blocks.begin())];
        const std::vector<MgLevel>& L = h.levels();
        *nlevels = static_cast<int32_t>(L.size());
        for (size_t l = 0; shape && l < L.size() && l < capacity; ++l) {
            shape[4 * l + 0] = L[l].ni;
            shape[4 * l + 1] = L[l].nj;
            shape[4 * l + 2] = L[l].ci;
            shape[4 * l + 3] = L[l].cj;
        }
        if (cycle) {
            cycle[0] = h.nu_pre;
            cycle[1] = h.nu_post;
            cycle[2] = h.nu_coarsest;
            cycle[3] = m.mg_dirichlet ? 1 : 0;
            cycle[4] = m.mg_perimeter_step ? 1 : 0;
            cycle[5] = m.mg_perimeter_sweeps;
        }
        if (omega) *omega = h.omega;
        return TM_OK;
    });
}
int tm_smoother_precondition_probe(tm_smoother* s, const double* f, double* z, double* f_after) {
    return guarded([&]() {
        if (!s || !f || !z) throw TmError(TM_E_ARG, "null argument");
        s->impl.precondition_probe_host(f, z, f_after);
        return TM_OK;
    });
}

// how the handle orders the two queues of a pipelined pass (include/tm_hip_diag.h)
int tm_smoother_queue_ordering(const tm_smoother* s) { return s ? s->impl.queue_ordering : static_cast<int>(TM_E_ARG); }

// ------------------------------------------------------------------ seam 1 (smooth.zig:74-80)
int tm_smooth_mesh(const tm_mesh_desc* mesh, uint64_t iterations, const tm_solver_opt* opt, const tm_control_fn* cf, tm_stats* stats) {
    tm_smoother* h = nullptr;
    if (cf && cf->kind == TM_CF_PRESCRIBED)   // a one-shot call has no way to pass the field: the handle API has tm_smoother_set_control_function
        return guarded([&]() -> int { throw TmError(TM_E_ARG, "tm_smooth_mesh cannot take a prescribed control function: use a handle and tm_smoother_set_control_function"); });
    int rc = tm_smoother_create(mesh, opt, cf, nullptr, nullptr, &h);
    if (rc < 0) return rc;
    tm_stats st;
    std::memset(&st, 0, sizeof(st));
    rc = tm_smoother_iterate(h, iterations, &st);
    if (rc >= 0 && iterations > 0) {   // iterations == 0 returns the mesh untouched (input.zig:28 default)
        const int rd = tm_smoother_download(h, mesh);
        if (rd < 0) rc = rd;
    }
    tm_smoother_destroy(h);
    if (stats) *stats = st;
    return rc;
}

// ------------------------------------------------------------------ host-only planning export
int tm_plan_local(const tm_mesh_desc* mesh, const int32_t* owner, int32_t rank, int32_t nranks, tm_plan_local_info* out) {
    return guarded([&]() {
        if (!mesh || !owner || !out) throw TmError(TM_E_ARG, "null argument");
        std::memset(out, 0, sizeof(*out));
        const Topology t = topo_of(mesh);
        const std::vector<PlanRow> rows = build_rows(t);
        const std::vector<int32_t> own(owner, owner + t.nblocks());
        const LocalPlan lp = build_local_plan(t, rows, own, rank, nranks);
        out->n_owned = lp.n_owned;
        out->n_ghost = static_cast<int64_t>(lp.ghost_gid.size());
        out->n_send = static_cast<int64_t>(lp.send_ids.size());
        out->npeers = static_cast<int32_t>(lp.peer_rank.size());
        out->nowned_blocks = static_cast<int32_t>(lp.owned_blocks.size());
        std::vector<int64_t> send_gid;
        for (int32_t l : lp.send_ids) {
            size_t k = lp.owned_blocks.size() - 1;
            while (l < lp.local_start[k]) --k;
            send_gid.push_back(t.start[lp.owned_blocks[k]] + (l - lp.local_start[k]));
        }
        out->owned_blocks = dup(lp.owned_blocks);
        out->local_start = dup(lp.local_start);
        out->ghost_gid = dup(lp.ghost_gid);
        out->send_ids = dup(lp.send_ids);
        out->send_gid = dup(send_gid);
        out->peer_rank = dup(lp.peer_rank);
        out->send_offset = dup(lp.send_off);
        out->send_count = dup(lp.send_cnt);
        out->recv_offset = dup(lp.recv_off);
        out->recv_count = dup(lp.recv_cnt);
        out->send_first = dup(lp.send_first);
        out->direct_send = lp.direct_send ? 1 : 0;
        std::vector<int64_t> gg, gc;
        std::vector<int32_t> gk;
        for (const PlanRow& g : lp.ghost_rows) {
            gg.push_back(g.gid);
            gk.push_back(g.kind);
            for (int q = 0; q < 9; ++q) gc.push_back(q < g.ncols ? g.col[q] : -1);
        }
        out->n_ghost_rows = static_cast<int64_t>(gg.size());
        out->ghost_row_gid = dup(gg);
        out->ghost_row_kind = dup(gk);
        out->ghost_row_cols = dup(gc);
        return TM_OK;
    });
}
void tm_plan_local_free(tm_plan_local_info* i) {
    if (!i) return;
    std::free(i->owned_blocks);
    std::free(i->local_start);
    std::free(i->ghost_gid);
    std::free(i->send_ids);
    std::free(i->send_gid);
    std::free(i->peer_rank);
    std::free(i->send_first);
    std::free(i->send_offset);
    std::free(i->send_count);
    std::free(i->recv_offset);
    std::free(i->recv_count);
    std::free(i->ghost_row_gid);
    std::free(i->ghost_row_kind);
    std::free(i->ghost_row_cols);
    std::memset(i, 0, sizeof(*i));
}

int tm_edge_tables_probe(const tm_mesh_desc* mesh, const int32_t* owner, int32_t rank, int32_t nranks, int32_t table, int32_t level_strip,
                         tm_edge_tables_info* out) {
    return guarded([&]() {
        if (!mesh || !owner || !out) throw TmError(TM_E_ARG, "null argument");
        if (table < 0 || table > 5 || level_strip < 0) throw TmError(TM_E_ARG, "table outside 0..5 or negative strip length");
        std::memset(out, 0, sizeof(*out));
        const Topology t = topo_of(mesh);
        const std::vector<PlanRow> rows = build_rows(t);
        const LocalPlan lp = build_local_plan(t, rows, std::vector<int32_t>(owner, owner + t.nblocks()), rank, nranks);
        const MovingSides moving = moving_sides(t, lp);
        std::vector<PlanRow> zone[3];
        auto selection = [&](int tab) {
            std::vector<const PlanRow*> sel;
            auto add = [&](const std::vector<PlanRow>& more) {
                for (const PlanRow& r : more) sel.push_back(&r);
            };
            if (tab == 0) add(lp.rows);
            else for (size_t k : moving.nf_rows) sel.push_back(&lp.rows[k]);
            if (tab >= 3) add(zone[tab - 3] = zone_rows(t, lp, moving.dyn_mask, tab - 3));
            if (tab == 3) add(lp.ghost_rows2);
            if (tab == 2 || tab == 4) add(lp.ghost_rows);
            return sel;
        };
        RunTable level[3];
        for (int tab = 3; tab < 5 && table == 5; ++tab) level[tab - 3] = build_run_table(t, lp, selection(tab));
        const std::vector<const PlanRow*> sel = selection(table);
        const RunTable T = build_run_table(t, lp, sel);
        std::vector<int32_t> f[12], task;
        for (const EdgeRun& R : T.runs) {
            const int32_t scalars[8] = {R.first, R.count, R.row0, R.row_stride, R.kind, R.ncols, R.self, R.flags};
            for (int q = 0; q < 8; ++q) f[q].push_back(scalars[q]);
            f[8].insert(f[8].end(), R.col0, R.col0 + 9);
            f[9].insert(f[9].end(), R.col_stride, R.col_stride + 9);
            f[10].insert(f[10].end(), R.met0, R.met0 + 4);
            f[11].insert(f[11].end(), R.met_stride, R.met_stride + 4);
        }
        std::vector<int64_t> gid;
        for (int32_t k : T.order) gid.push_back(sel[k]->gid);
        StripPlan plan;
        if (table == 5) {
            const std::vector<EdgeRun>* const runs[3] = {&level[0].runs, &level[1].runs, &T.runs};
            plan = build_strip_plan(runs, T.where, level_strip ? level_strip : 60);
            for (int s = 0; s < plan.nstrips; ++s)
                for (int l = 0; l < 3; ++l)
                    for (int32_t k = plan.off[4 * s + l]; k < plan.off[4 * s + l + 1]; ++k)
                        task.insert(task.end(), {l + 1, plan.tasks[k].run, plan.tasks[k].k0, plan.tasks[k].count});
        }
        out->nrows = static_cast<int64_t>(sel.size());
        out->nruns = static_cast<int64_t>(T.runs.size());
        out->nwg = static_cast<int64_t>(T.wg_run.size());
        int32_t** const dst[12] = {&out->first, &out->count, &out->row0, &out->row_stride, &out->kind, &out->ncols, &out->self, &out->flags,
                                   &out->col0, &out->col_stride, &out->met0, &out->met_stride};
        for (int q = 0; q < 12; ++q) *dst[q] = dup(f[q]);
        out->wg_run = dup(T.wg_run);
        out->wg_k0 = dup(T.wg_k0);
        out->gid = dup(gid);
        out->nstrips = plan.nstrips;
        out->ntasks = static_cast<int64_t>(plan.tasks.size());
        out->strip_off = dup(plan.off);
        out->task = dup(task);
        return TM_OK;
    });
}
void tm_edge_tables_free(tm_edge_tables_info* i) {
    if (!i) return;
    int32_t* const arrays[] = {i->first, i->count, i->row0,   i->row_stride, i->col0,   i->col_stride, i->met0,      i->met_stride,
                               i->kind,  i->ncols, i->self,   i->flags,      i->wg_run, i->wg_k0,      i->strip_off, i->task};
    for (int32_t* p : arrays) std::free(p);
    std::free(i->gid);
    std::memset(i, 0, sizeof(*i));
}

int tm_plan_build(const tm_mesh_desc* mesh, tm_plan_rows* out) {
    return guarded([&]() {
        if (!mesh || !out) throw TmError(TM_E_ARG, "null argument");
        std::memset(out, 0, sizeof(*out));
        const Topology t = topo_of(mesh);
        const std::vector<PlanRow> rows = build_rows(t);
        const size_t n = rows.size();
        out->nrows = n;
        out->row = static_cast<int64_t*>(std::malloc(sizeof(int64_t) * (n ? n : 1)));
        out->kind = static_cast<int32_t*>(std::malloc(sizeof(int32_t) * (n ? n : 1)));
        out->ncols = static_cast<int32_t*>(std::malloc(sizeof(int32_t) * (n ? n : 1)));
        out->cols = static_cast<int64_t*>(std::malloc(sizeof(int64_t) * 9 * (n ? n : 1)));
        out->coef_x = static_cast<double*>(std::malloc(sizeof(double) * 9 * (n ? n : 1)));
        out->coef_y = static_cast<double*>(std::malloc(sizeof(double) * 9 * (n ? n : 1)));
        out->rhs = static_cast<double*>(std::malloc(sizeof(double) * 2 * (n ? n : 1)));
        out->slot = static_cast<int32_t*>(std::malloc(sizeof(int32_t) * 9 * (n ? n : 1)));
        if (!out->row || !out->kind || !out->ncols || !out->cols || !out->coef_x || !out->coef_y || !out->rhs || !out->slot) {
            tm_plan_free(out);
            throw TmError(TM_E_MEMORY, "out of host memory");
        }
        const double nan = std::numeric_limits<double>::quiet_NaN();
        for (size_t k = 0; k < n; ++k) {
            const PlanRow& r = rows[k];
            out->row[k] = r.gid;
            out->kind[k] = r.kind;
            out->ncols[k] = r.ncols;
            for (int q = 0; q < 9; ++q) {
                out->cols[k * 9 + q] = q < r.ncols ? r.col[q] : -1;
                out->coef_x[k * 9 + q] = (r.kind == KIND_SMOOTHED) ? nan : r.cx[q];
                out->coef_y[k * 9 + q] = (r.kind == KIND_SMOOTHED) ? nan : r.cy[q];
                out->slot[k * 9 + q] = r.slot[q];
            }
            out->rhs[2 * k] = (r.rhs_coord & 1) ? nan : r.rhs[0];
            out->rhs[2 * k + 1] = (r.rhs_coord & 2) ? nan : r.rhs[1];
        }
        return TM_OK;
    });
}
void tm_plan_free(tm_plan_rows* rows) {
    if (!rows) return;
    std::free(rows->row);
    std::free(rows->kind);
    std::free(rows->ncols);
    std::free(rows->cols);
    std::free(rows->coef_x);
    std::free(rows->coef_y);
    std::free(rows->rhs);
    std::free(rows->slot);
    std::memset(rows, 0, sizeof(*rows));
}

}  // extern "C"
