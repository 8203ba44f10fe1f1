// K22  smooth3d: Jacobi sweeps of the 3-D Winslow equations on a stored block with its six faces held (include/tm_hip.h, "elliptic
//      smoothing of stacked blocks"), plain or with the Thomas-Middlecoff / a prescribed control field.  gfx950, wave64.  The per-node
//      arithmetic, the line formula and the blend are tm_smooth3d.hpp, shared with the host twin (tm_smooth3d_host.cpp).
//
// k_s3_sweep<CONTROL>.  A workgroup of 256 threads owns a tile of S3_TI x S3_TJ = 32 x 8 nodes of an i-j plane, thread t node
// (i0 + t%32, j0 + t/32): consecutive lanes go along i, the fastest index of the planes, so a wave reads and writes two rows of 256
// contiguous bytes per component.  The workgroup MARCHES along k over a chunk of S3_KCHUNK node layers (grid.z chunks, so that a block
// with few tiles per plane still fills the part).  At layer k every thread loads its node of plane k+1 -- and the first 84 threads one
// node of the one-node rim around the tile -- into LDS slot (k+1) & 3, one barrier, then evaluates node k from the slots of the planes
// k-1, k, k+1: 48 LDS reads of 8 B per node (the node's own column km, P, kp rotates through registers).  Four slots, not three: the
// slot written at layer k was last read at layer k-2, and the barrier of layer k-1 lies between.  A plane is fetched from memory once
// per tile (x 340/256 for the rim, x (S3_KCHUNK + 2)/S3_KCHUNK for the chunk ends) instead of three times.  Row pitch 34 doubles: the 32
// lanes of a row read 256 contiguous bytes, every bank once.
// Nodes that are not interior are copied; lanes past the block load a clamped node and store nothing.
//
// Record: in-lane over the march, across the workgroup by a fixed tree through LDS (the plane slots are reused behind a barrier), one
// S3Acc per workgroup; k_s3_finalize (one wave) combines them in the fixed order of records_reduce_wave.  No floating-point atomics.
// The control maxima are order-independent: integer atomicMax on the bit patterns of |f|.
//
// LDS 32 640 B per workgroup.  Compiler's resource usage: DESIGN.md section 4, K22.
#include "tm_smooth3d.hpp"
#include "tm_stack_dev.hpp"
#include "tm_records.hpp"

#include <cstring>

namespace tmh {

constexpr int S3_TI = 32, S3_TJ = 8, S3_THREADS = S3_TI * S3_TJ, S3_KCHUNK = 16, S3_SLOTS = 4;
constexpr int S3_PI = S3_TI + 2, S3_PJ = S3_TJ + 2, S3_PLANE = S3_PI * S3_PJ, S3_RIM = S3_PLANE - S3_THREADS;
static_assert(S3_RIM <= S3_THREADS, "one thread stages at most one rim node");
static_assert(sizeof(S3Acc) * S3_THREADS <= sizeof(double) * S3_SLOTS * 3 * S3_PLANE, "the record tree reuses the plane slots");

struct S3Dims {
    size_t n[3];
};
struct S3Planes {
    const double* c[3];
};
struct S3Out {
    double* c[3];
};

template <bool CONTROL>
__global__ __launch_bounds__(S3_THREADS) void k_s3_sweep(S3Planes in, S3Out out, S3Planes f, int ni, int nj, int nk, double omega, S3Acc* __restrict__ partials) {
    __shared__ double sh[S3_SLOTS][3][S3_PLANE];
    const int t = threadIdx.x, ti = t % S3_TI, tj = t / S3_TI;
    const int i0 = static_cast<int>(blockIdx.x) * S3_TI, j0 = static_cast<int>(blockIdx.y) * S3_TJ;
    const int kb = static_cast<int>(blockIdx.z) * S3_KCHUNK, ke = kb + S3_KCHUNK < nk ? kb + S3_KCHUNK : nk;
    const int i = i0 + ti, j = j0 + tj;
    const bool inside = i < ni && j < nj;
    const int ic = i < ni ? i : ni - 1, jc = j < nj ? j : nj - 1;
    const bool interior_ij = i >= 1 && i + 1 < ni && j >= 1 && j + 1 < nj;
    // the rim node of this thread: padded position (ra, rb), clamped into the block
    const bool has_rim = t < S3_RIM;
    int ra = 0, rb = 0;
    if (t < S3_PI) {
        ra = t;
    } else if (t < 2 * S3_PI) {
        ra = t - S3_PI;
        rb = S3_PJ - 1;
    } else {
        ra = ((t - 2 * S3_PI) & 1) ? S3_PI - 1 : 0;
        rb = 1 + (t - 2 * S3_PI) / 2;
    }
    int gi = i0 - 1 + ra, gj = j0 - 1 + rb;
    gi = gi < 0 ? 0 : (gi < ni ? gi : ni - 1);
    gj = gj < 0 ? 0 : (gj < nj ? gj : nj - 1);
    const int own = (tj + 1) * S3_PI + ti + 1, rim = rb * S3_PI + ra;
    const size_t plane = static_cast<size_t>(ni) * nj;
    const size_t o_own = static_cast<size_t>(jc) * ni + ic, o_rim = static_cast<size_t>(gj) * ni + gi;

    auto stage = [&](int k) {
        double(*b)[S3_PLANE] = sh[k & (S3_SLOTS - 1)];
        const size_t base = static_cast<size_t>(k) * plane;
        const S3Vec v{in.c[0][base + o_own], in.c[1][base + o_own], in.c[2][base + o_own]};
        b[0][own] = v.x;
        b[1][own] = v.y;
        b[2][own] = v.z;
        if (has_rim) {
            b[0][rim] = in.c[0][base + o_rim];
            b[1][rim] = in.c[1][base + o_rim];
            b[2][rim] = in.c[2][base + o_rim];
        }
        return v;
    };

    S3Acc acc;
    s3_init(acc);
    S3Vec km{0.0, 0.0, 0.0}, cc, kp{0.0, 0.0, 0.0};
    if (kb > 0) km = stage(kb - 1);
    cc = stage(kb);
    for (int k = kb; k < ke; ++k) {
        if (k + 1 < nk) kp = stage(k + 1);
        __syncthreads();
        const size_t o = static_cast<size_t>(k) * plane + o_own;
        if (interior_ij && k >= 1 && k + 1 < nk) {
            const double(*bm)[S3_PLANE] = sh[(k - 1) & (S3_SLOTS - 1)];
            const double(*b0)[S3_PLANE] = sh[k & (S3_SLOTS - 1)];
            const double(*bp)[S3_PLANE] = sh[(k + 1) & (S3_SLOTS - 1)];
            auto at = [&](const double(*b)[S3_PLANE], int dj, int di) {
                const int q = own + dj * S3_PI + di;
                return S3Vec{b[0][q], b[1][q], b[2][q]};
            };
            S3Stencil s;
            s.p[1][1][1] = cc;
            s.p[0][1][1] = km;
            s.p[2][1][1] = kp;
            s.p[1][1][0] = at(b0, 0, -1);
            s.p[1][1][2] = at(b0, 0, 1);
            s.p[1][0][1] = at(b0, -1, 0);
            s.p[1][2][1] = at(b0, 1, 0);
            s.p[1][0][0] = at(b0, -1, -1);
            s.p[1][0][2] = at(b0, -1, 1);
            s.p[1][2][0] = at(b0, 1, -1);
            s.p[1][2][2] = at(b0, 1, 1);
            s.p[0][1][0] = at(bm, 0, -1);
            s.p[0][1][2] = at(bm, 0, 1);
            s.p[0][0][1] = at(bm, -1, 0);
            s.p[0][2][1] = at(bm, 1, 0);
            s.p[2][1][0] = at(bp, 0, -1);
            s.p[2][1][2] = at(bp, 0, 1);
            s.p[2][0][1] = at(bp, -1, 0);
            s.p[2][2][1] = at(bp, 1, 0);
            double f1 = 0.0, f2 = 0.0, f3 = 0.0;
            if (CONTROL) {
                f1 = f.c[0][o];
                f2 = f.c[1][o];
                f3 = f.c[2][o];
            }
            const S3Node n = s3_node<CONTROL>(s, f1, f2, f3, omega);
            out.c[0][o] = n.out.x;
            out.c[1][o] = n.out.y;
            out.c[2][o] = n.out.z;
            s3_count(acc, n, o);
        } else if (inside) {
            out.c[0][o] = cc.x;
            out.c[1][o] = cc.y;
            out.c[2][o] = cc.z;
        }
        km = cc;
        cc = kp;
    }
    __syncthreads();   // the last reads of the slots are done: the tree takes their place
    S3Acc* red = reinterpret_cast<S3Acc*>(&sh[0][0][0]);
    red[t] = acc;
    __syncthreads();
    for (int off = S3_THREADS / 2; off > 0; off >>= 1) {
        if (t < off) s3_combine(red[t], red[t + off]);
        __syncthreads();
    }
    if (t == 0) partials[(static_cast<size_t>(blockIdx.z) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = red[0];
}

__global__ __launch_bounds__(64) void k_s3_finalize(const S3Acc* __restrict__ partials, long long nrec, S3Acc* __restrict__ out) {
    __shared__ S3Acc sh[64];
    records_reduce_wave<S3Acc, s3_init, s3_combine>(partials, 0ll, nrec, sh);
    if (threadIdx.x == 0) *out = sh[0];
}

// the line formula on the faces: blockIdx.y is the direction, a thread takes one entry of its face tables
__global__ __launch_bounds__(256) void k_s3_control_faces(S3Dims dims, S3Planes in, S3Out F) {
    const int d = blockIdx.y;
    const size_t e = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
    if (e < s3_face_count(d, dims.n)) F.c[d][e] = s3_face_value(d, e, dims.n, in.c[0], in.c[1], in.c[2]);
}

__device__ __forceinline__ void s3_publish_max(unsigned long long* sh_max, const double* a, unsigned long long* cmax) {
    if (threadIdx.x < 3) sh_max[threadIdx.x] = 0;
    __syncthreads();
    for (int c = 0; c < 3; ++c)
        if (a[c] > 0.0) atomicMax(&sh_max[c], static_cast<unsigned long long>(__double_as_longlong(a[c])));   // >= 0: the bit pattern orders as the value
    __syncthreads();
    if (threadIdx.x < 3 && sh_max[threadIdx.x]) atomicMax(&cmax[threadIdx.x], sh_max[threadIdx.x]);
}

// the transfinite blend: a thread per node, the three planes written once (0 on every node that is not interior); BLEND false: the
// maxima of planes that are there already (TM_S3_PRESCRIBED)
template <bool BLEND>
__global__ __launch_bounds__(256) void k_s3_control_blend(S3Dims dims, S3Planes F, S3Out f, unsigned long long* __restrict__ cmax) {
    __shared__ unsigned long long sh_max[3];
    const size_t ni = dims.n[0], nj = dims.n[1], nk = dims.n[2];
    const size_t o = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
    double a[3] = {0.0, 0.0, 0.0};
    if (o < ni * nj * nk) {
        const size_t i = o % ni, j = (o / ni) % nj, k = o / (ni * nj);
        const bool interior = i >= 1 && i + 1 < ni && j >= 1 && j + 1 < nj && k >= 1 && k + 1 < nk;
        if (BLEND) {
            const double v0 = interior ? s3_blend(0, dims.n, F.c[0], i, j, k) : 0.0;
            const double v1 = interior ? s3_blend(1, dims.n, F.c[1], j, i, k) : 0.0;
            const double v2 = interior ? s3_blend(2, dims.n, F.c[2], k, i, j) : 0.0;
            f.c[0][o] = v0;
            f.c[1][o] = v1;
            f.c[2][o] = v2;
            a[0] = fabs(v0);
            a[1] = fabs(v1);
            a[2] = fabs(v2);
        } else if (interior) {
            for (int c = 0; c < 3; ++c) a[c] = fabs(F.c[c][o]);
        }
    }
    s3_publish_max(sh_max, a, cmax);
}

static dim3 s3_sweep_grid(const S3Plan& p) {
    return dim3(static_cast<unsigned>((p.n[0] + S3_TI - 1) / S3_TI), static_cast<unsigned>((p.n[1] + S3_TJ - 1) / S3_TJ),
                static_cast<unsigned>((p.n[2] + S3_KCHUNK - 1) / S3_KCHUNK));
}

static void s3_check_grid(const S3Plan& p) {
    const dim3 g = s3_sweep_grid(p);
    if (g.y > 65535u || g.z > 65535u) throw TmError(TM_E_SIZE, "block size out of range");
}

// Everything of a call that lives on the device: two copies of the block (the input goes into state[0 .. 3 nodes)), the field, the
// face tables, the records.
struct S3Dev {
    DevBuf state, field, faces, partials, acc, cmax;
    double* result = nullptr;   // where the planes lie behind run(): 3 * nodes doubles
    S3Planes f{{nullptr, nullptr, nullptr}};

    void alloc_state(const S3Plan& p) { state.grow(sizeof(double) * 6 * p.nodes, "smooth3d: two copies of the block"); }

    // f1..f3 of the block in state[0 .. 3 nodes) into `field` (TM_S3_THOMAS_MIDDLECOFF), or `prescribed` (host planes) up; the maxima
    void control(const S3Plan& p, const tm_smooth3d_opt* opt, hipStream_t st) {
        cmax.grow(sizeof(unsigned long long) * 3, "smooth3d: control maxima");
        HIPCHK(hipMemsetAsync(cmax.p, 0, sizeof(unsigned long long) * 3, st));
        if (p.algorithm == TM_S3_LAPLACE) return;
        field.grow(sizeof(double) * 3 * p.nodes, "smooth3d: control field");
        double* fd = field.as<double>();
        f = S3Planes{{fd, fd + p.nodes, fd + 2 * p.nodes}};
        const S3Out fo{{fd, fd + p.nodes, fd + 2 * p.nodes}};
        S3Dims dims{{p.n[0], p.n[1], p.n[2]}};
        const unsigned node_groups = static_cast<unsigned>((p.nodes + 255) / 256);
        if (p.algorithm == TM_S3_PRESCRIBED) {
            const double* h[3] = {opt->f1, opt->f2, opt->f3};
            for (int c = 0; c < 3; ++c) HIPCHK(hipMemcpyAsync(fd + c * p.nodes, h[c], sizeof(double) * p.nodes, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL((k_s3_control_blend<false>), dim3(node_groups), dim3(256), 0, st, dims, f, fo, cmax.as<unsigned long long>());
            HIPCHK(hipGetLastError());
            return;
        }
        size_t off[4] = {0, 0, 0, 0}, most = 0;
        for (int d = 0; d < 3; ++d) {
            const size_t cnt = s3_face_count(d, p.n);
            off[d + 1] = off[d] + cnt;
            most = cnt > most ? cnt : most;
        }
        faces.grow(sizeof(double) * off[3], "smooth3d: face tables");
        double* F = faces.as<double>();
        const double* s = state.as<double>();
        const S3Planes in{{s, s + p.nodes, s + 2 * p.nodes}};
        hipLaunchKernelGGL(k_s3_control_faces, dim3(static_cast<unsigned>((most + 255) / 256), 3), dim3(256), 0, st, dims, in, S3Out{{F + off[0], F + off[1], F + off[2]}});
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL((k_s3_control_blend<true>), dim3(node_groups), dim3(256), 0, st, dims, S3Planes{{F + off[0], F + off[1], F + off[2]}}, fo,
                           cmax.as<unsigned long long>());
        HIPCHK(hipGetLastError());
    }

    // The sweeps on `st`, ping-pong between the halves of `state`; the record into *info.  Synchronises st.
    void run(const S3Plan& p, const tm_smooth3d_opt* opt, hipStream_t st, tm_smooth3d_info* info) {
        s3_check_grid(p);
        control(p, opt, st);
        double* cur = state.as<double>();
        double* nxt = cur + 3 * p.nodes;
        const dim3 grid = s3_sweep_grid(p);
        const size_t nrec = static_cast<size_t>(grid.x) * grid.y * grid.z;   // the records buffer is sized from the very grid that writes it
        const bool sweeping = p.sweeps > 0 && p.interior > 0;
        if (sweeping) {
            partials.grow(sizeof(S3Acc) * nrec, "smooth3d: records");
            acc.grow(sizeof(S3Acc) * 2, "smooth3d: reduced records");
        }
        S3Acc host_acc[2];
        uint64_t done = 0;
        const bool with_control = p.algorithm != TM_S3_LAPLACE;
        auto finalize = [&](int slot) {
            hipLaunchKernelGGL(k_s3_finalize, dim3(1), dim3(64), 0, st, partials.as<S3Acc>(), static_cast<long long>(nrec), acc.as<S3Acc>() + slot);
            HIPCHK(hipGetLastError());
        };
        while (sweeping && done < p.sweeps) {
            const S3Planes in{{cur, cur + p.nodes, cur + 2 * p.nodes}};
            const S3Out out{{nxt, nxt + p.nodes, nxt + 2 * p.nodes}};
            if (with_control)
                hipLaunchKernelGGL((k_s3_sweep<true>), grid, dim3(S3_THREADS), 0, st, in, out, f, static_cast<int>(p.n[0]), static_cast<int>(p.n[1]),
                                   static_cast<int>(p.n[2]), p.omega, partials.as<S3Acc>());
            else
                hipLaunchKernelGGL((k_s3_sweep<false>), grid, dim3(S3_THREADS), 0, st, in, out, f, static_cast<int>(p.n[0]), static_cast<int>(p.n[1]),
                                   static_cast<int>(p.n[2]), p.omega, partials.as<S3Acc>());
            HIPCHK(hipGetLastError());
            std::swap(cur, nxt);
            if (done++ == 0) finalize(0);
            const bool check = s3_check_after(p, done);
            if (check || done == p.sweeps) finalize(1);
            if (check) {   // the one read-back inside a call
                HIPCHK(hipMemcpyAsync(&host_acc[1], acc.as<S3Acc>() + 1, sizeof(S3Acc), hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
                if (s3_converged(p, host_acc[1].sum_sq)) break;
            }
        }
        result = cur;
        unsigned long long bits[3];
        HIPCHK(hipMemcpyAsync(bits, cmax.p, sizeof bits, hipMemcpyDeviceToHost, st));
        if (sweeping) HIPCHK(hipMemcpyAsync(host_acc, acc.p, sizeof(S3Acc) * 2, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        double cm[3];
        std::memcpy(cm, bits, sizeof cm);
        s3_fill_info(p, done, sweeping ? &host_acc[0] : nullptr, sweeping ? &host_acc[1] : nullptr, cm, info);
    }

    void download(const S3Plan& p, const double* from, double* x, double* y, double* z, hipStream_t st) {
        HIPCHK(hipMemcpyAsync(x, from, sizeof(double) * p.nodes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(y, from + p.nodes, sizeof(double) * p.nodes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(z, from + 2 * p.nodes, sizeof(double) * p.nodes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    void upload(const S3Plan& p, const double* x, const double* y, const double* z, hipStream_t st) {
        alloc_state(p);
        double* s = state.as<double>();
        HIPCHK(hipMemcpyAsync(s, x, sizeof(double) * p.nodes, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(s + p.nodes, y, sizeof(double) * p.nodes, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(s + 2 * p.nodes, z, sizeof(double) * p.nodes, hipMemcpyHostToDevice, st));
    }
};

}  // namespace tmh

using namespace tmh;

extern "C" int tm_smooth3d_planes(uint64_t ni, uint64_t nj, uint64_t nk, double* x, double* y, double* z, const tm_smooth3d_opt* opt, tm_smooth3d_info* info) {
    return guarded([&]() {
        if (!info) throw TmError(TM_E_ARG, "null argument");
        const S3Plan p = s3_plan(ni, nj, nk, x, y, z, opt);
        require_gfx950();
        S3Dev dev;
        dev.upload(p, x, y, z, nullptr);
        dev.run(p, opt, nullptr, info);
        if (info->sweeps_done) dev.download(p, dev.result, x, y, z, nullptr);
        return TM_OK;
    });
}

extern "C" int tm_smooth3d_control(uint64_t ni, uint64_t nj, uint64_t nk, const double* x, const double* y, const double* z, double* f1, double* f2, double* f3) {
    return guarded([&]() {
        if (!f1 || !f2 || !f3) throw TmError(TM_E_ARG, "null argument");
        tm_smooth3d_opt o{};
        o.algorithm = TM_S3_THOMAS_MIDDLECOFF;
        o.omega = 1.0;
        const S3Plan p = s3_plan(ni, nj, nk, x, y, z, &o);
        require_gfx950();
        S3Dev dev;
        dev.upload(p, x, y, z, nullptr);
        dev.control(p, &o, nullptr);
        dev.download(p, dev.field.as<double>(), f1, f2, f3, nullptr);
        return TM_OK;
    });
}

// sf: the filled meridional plan of the _surf entry point, null for the plain one (`p` then comes from stack_plan)
static void stack_smoothers_smooth(tm_smoother* const* cuts, const StackPlan& p, const SurfPlan* sf, uint64_t block, const tm_smooth3d_opt* opt, double* x, double* y,
                                   double* z, tm_smooth3d_info* info) {
    StackCuts dc{};
    uint64_t ni = 0, nj = 0;
    stack_resident_cuts(cuts, p, block, dc, &ni, &nj);
    if (p.nlayers >= (uint64_t{1} << 31)) throw TmError(TM_E_SIZE, "layer window out of range");
    const S3Plan sp = s3_plan(ni, nj, p.nlayers, x, y, z, opt);
    std::vector<std::unique_ptr<StackEvent>> events;
    const hipStream_t st = stack_order_behind(cuts, p.ncuts, events);
    stack_fill_radii(p, dc);
    StackSurfDev sd;
    if (sf) stack_surf_upload(p, *sf, dc, sd, st);
    const std::vector<double> table = stack_weight_table(p, 0, p.nlayers);
    DevBuf d_table;
    d_table.upload(table.data(), table.size(), st, "stack weights");
    S3Dev dev;
    dev.alloc_state(sp);
    double* s = dev.state.as<double>();
    HIPCHK(launch_stack_planes(p.ncuts, dc, sd.surf, p.mapping, d_table.as<double>(), static_cast<int>(p.nlayers), static_cast<int>(ni), static_cast<int>(nj), s,
                               s + sp.nodes, s + 2 * sp.nodes, nullptr, st));
    dev.run(sp, opt, st, info);   // synchronises st: `table` and the other handles' coordinates have been read when it returns
    dev.download(sp, dev.result ? dev.result : s, x, y, z, st);
}

extern "C" int tm_stack_smoothers_smooth(tm_smoother* const* cuts, const tm_stack_opt* opt, uint64_t block, const tm_smooth3d_opt* smooth, double* x, double* y,
                                         double* z, tm_smooth3d_info* info) {
    return guarded([&]() {
        if (!cuts || !x || !y || !z || !smooth || !info) throw TmError(TM_E_ARG, "null argument");
        stack_smoothers_smooth(cuts, stack_plan(opt), nullptr, block, smooth, x, y, z, info);
        return TM_OK;
    });
}

extern "C" int tm_stack_smoothers_smooth_surf(tm_smoother* const* cuts, const tm_stack_opt* opt, const tm_stack_surfaces* surfaces, uint64_t block,
                                              const tm_smooth3d_opt* smooth, double* x, double* y, double* z, tm_smooth3d_info* info) {
    return guarded([&]() {
        if (!cuts || !x || !y || !z || !smooth || !info) throw TmError(TM_E_ARG, "null argument");
        SurfPlan sf;
        const StackPlan p = stack_plan_surf(opt, surfaces, sf);
        stack_smoothers_smooth(cuts, p, &sf, block, smooth, x, y, z, info);
        return TM_OK;
    });
}
