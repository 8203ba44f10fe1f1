// Seam 2 -- the reference's linear-solver slot (reference src/core/smoothing/solver.zig:40-93): a backend receives the
// ASSEMBLED system `RowCompressedMatrixSystem2d` (smooth.zig:277-307: lhs_p, lhs_i, lhs_values, rhs_x, rhs_y, x_new, y_new)
// and solves the x- and the y-system, calling system.fillXSpecific() / fillYSpecific() before the respective solve
// (umfpack.zig:18-24) -- the two systems share the pattern and differ only in the two entries of each `sliding_circ` row
// (smooth.zig:1115-1165).  tm_csr_solve is that backend on the MI355X: caller-assembled CSR in, both components solved
// TOGETHER as double2 vectors with the same device-resident BiCGStab as the matrix-free path (recurrences of
// BiCGStab.zig:279-370 on the row-equilibrated system D^-1 A x = D^-1 b, scale-aware stop test, restart on breakdown).
// Not the performance path: the matrix travels over PCIe per call and the mat-vec streams 12 B per non-zero; it exists so
// that a Zig `Solver` arm needs no change to smooth.mesh, and so that the tests have an operator check that never touches
// the matrix-free kernels.
#include "tm_api_util.hpp"
#include "tm_devutil.hpp"
#include "tm_ilu.hpp"
#include "tm_refine.hpp"
#include <array>
#include <chrono>
#include <cstring>
#include <memory>
#include <vector>

namespace tmh {

namespace {

struct CsrDev {
    int n;
    const int32_t* p;
    const int32_t* i;
    const double* vx;   // values of the x-system
    const double* vy;   // values of the y-system (== vx when the caller passes one array)
    const double2* dinv;
};

// 1 / a_ii per row and component; a missing or zero diagonal scales by 1 (BiCGStab.zig:155-175)
__global__ __launch_bounds__(256) void k_csr_dinv(int n, const int32_t* __restrict__ p, const int32_t* __restrict__ ci, const double* __restrict__ vx,
                                                  const double* __restrict__ vy, double2* __restrict__ dinv, double2* __restrict__ dvec) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    double dx = 0.0, dy = 0.0;
    for (int k = p[row]; k < p[row + 1]; ++k)
        if (ci[k] == row) {
            dx = vx[k];
            dy = vy[k];
            break;
        }
    dinv[row] = make_double2(dx == 0.0 ? 1.0 : 1.0 / dx, dy == 0.0 ? 1.0 : 1.0 / dy);
    if (dvec) dvec[row] = make_double2(dx == 0.0 ? 1.0 : dx, dy == 0.0 ? 1.0 : dy);
}

// one thread per row (<= 9 non-zeros in the reference's systems).  RESID: out = D^-1 (b - A in), else out = D^-1 A in;
// fused partial dot products like K2 (tm_kernels.h DotMode)
template <bool RESID, int DOT>
__global__ __launch_bounds__(256) void k_csr_apply(CsrDev A, const double2* __restrict__ in, const double2* __restrict__ b, const double2* __restrict__ aux,
                                                   double2* __restrict__ out, double* partials) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    double acc[MAX_PARTIALS] = {0.0, 0.0, 0.0, 0.0};
    if (row < A.n) {
        double sx = 0.0, sy = 0.0;
        for (int k = A.p[row]; k < A.p[row + 1]; ++k) {   // BiCGStab.zig:424-435, both components
            const double2 w = in[A.i[k]];
            sx += A.vx[k] * w.x;
            sy += A.vy[k] * w.y;
        }
        const double2 d = A.dinv[row];
        double2 o;
        if (RESID) {
            const double2 rhs = b[row];
            o = make_double2(rhs.x * d.x - sx * d.x, rhs.y * d.y - sy * d.y);
        } else {
            o = make_double2(sx * d.x, sy * d.y);
        }
        out[row] = o;
        if (DOT == DOT_AUX) {
            const double2 a = aux[row];
            acc[0] = a.x * o.x;
            acc[1] = a.y * o.y;
        } else if (DOT == DOT_IN) {
            const double2 w = in[row];
            acc[0] = w.x * o.x;
            acc[1] = w.y * o.y;
            acc[2] = o.x * o.x;
            acc[3] = o.y * o.y;
        } else if (DOT == DOT_AUX2) {   // the operator acted on a preconditioned vector: t.s and t.t with the UNpreconditioned s in `aux`
            const double2 a = aux[row];
            acc[0] = a.x * o.x;
            acc[1] = a.y * o.y;
            acc[2] = o.x * o.x;
            acc[3] = o.y * o.y;
        } else if (DOT == DOT_OUT2) {
            acc[0] = o.x * o.x;
            acc[1] = o.y * o.y;
        }
    }
    if (DOT != DOT_NONE) block_partials<256>(acc, partials + static_cast<size_t>(blockIdx.x) * MAX_PARTIALS);
}

// partials of ||D^-1 b||^2 per component (the stop test's reference norm)
__global__ __launch_bounds__(256) void k_csr_bnorm(int n, const double2* __restrict__ b, const double2* __restrict__ dinv, double* partials) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    double acc[MAX_PARTIALS] = {0.0, 0.0, 0.0, 0.0};
    if (row < n) {
        const double2 v = b[row], d = dinv[row];
        acc[0] = (v.x * d.x) * (v.x * d.x);
        acc[1] = (v.y * d.y) * (v.y * d.y);
    }
    block_partials<256>(acc, partials + static_cast<size_t>(blockIdx.x) * MAX_PARTIALS);
}

// partials of ||v||^2 per component
__global__ __launch_bounds__(256) void k_csr_norm2(int n, const double2* __restrict__ v, double* partials) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    double acc[MAX_PARTIALS] = {0.0, 0.0, 0.0, 0.0};
    if (row < n) {
        const double2 w = v[row];
        acc[0] = w.x * w.x;
        acc[1] = w.y * w.y;
    }
    block_partials<256>(acc, partials + static_cast<size_t>(blockIdx.x) * MAX_PARTIALS);
}

__global__ __launch_bounds__(256) void k_interleave(int n, const double* __restrict__ a, const double* __restrict__ b, double2* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = make_double2(a[i], b[i]);
}
__global__ __launch_bounds__(256) void k_deinterleave(int n, const double2* __restrict__ in, double* __restrict__ a, double* __restrict__ b) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const double2 v = in[i];
        a[i] = v.x;
        b[i] = v.y;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// ILU(0) on the device (TM_OPT_PRECOND_ILU0: seam 2 and TM_INNER_REFERENCE_GMRES; IluState in tm_ilu.hpp): the reference's second preconditioner (preconditioner.zig:1-4; factorisation
// BiCGStab.zig:178-277, application :384-422 -- identical copies in GMRES.zig:199-298, 437-475), which its example inputs select.
// The recurrence is sequential row by row; what is parallel are the LEVEL SETS of its dependency graph: row i needs the finished rows
// k < i of its own pattern (factorisation and forward substitution alike), the backward substitution the rows k > i.  The host sorts the
// rows by level once per call (the pattern is the caller's); every row keeps the reference's operation order -- entries in CSR order,
// the update `lu[pos] -= l_ik * lu[k, j]` un-fused -- so the factor and M^-1 r equal the reference's bit for bit (tests/test_gpu_ilu0.py
// against the faithful oracle).  Levels of the reference's systems are narrow (T106: 1790 levels of ~14 rows): runs of levels with at most
// 256 rows execute inside ONE single-workgroup launch with a barrier between levels; a wider level gets a launch of its own.
// k_ilu_levels serves the factorisation (once per outer iteration) and, for patterns with more than 16 entries on one side of the diagonal,
// the substitutions: there a level is a chain of dependent loads (~1.8-2.3 us; T106's 2655 levels: 4.8 ms per application).  The
// substitutions of every other pattern run on the level-packed form below (k_ilu_subst_packed: T106 2.2 ms; tools/reference_solve_timing.py).
// Tried and dropped: fetching a level's matrix data one level ahead into DYNAMICALLY indexed per-thread arrays (they go to scratch: 43 ms per
// iteration instead of 14) -- the packed kernel's arrays have a template width and index statically.
enum { ILU_FACTOR = 0, ILU_FORWARD = 1, ILU_BACKWARD = 2 };

__device__ __forceinline__ double ilu_pivot(const double* lu, int pos) {   // a missing or zero diagonal counts as 1 (BiCGStab.zig:240-249, 413-418)
    if (pos < 0) return 1.0;
    const double d = lu[pos];
    return d == 0.0 ? 1.0 : d;
}
__device__ __forceinline__ void ilu_factor_row(const IluDev& M, double* lu, int row) {
    const int start = M.p[row], end = M.p[row + 1];
    for (int idx = start; idx < end; ++idx) {
        const int col = M.ci[idx];
        if (col >= row) continue;
        const double lij = lu[idx] / ilu_pivot(lu, M.diag_pos[col]);
        lu[idx] = lij;
        for (int r = M.p[col]; r < M.p[col + 1]; ++r) {
            const int col_k = M.ci[r];
            if (col_k <= col) continue;
            for (int q = start; q < end; ++q)   // the reference's marker[]: where column col_k sits in THIS row, if it does
                if (M.ci[q] == col_k) {
                    lu[q] -= lij * lu[r];
                    break;
                }
        }
    }
}
template <int OP>
__device__ __forceinline__ void ilu_row(const IluDev& M, int row, const double2* __restrict__ rhs, double2* out) {
    if (OP == ILU_FACTOR) {
        ilu_factor_row(M, M.lux, row);
        if (M.luy != M.lux) ilu_factor_row(M, M.luy, row);
        return;
    }
    const int start = M.p[row], end = M.p[row + 1];
    if (OP == ILU_FORWARD) {
        double2 sum = rhs[row];
        if (M.dvec) {
            const double2 d = M.dvec[row];
            sum.x *= d.x;
            sum.y *= d.y;
        }
        for (int idx = start; idx < end; ++idx) {
            const int col = M.ci[idx];
            if (col < row) {
                const double2 o = out[col];
                sum.x -= M.lux[idx] * o.x;
                sum.y -= M.luy[idx] * o.y;
            }
        }
        out[row] = sum;
    } else {
        double2 sum = out[row];
        for (int idx = start; idx < end; ++idx) {
            const int col = M.ci[idx];
            if (col > row) {
                const double2 o = out[col];
                sum.x -= M.lux[idx] * o.x;
                sum.y -= M.luy[idx] * o.y;
            }
        }
        out[row] = make_double2(sum.x / ilu_pivot(M.lux, M.diag_pos[row]), sum.y / ilu_pivot(M.luy, M.diag_pos[row]));
    }
}
// levels [lv0, lv1) of `order` / `lev_ptr`.  One workgroup: every level has <= 256 rows, a barrier separates them (what a level reads
// was written by this workgroup).  Several workgroups: lv1 == lv0 + 1, one thread per row of that level.
template <int OP>
__global__ __launch_bounds__(256) void k_ilu_levels(IluDev M, const int32_t* __restrict__ order, const int32_t* __restrict__ lev_ptr, int lv0, int lv1,
                                                    const double2* __restrict__ rhs, double2* out) {
    if (gridDim.x > 1) {
        const int k = lev_ptr[lv0] + static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
        if (k < lev_ptr[lv0 + 1]) ilu_row<OP>(M, order[k], rhs, out);
        return;
    }
    for (int l = lv0; l < lv1; ++l) {
        const int k = lev_ptr[l] + static_cast<int>(threadIdx.x);
        if (k < lev_ptr[l + 1]) ilu_row<OP>(M, order[k], rhs, out);
        __syncthreads();   // (a workgroup-scope release / acquire: the next level reads what this one stored)
    }
}

// ---- the substitutions on the level-packed form (IluPacked, tm_ilu.hpp).  In k_ilu_levels a row of a level walks order[k] -> p[row] ->
// ci[idx] -> lu[idx], out[col] -> diag_pos -> lu[diag]: four to five DEPENDENT loads, of which only out[col] depends on the previous level.
// Here position k of the level order owns WIDTH slots (column, both factors' values) at unit stride, the pivot and its right-hand side, all
// independent of `out`: a lane fetches them ONE LEVEL AHEAD into registers (WIDTH is a template constant: the slot loops unroll fully and
// index statically), so that a level costs one gather of out[col], the subtraction chain in the row's CSR order and a barrier.
// One workgroup per launch: the hand-off between levels is the workgroup barrier (NT == 64: one wave).  A level wider than the workgroup is
// taken in strides of NT rows, the later strides loading on demand.
template <int WIDTH>
struct PackedRow {
    int32_t row;
    int32_t c[WIDTH];
    double2 v[WIDTH];
    double2 piv, rhs;
};
template <int WIDTH, bool BACK>
__device__ __forceinline__ void packed_load(const IluPackedDev& P, size_t k, const double2* rhs, const double2* dvec, PackedRow<WIDTH>& R) {
    R.row = P.order[k];
#pragma unroll
    for (int s = 0; s < WIDTH; ++s) {
        R.c[s] = P.col[static_cast<size_t>(s) * P.n + k];
        R.v[s] = P.val[static_cast<size_t>(s) * P.n + k];
    }
    R.rhs = rhs[R.row];   // backward: what the forward pass left in out[row] -- only this row's own store changes it
    if (BACK) {
        R.piv = P.piv[k];
    } else if (dvec) {
        const double2 d = dvec[R.row];
        R.rhs.x *= d.x;
        R.rhs.y *= d.y;
    }
}
template <int WIDTH, bool BACK>
__device__ __forceinline__ void packed_row(const PackedRow<WIDTH>& R, double2* out) {
    double2 o[WIDTH];
#pragma unroll
    for (int s = 0; s < WIDTH; ++s) o[s] = out[R.c[s] < 0 ? 0 : R.c[s]];   // the one access that depends on the previous level
    double2 sum = R.rhs;
#pragma unroll
    for (int s = 0; s < WIDTH; ++s)
        if (R.c[s] >= 0) {   // (an empty slot is skipped, not multiplied by zero: -0.0 - 0.0 * o would lose its sign)
            sum.x -= R.v[s].x * o[s].x;
            sum.y -= R.v[s].y * o[s].y;
        }
    if (BACK) sum = make_double2(sum.x / R.piv.x, sum.y / R.piv.y);
    out[R.row] = sum;
}
template <int WIDTH, bool BACK, int NT>
__global__ __launch_bounds__(NT) void k_ilu_subst_packed(IluPackedDev P, const double2* rhs, const double2* dvec, double2* out) {
    const int tid = static_cast<int>(threadIdx.x);
    int beg = P.ptr[0], end = P.ptr[1];
    PackedRow<WIDTH> cur, nxt;
    if (beg + tid < end) packed_load<WIDTH, BACK>(P, static_cast<size_t>(beg + tid), rhs, dvec, cur);
    for (int l = 0; l < P.nlev; ++l) {
        const int nbeg = end, nend = l + 1 < P.nlev ? P.ptr[l + 2] : end;
        if (nbeg + tid < nend) packed_load<WIDTH, BACK>(P, static_cast<size_t>(nbeg + tid), rhs, dvec, nxt);
        if (beg + tid < end) packed_row<WIDTH, BACK>(cur, out);
        for (int k = beg + tid + NT; k < end; k += NT) {
            PackedRow<WIDTH> more;
            packed_load<WIDTH, BACK>(P, static_cast<size_t>(k), rhs, dvec, more);
            packed_row<WIDTH, BACK>(more, out);
        }
        __syncthreads();   // (a workgroup-scope release / acquire: the next level reads what this one stored)
        cur = nxt;
        beg = nbeg;
        end = nend;
    }
}
// values of the packed slots from the factors (after every factorisation); src = position in lu, -1 = empty slot
__global__ __launch_bounds__(256) void k_ilu_pack(size_t nslots, const int32_t* __restrict__ src, const double* __restrict__ lux, const double* __restrict__ luy,
                                                  double2* __restrict__ val) {
    const size_t t = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
    if (t >= nslots) return;
    const int32_t idx = src[t];
    val[t] = idx < 0 ? make_double2(0.0, 0.0) : make_double2(lux[idx], luy[idx]);
}
__global__ __launch_bounds__(256) void k_ilu_pack_pivots(IluDev M, const int32_t* __restrict__ order, double2* __restrict__ piv) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= M.n) return;
    const int pos = M.diag_pos[order[k]];
    piv[k] = make_double2(ilu_pivot(M.lux, pos), ilu_pivot(M.luy, pos));
}

template <int WIDTH, bool BACK>
void launch_subst_packed(const IluPackedDev& P, int max_width, const double2* rhs, const double2* dvec, double2* out, hipStream_t st) {
    if (max_width <= 64) hipLaunchKernelGGL((k_ilu_subst_packed<WIDTH, BACK, 64>), dim3(1), dim3(64), 0, st, P, rhs, dvec, out);
    else hipLaunchKernelGGL((k_ilu_subst_packed<WIDTH, BACK, 256>), dim3(1), dim3(256), 0, st, P, rhs, dvec, out);
    HIPCHK(hipGetLastError());
}
template <bool BACK>
void subst_packed(int width, const IluPackedDev& P, int max_width, const double2* rhs, const double2* dvec, double2* out, hipStream_t st) {
    if (width <= 4) launch_subst_packed<4, BACK>(P, max_width, rhs, dvec, out, st);
    else if (width <= 8) launch_subst_packed<8, BACK>(P, max_width, rhs, dvec, out, st);
    else launch_subst_packed<16, BACK>(P, max_width, rhs, dvec, out, st);
}

__global__ __launch_bounds__(256) void k_csr_sub(int n, const double2* b, const double2* w, double2* r) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double2 bi = b[i], wi = w[i];
    r[i] = make_double2(bi.x - wi.x, bi.y - wi.y);
}
__global__ __launch_bounds__(256) void k_csr_diag_precond(int n, const double2* __restrict__ dinv, const double2* r, double2* z) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double2 d = dinv[i], ri = r[i];
    z[i] = make_double2(ri.x * d.x, ri.y * d.y);
}

}  // namespace

void IluLevels::build(int n, const int32_t* p, const int32_t* ci, bool lower) {
    std::vector<int32_t> lev(static_cast<size_t>(n), 0);
    int32_t nlev = 0;
    auto visit = [&](int row) {
        int32_t l = 0;
        for (int k = p[row]; k < p[row + 1]; ++k) {
            const int col = ci[k];
            if (lower ? col < row : col > row) l = std::max(l, lev[col] + 1);
        }
        lev[row] = l;
        nlev = std::max(nlev, l + 1);
    };
    if (lower) for (int row = 0; row < n; ++row) visit(row);
    else for (int row = n - 1; row >= 0; --row) visit(row);
    ptr.assign(static_cast<size_t>(nlev) + 1, 0);
    for (int row = 0; row < n; ++row) ptr[lev[row] + 1] += 1;
    max_width = 0;
    for (int l = 0; l < nlev; ++l) {
        max_width = std::max<int>(max_width, ptr[l + 1]);
        ptr[l + 1] += ptr[l];
    }
    order.resize(static_cast<size_t>(n));
    std::vector<int32_t> at(ptr.begin(), ptr.end() - 1);
    for (int row = 0; row < n; ++row) order[at[lev[row]]++] = row;   // ascending row id inside a level
    chunks.clear();
    for (int l = 0; l < nlev;) {
        if (ptr[l + 1] - ptr[l] > 256) {
            chunks.push_back({l, l + 1});
            ++l;
            continue;
        }
        int e = l;
        while (e < nlev && ptr[e + 1] - ptr[e] <= 256 && e - l < (1 << 20)) ++e;
        chunks.push_back({l, e});
        l = e;
    }
}

void IluPacked::build(int n, const int32_t* p, const int32_t* ci, const IluLevels& lv, bool lower) {
    int most = 0;
    for (int row = 0; row < n; ++row) {
        int cnt = 0;
        for (int k = p[row]; k < p[row + 1]; ++k) cnt += (lower ? ci[k] < row : ci[k] > row) ? 1 : 0;
        most = std::max(most, cnt);
    }
    width = most <= 4 ? 4 : most <= 8 ? 8 : most <= 16 ? 16 : 0;   // the instantiated kernels; 0: not packable
    if (!width) return;
    const size_t nslots = static_cast<size_t>(width) * static_cast<size_t>(n);
    std::vector<int32_t> col(nslots, -1), src(nslots, -1);
    for (int k = 0; k < n; ++k) {
        const int row = lv.order[static_cast<size_t>(k)];
        int s = 0;
        for (int idx = p[row]; idx < p[row + 1]; ++idx)   // the row's CSR order
            if (lower ? ci[idx] < row : ci[idx] > row) {
                col[static_cast<size_t>(s) * n + k] = ci[idx];
                src[static_cast<size_t>(s) * n + k] = idx;
                ++s;
            }
    }
    d_col.grow(sizeof(int32_t) * nslots, "ilu col");
    d_src.grow(sizeof(int32_t) * nslots, "ilu src");
    d_val.grow(sizeof(double2) * nslots, "ilu val");
    d_piv.grow(sizeof(double2) * static_cast<size_t>(n), "ilu piv");
    HIPCHK(hipMemcpy(d_col.p, col.data(), sizeof(int32_t) * nslots, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_src.p, src.data(), sizeof(int32_t) * nslots, hipMemcpyHostToDevice));
}

IluState::IluState(int n_, const int32_t* Ap, const int32_t* Ai, size_t nnz, bool two, int use_packed)
    : d_diag(sizeof(int32_t) * static_cast<size_t>(n_), "ilu diag"), d_lux(sizeof(double) * nnz, "ilu lux"), d_luy(two ? sizeof(double) * nnz : 0, "ilu luy"),
      d_ordL(sizeof(int32_t) * static_cast<size_t>(n_), "ilu ordL"), d_ordU(sizeof(int32_t) * static_cast<size_t>(n_), "ilu ordU"), n(n_) {
    std::vector<int32_t> diag(static_cast<size_t>(n), -1);
    for (int row = 0; row < n; ++row)
        for (int k = Ap[row]; k < Ap[row + 1]; ++k)
            if (Ai[k] == row) {
                diag[row] = k;
                break;
            }
    L.build(n, Ap, Ai, true);
    U.build(n, Ap, Ai, false);
    HIPCHK(hipMemcpy(d_diag.p, diag.data(), sizeof(int32_t) * diag.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_ordL.p, L.order.data(), sizeof(int32_t) * L.order.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_ordU.p, U.order.data(), sizeof(int32_t) * U.order.size(), hipMemcpyHostToDevice));
    d_ptrL.grow(sizeof(int32_t) * L.ptr.size(), "ilu ptrL");
    d_ptrU.grow(sizeof(int32_t) * U.ptr.size(), "ilu ptrU");
    HIPCHK(hipMemcpy(d_ptrL.p, L.ptr.data(), sizeof(int32_t) * L.ptr.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_ptrU.p, U.ptr.data(), sizeof(int32_t) * U.ptr.size(), hipMemcpyHostToDevice));
    if (use_packed < 0) {
        const char* e = std::getenv("TM_ILU_PACKED");   // 0: the substitutions by k_ilu_levels (measurement: tools/reference_solve_timing.py)
        use_packed = (e && std::atoi(e) == 0) ? 0 : 1;
    }
    if (use_packed) {
        PL.build(n, Ap, Ai, L, true);
        PU.build(n, Ap, Ai, U, false);
        packed = PL.width > 0 && PU.width > 0;
    }
}

namespace {
template <int OP>
void run_levels(const IluDev& M, const IluLevels& lv, const int32_t* order, const int32_t* ptr, const double2* rhs, double2* out, hipStream_t st) {
    for (const auto& c : lv.chunks) {
        const int width = lv.ptr[c[0] + 1] - lv.ptr[c[0]];
        const int grid = (c[1] - c[0] == 1 && width > 256) ? (width + 255) / 256 : 1;
        hipLaunchKernelGGL((k_ilu_levels<OP>), dim3(grid), dim3(256), 0, st, M, order, ptr, c[0], c[1], rhs, out);
        HIPCHK(hipGetLastError());
    }
}
}  // namespace

void IluState::factor(int n_, const int32_t* d_p, const int32_t* d_i, const double* d_vx, const double* d_vy, size_t nnz, const double2* dvec, hipStream_t st) {
    const bool two = d_vy != nullptr && d_vy != d_vx;
    HIPCHK(hipMemcpyAsync(d_lux.p, d_vx, sizeof(double) * nnz, hipMemcpyDeviceToDevice, st));
    if (two) HIPCHK(hipMemcpyAsync(d_luy.p, d_vy, sizeof(double) * nnz, hipMemcpyDeviceToDevice, st));
    M = IluDev{n_, d_p, d_i, d_diag.as<int32_t>(), d_lux.as<double>(), two ? d_luy.as<double>() : d_lux.as<double>(), dvec};
    run_levels<ILU_FACTOR>(M, L, d_ordL.as<int32_t>(), d_ptrL.as<int32_t>(), nullptr, nullptr, st);
    if (!packed) return;
    for (IluPacked* P : {&PL, &PU}) {
        const size_t nslots = static_cast<size_t>(P->width) * static_cast<size_t>(n);
        hipLaunchKernelGGL(k_ilu_pack, dim3(static_cast<unsigned>((nslots + 255) / 256)), dim3(256), 0, st, nslots, P->d_src.as<int32_t>(), M.lux, M.luy,
                           P->d_val.as<double2>());
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_ilu_pack_pivots, dim3((n + 255) / 256), dim3(256), 0, st, M, d_ordU.as<int32_t>(), PU.d_piv.as<double2>());
    HIPCHK(hipGetLastError());
}

void IluState::apply(const double2* rhs, double2* out, hipStream_t st, bool times_d) {
    if (packed) {
        const IluPackedDev fw{n, static_cast<int>(L.ptr.size()) - 1, d_ptrL.as<int32_t>(), d_ordL.as<int32_t>(), PL.d_col.as<int32_t>(), PL.d_val.as<double2>(), nullptr};
        const IluPackedDev bw{n, static_cast<int>(U.ptr.size()) - 1, d_ptrU.as<int32_t>(), d_ordU.as<int32_t>(), PU.d_col.as<int32_t>(), PU.d_val.as<double2>(),
                              PU.d_piv.as<double2>()};
        subst_packed<false>(PL.width, fw, L.max_width, rhs, times_d ? M.dvec : nullptr, out, st);
        subst_packed<true>(PU.width, bw, U.max_width, out, nullptr, out, st);
        return;
    }
    const double2* keep = M.dvec;
    if (!times_d) M.dvec = nullptr;
    run_levels<ILU_FORWARD>(M, L, d_ordL.as<int32_t>(), d_ptrL.as<int32_t>(), rhs, out, st);
    run_levels<ILU_BACKWARD>(M, U, d_ordU.as<int32_t>(), d_ptrU.as<int32_t>(), rhs, out, st);
    M.dvec = keep;
}

hipError_t launch_csr_dinv(int n, const int32_t* p, const int32_t* ci, const double* vx, const double* vy, double2* dinv, hipStream_t st) {
    hipLaunchKernelGGL(k_csr_dinv, dim3(csr_nwg(n)), dim3(256), 0, st, n, p, ci, vx, vy, dinv, static_cast<double2*>(nullptr));
    return hipGetLastError();
}
hipError_t launch_csr_scaled_residual(int n, const int32_t* p, const int32_t* ci, const double* vx, const double* vy, const double2* dinv, const double2* in,
                                      const double2* b, double2* out, double* partials, hipStream_t st) {
    const CsrDev A{n, p, ci, vx, vy, dinv};
    hipLaunchKernelGGL((k_csr_apply<true, DOT_OUT2>), dim3(csr_nwg(n)), dim3(256), 0, st, A, in, b, static_cast<const double2*>(nullptr), out, partials);
    return hipGetLastError();
}
hipError_t launch_csr_scaled_residual_plain(int n, const int32_t* p, const int32_t* ci, const double* vx, const double* vy, const double2* dinv, const double2* in,
                                            const double2* b, double2* out, hipStream_t st) {
    const CsrDev A{n, p, ci, vx, vy, dinv};
    hipLaunchKernelGGL((k_csr_apply<true, DOT_NONE>), dim3(csr_nwg(n)), dim3(256), 0, st, A, in, b, static_cast<const double2*>(nullptr), out, static_cast<double*>(nullptr));
    return hipGetLastError();
}
hipError_t launch_csr_norm2(int n, const double2* v, double* partials, hipStream_t st) {
    hipLaunchKernelGGL(k_csr_norm2, dim3(csr_nwg(n)), dim3(256), 0, st, n, v, partials);
    return hipGetLastError();
}
hipError_t launch_csr_sub(int n, const double2* b, const double2* w, double2* r, hipStream_t st) {
    hipLaunchKernelGGL(k_csr_sub, dim3(csr_nwg(n)), dim3(256), 0, st, n, b, w, r);
    return hipGetLastError();
}
hipError_t launch_csr_diag_precond(int n, const double2* dinv, const double2* r, double2* z, hipStream_t st) {
    hipLaunchKernelGGL(k_csr_diag_precond, dim3(csr_nwg(n)), dim3(256), 0, st, n, dinv, r, z);
    return hipGetLastError();
}

}  // namespace tmh

using namespace tmh;

// diagnostic (include/tm_hip_diag.h): ILU(0) of one CSR matrix on the device -- the factor in A's pattern and M^-1 rhs -- for the bit-for-bit
// comparison with the reference's recurrence (tests/test_gpu_ilu0.py)
extern "C" int tm_csr_ilu0_probe(uint64_t n64, const int32_t* Ap, const int32_t* Ai, const double* Ax, const double* rhs, double* lu_out, double* z_out) {
    return guarded([&]() {
        if (!Ap || !Ai || !Ax || !lu_out) throw TmError(TM_E_ARG, "null argument");
        if (n64 == 0 || n64 >= (uint64_t{1} << 31)) throw TmError(TM_E_SIZE, "system size out of range");
        {
            int dev = 0;
            HIPCHK(hipGetDevice(&dev));
            hipDeviceProp_t prop;
            HIPCHK(hipGetDeviceProperties(&prop, dev));
            if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) throw TmError(TM_E_HIP, std::string("libtm_hip is built for gfx950 (MI355X) only, found ") + prop.gcnArchName);
        }
        const int n = static_cast<int>(n64);
        const size_t nnz = static_cast<size_t>(Ap[n]);
        DevBuf d_p(sizeof(int32_t) * (static_cast<size_t>(n) + 1), "csr p"), d_i(sizeof(int32_t) * nnz, "csr i"), d_v(sizeof(double) * nnz, "csr v");
        HIPCHK(hipMemcpy(d_p.p, Ap, sizeof(int32_t) * (static_cast<size_t>(n) + 1), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_i.p, Ai, sizeof(int32_t) * nnz, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_v.p, Ax, sizeof(double) * nnz, hipMemcpyHostToDevice));
        IluState ilu(n, Ap, Ai, nnz, false);
        ilu.factor(n, d_p.as<int32_t>(), d_i.as<int32_t>(), d_v.as<double>(), nullptr, nnz, nullptr, nullptr);
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(lu_out, ilu.d_lux.p, sizeof(double) * nnz, hipMemcpyDeviceToHost));
        if (rhs && z_out) {
            std::vector<double2> r2(static_cast<size_t>(n));
            for (int k = 0; k < n; ++k) r2[k] = make_double2(rhs[k], rhs[k]);
            DevBuf d_r(sizeof(double2) * static_cast<size_t>(n), "csr r"), d_z(sizeof(double2) * static_cast<size_t>(n), "csr z");
            HIPCHK(hipMemcpy(d_r.p, r2.data(), sizeof(double2) * r2.size(), hipMemcpyHostToDevice));
            ilu.apply(d_r.as<double2>(), d_z.as<double2>(), nullptr);
            HIPCHK(hipDeviceSynchronize());
            HIPCHK(hipMemcpy(r2.data(), d_z.p, sizeof(double2) * r2.size(), hipMemcpyDeviceToHost));
            for (int k = 0; k < n; ++k) z_out[k] = r2[k].x;
        }
        return TM_OK;
    });
}

extern "C" int tm_csr_solve(uint64_t n64, const int32_t* Ap, const int32_t* Ai, const double* Ax_x, const double* Ax_y, const double* bx,
                            const double* by, double* x, double* y, const tm_solver_opt* opt_in, tm_stats* stats) {
    return guarded([&]() {
        const auto t0 = std::chrono::steady_clock::now();
        if (!Ap || !Ai || !Ax_x || !bx || !by || !x || !y) throw TmError(TM_E_ARG, "null argument");
        if (n64 == 0 || n64 >= (uint64_t{1} << 31)) throw TmError(TM_E_SIZE, "system size out of range");
        if (opt_in && opt_in->tag != TM_SOLVER_HIP)
            throw TmError(TM_E_UNSUPPORTED, "ExternalSolverNotEnabled: libtm_hip serves only solver tag `hip`");
        const int n = static_cast<int>(n64);
        if (Ap[0] != 0 || Ap[n] < 0) throw TmError(TM_E_ARG, "InvalidMatrix: row pointers must start at 0");
        const size_t nnz = static_cast<size_t>(Ap[n]);
        for (int r = 0; r < n; ++r)
            if (Ap[r + 1] < Ap[r]) throw TmError(TM_E_ARG, "InvalidMatrix: row pointers must not decrease");
        for (size_t k = 0; k < nnz; ++k)
            if (Ai[k] < 0 || Ai[k] >= n) throw TmError(TM_E_ARG, "InvalidMatrix: column index out of range");
        tm_solver_opt opt;
        std::memset(&opt, 0, sizeof(opt));
        if (opt_in) opt = *opt_in;
        // 1e-14 at every size: the size-aware default of the matrix-free path belongs to ITS operator (the frozen Winslow system, whose
        // conditioning grows with the node count); this entry point takes any matrix the caller assembled
        if (!(opt.rtol > 0)) opt.rtol = 1e-14;
        if (!(opt.atol > 0)) opt.atol = 0.0;
        if (opt.max_inner == 0) opt.max_inner = default_max_inner(static_cast<double>(n));
        if (opt.check_every == 0) opt.check_every = (opt.flags & TM_OPT_PRECOND_ILU0) ? 1 : 8;   // an ILU(0) iteration is thousands of dependent steps: poll each

        int dev = 0;
        HIPCHK(hipGetDevice(&dev));
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, dev));
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) throw TmError(TM_E_HIP, std::string("libtm_hip is built for gfx950 (MI355X) only, found ") + prop.gcnArchName);

        const bool two = Ax_y != nullptr && Ax_y != Ax_x;
        const bool use_ilu = (opt.flags & TM_OPT_PRECOND_ILU0) != 0;
        const size_t vb = sizeof(double2) * static_cast<size_t>(n);
        DevBuf d_p(sizeof(int32_t) * (static_cast<size_t>(n) + 1), "csr p"), d_i(sizeof(int32_t) * nnz, "csr i"), d_vx(sizeof(double) * nnz, "csr vx"), d_vy(two ? sizeof(double) * nnz : 0, "csr vy");
        DevBuf d_dinv(vb, "csr dinv"), d_b(vb, "csr b"), d_u(vb, "csr u"), d_r(vb, "csr r"), d_rh(vb, "csr rh"), d_pv(vb, "csr pv"), d_v(vb, "csr v"), d_s(vb, "csr s"), d_t(vb, "csr t"), d_tmp(sizeof(double) * 2 * static_cast<size_t>(n), "csr tmp");
        const int nwg = (n + 255) / 256, nwg_vec = vec_nwg(n);
        // small systems are bound by dependent launches: the scalar steps travel with the kernels that consume them (LazyScalars,
        // tm_kernels.h; three partial-sum buffers in rotation, two scalar blocks) -- 5 launches per iteration instead of 9
        const int npart = std::max(nwg, nwg_vec);
        const bool lazy = npart <= 512 && !(opt.flags & TM_OPT_EAGER_SCALARS);
        DevBuf d_part(sizeof(double) * MAX_PARTIALS * static_cast<size_t>(npart) * (lazy ? 3 : 1), "csr part"), d_red(sizeof(double) * MAX_PARTIALS, "csr red"), d_S(sizeof(KrylovScalars) * 2, "csr S");
        hipStream_t st = nullptr;
        HIPCHK(hipMemcpyAsync(d_p.p, Ap, sizeof(int32_t) * (static_cast<size_t>(n) + 1), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_i.p, Ai, sizeof(int32_t) * nnz, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_vx.p, Ax_x, sizeof(double) * nnz, hipMemcpyHostToDevice, st));
        if (two) HIPCHK(hipMemcpyAsync(d_vy.p, Ax_y, sizeof(double) * nnz, hipMemcpyHostToDevice, st));
        double* tmp = d_tmp.as<double>();
        auto upload2 = [&](const double* a, const double* b, double2* out) {   // two host arrays -> one interleaved device vector
            HIPCHK(hipMemcpyAsync(tmp, a, sizeof(double) * n, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(tmp + n, b, sizeof(double) * n, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_interleave, dim3(nwg), dim3(256), 0, st, n, tmp, tmp + n, out);
            HIPCHK(hipGetLastError());
        };
        upload2(bx, by, d_b.as<double2>());
        upload2(x, y, d_u.as<double2>());   // warm start: the caller's x_new / y_new (BiCGStab.zig:136-153 seeds them from the coordinates)
        CsrDev A{n, d_p.as<int32_t>(), d_i.as<int32_t>(), d_vx.as<double>(), two ? d_vy.as<double>() : d_vx.as<double>(), d_dinv.as<double2>()};
        DevBuf d_dvec(use_ilu ? vb : 0, "csr dvec"), d_ph(use_ilu ? vb : 0, "csr ph"), d_sh(use_ilu ? vb : 0, "csr sh");
        hipLaunchKernelGGL(k_csr_dinv, dim3(nwg), dim3(256), 0, st, n, A.p, A.i, A.vx, A.vy, d_dinv.as<double2>(), use_ilu ? d_dvec.as<double2>() : nullptr);
        HIPCHK(hipGetLastError());
        // ILU(0) as RIGHT preconditioner (BiCGStab.zig:314-316, 340-342) of the row-equilibrated operator B = D^-1 A the device iterates on:
        // B P^-1 ~ I with P = D^-1 M, M = ILU(0)(A) factorised from the caller's values exactly as the reference does, so P^-1 v = M^-1 (D v)
        // -- the forward substitution multiplies its right-hand side by the diagonal.  The stop test stays the scale-aware one.
        std::unique_ptr<IluState> ilu;
        if (use_ilu) {
            ilu = std::make_unique<IluState>(n, Ap, Ai, nnz, two);
            ilu->factor(n, A.p, A.i, A.vx, two ? A.vy : nullptr, nnz, d_dvec.as<double2>(), st);
        }

        LazyScalarQueue lsq;   // (tm_krylov.hpp; no all-reduce: one process)
        lsq.lazy = lazy;
        lsq.stream = st;
        for (int k = 0; k < 3; ++k) lsq.part_buf[k] = d_part.as<double>() + (lazy ? k : 0) * MAX_PARTIALS * static_cast<size_t>(npart);
        lsq.partials = lsq.part_buf[0];
        lsq.red = d_red.as<double>();
        lsq.S_buf[0] = d_S.as<KrylovScalars>();
        lsq.S_buf[1] = lsq.S_buf[0] + 1;
        lsq.S = lsq.S_buf[0];
        HIPCHK(hipMemsetAsync(lsq.S_buf[0], 0, sizeof(KrylovScalars) * 2, st));
        double*& partials = lsq.partials;
        double* const red = lsq.red;
        KrylovScalars*& S = lsq.S;
        double2 *r = d_r.as<double2>(), *r_hat = d_rh.as<double2>(), *p = d_pv.as<double2>(), *v = d_v.as<double2>(),
                *s = d_s.as<double2>(), *t = d_t.as<double2>();
        // one solve of A u = bvec from the guess in u, stop test relative to ||D^-1 bvec||: the call's own solve and, with TM_OPT_REFINE, the
        // corrections behind it (bvec = the double-double residual, u = 0)
        struct SolveOut {
            bool converged = false;
            uint64_t iterations = 0, sweeps = 0;
            double rr0[2] = {0.0, 0.0};
        };
        const bool use_gmres = opt.inner == TM_INNER_GMRES;
        DevBuf d_W(use_gmres ? vb : 0, "csr W"), d_V(use_gmres ? vb * (GMRES_M + 1) : 0, "csr V"), d_G(use_gmres ? sizeof(GmresScalars) : 0, "csr G");
        auto solve = [&](const double2* bvec, double2* u, double rtol) -> SolveOut {
        SolveOut out;
        hipLaunchKernelGGL(k_csr_bnorm, dim3(nwg), dim3(256), 0, st, n, bvec, A.dinv, partials);
        HIPCHK(hipGetLastError());
        HIPCHK(launch_finalize_scalar(partials, nwg, red, S, STEP_TOL, st, rtol, opt.atol));

        if (use_gmres) {
            // The reference's other Krylov solver in the slot (GMRES.zig:300-423; csrc/tm_gmres.hip for the kernels): restarted GMRES(30), LEFT
            // preconditioned (GMRES.zig:335-336: z = M^-1 (A v)) with the diagonal -- the row-equilibrated operator the BiCGStab branch uses --
            // or with ILU(0): M^-1 A v = M^-1 (D (D^-1 A v)), the substitution multiplying its right-hand side by the diagonal.  Stop test:
            // GMRES's own residual norm |g_{j+1}| = ||P (b - A x)|| <= max(atol, rtol ||P b||), P the preconditioner (with the diagonal: the
            // scale-aware test of every other path).
            double2 *W = d_W.as<double2>(), *V = d_V.as<double2>();
            GmresScalars* G = d_G.as<GmresScalars>();
            HIPCHK(hipMemsetAsync(G, 0, sizeof(GmresScalars), st));
            HIPCHK(hipMemsetAsync(V, 0, vb * (GMRES_M + 1), st));
            const GmresSpace g{G, V, n, W, n, partials, red, st};
            auto norm2_of = [&](const double2* v) {
                hipLaunchKernelGGL(k_csr_norm2, dim3(nwg), dim3(256), 0, st, n, v, partials);
                HIPCHK(hipGetLastError());
                HIPCHK(launch_finalize(partials, nwg, red, st));
            };
            if (use_ilu) {
                ilu->apply(bvec, W, st, false);   // M^-1 b
                norm2_of(W);
            } else {
                hipLaunchKernelGGL(k_csr_bnorm, dim3(nwg), dim3(256), 0, st, n, bvec, A.dinv, partials);
                HIPCHK(hipGetLastError());
                HIPCHK(launch_finalize(partials, nwg, red, st));
            }
            HIPCHK(launch_gm_tol(G, red, rtol, opt.atol, st));
            GmresScalars h_G;
            auto poll = [&]() {
                HIPCHK(hipMemcpyAsync(&h_G, G, sizeof(GmresScalars), hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
                return h_G.done[0] == 1 && h_G.done[1] == 1;
            };
            auto apply_op = [&](const double2* vj, double2* w) {
                hipLaunchKernelGGL((k_csr_apply<false, DOT_NONE>), dim3(nwg), dim3(256), 0, st, A, vj, nullptr, nullptr, w, partials);   // D^-1 A v_j
                HIPCHK(hipGetLastError());
                if (use_ilu) ilu->apply(w, w, st);
            };
            uint64_t it_total = 0;
            bool converged = false, first = true;
            double rr0[2] = {0.0, 0.0};
            while (it_total < opt.max_inner) {
                hipLaunchKernelGGL((k_csr_apply<true, DOT_OUT2>), dim3(nwg), dim3(256), 0, st, A, u, bvec, nullptr, W, partials);   // D^-1 (b - A x)
                HIPCHK(hipGetLastError());
                if (use_ilu) {
                    ilu->apply(W, W, st);   // M^-1 (b - A x)
                    norm2_of(W);
                } else {
                    HIPCHK(launch_finalize(partials, nwg, red, st));
                }
                HIPCHK(launch_gm_begin(G, red, st));
                converged = poll();
                if (first) {
                    rr0[0] = h_G.rr0[0];
                    rr0[1] = h_G.rr0[1];
                    first = false;
                }
                if (converged) break;
                converged = gmres_cycle(g, u, apply_op, [&] { HIPCHK(launch_finalize(partials, nwg_vec, red, st)); }, poll, opt.check_every, it_total, opt.max_inner);
                if (converged) break;
            }
            out.converged = converged;
            out.iterations = it_total;
            out.sweeps = it_total + (it_total + GMRES_M - 1) / GMRES_M + 1;
            out.rr0[0] = rr0[0];   // of P (b - A x0), P the preconditioner
            out.rr0[1] = rr0[1];
            return out;
        }

        KrylovScalars h_S;
        auto read_S = [&]() {
            lsq.flush();
            HIPCHK(hipMemcpyAsync(&h_S, S, sizeof(KrylovScalars), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        };
        uint64_t it_total = 0;
        int restarts = 0;
        bool converged = false;
        double rr0[2] = {0.0, 0.0};
        StallWatch stall;   // runs without ILU(0) only
        stall.window = StallWatch::window_for(static_cast<double>(n));
        // with ILU(0): the preconditioned recurrence, the substitutions where the handle's mg_bicgstab has its multigrid cycle
        const BicgVectors w{r, p, v, s, t, use_ilu ? d_ph.as<double2>() : p, use_ilu ? d_sh.as<double2>() : s, r_hat, n, nwg_vec};
        auto precond = [&](const double2* in, double2* out) { ilu->apply(in, out, st); };
        auto apply_op = [&](const double2* in, double2* out, int dot, const double2* aux, int step) {
            const auto kernel = dot == DOT_AUX ? k_csr_apply<false, DOT_AUX> : (dot == DOT_AUX2 ? k_csr_apply<false, DOT_AUX2> : k_csr_apply<false, DOT_IN>);
            hipLaunchKernelGGL(kernel, dim3(nwg), dim3(256), 0, st, A, in, nullptr, aux, out, partials);
            HIPCHK(hipGetLastError());
            lsq.reduce_update(nwg, step);
        };
        while (true) {
            hipLaunchKernelGGL((k_csr_apply<true, DOT_OUT2>), dim3(nwg), dim3(256), 0, st, A, u, bvec, nullptr, r, partials);
            HIPCHK(hipGetLastError());
            lsq.flush();
            HIPCHK(launch_finalize_scalar(partials, nwg, red, S, STEP_INIT, st));
            HIPCHK(hipMemcpyAsync(r_hat, r, vb, hipMemcpyDeviceToDevice, st));
            HIPCHK(hipMemsetAsync(p, 0, vb, st));
            HIPCHK(hipMemsetAsync(v, 0, vb, st));
            if (restarts == 0) {
                read_S();
                rr0[0] = h_S.rr0[0];
                rr0[1] = h_S.rr0[1];
                if (h_S.done[0] == 1 && h_S.done[1] == 1) {
                    converged = true;
                    break;
                }
            }
            bool breakdown = false;
            while (it_total < opt.max_inner) {
                bicgstab_direction(lsq, w, precond, apply_op);
                bicgstab_correction(lsq, w, u, precond, apply_op);
                it_total += 1;
                if (it_total % opt.check_every == 0 || it_total == opt.max_inner) {
                    read_S();
                    if (h_S.done[0] && h_S.done[1]) {
                        converged = h_S.done[0] == 1 && h_S.done[1] == 1;
                        breakdown = !converged;
                        break;
                    }
                    if (!use_ilu && stall.observe(h_S, it_total)) break;
                }
            }
            if (converged || !breakdown || stall.stalled || restarts >= 8 || it_total >= opt.max_inner) break;
            restarts += 1;   // rho or omega vanished: restart from the current iterate (the reference only warns, BiCGStab.zig:368-369)
        }
        lsq.drop();   // scalar steps still pending belong to an iteration nobody reads
        out.converged = converged;
        out.iterations = it_total;
        out.sweeps = 1 + static_cast<uint64_t>(restarts) + 2 * it_total;
        out.rr0[0] = rr0[0];
        out.rr0[1] = rr0[1];
        return out;
        };

        double2* const u = d_u.as<double2>();
        const SolveOut first = solve(d_b.as<double2>(), u, opt.rtol);
        uint64_t it_total = first.iterations, sweeps = first.sweeps;
        if (opt.flags & TM_OPT_REFINE) {
            // Iterative refinement (tm_refine.hpp): r = b - A u in double-double, A d = r from d = 0 by the same solver and preconditioner with
            // the stop test relative to ||D^-1 r||, u += d; at most REFINE_MAX_STEPS times, one poll (four sums) per step.
            // The corrections keep the call's own rtol: 1e-8 was tried and costs the flat 1e-10 bar on T106;
            // TM_REFINE_RTOL in the environment overrides it, for measurement.
            double rtol_c = opt.rtol;
            if (const char* e = std::getenv("TM_REFINE_RTOL"))
                if (std::atof(e) > 0.0) rtol_c = std::atof(e);
            DevBuf d_rr(vb, "csr rr"), d_d(vb, "csr d");
            double h_red[MAX_PARTIALS] = {0.0};
            uint32_t steps = 0;
            uint64_t it_corr = 0;
            double rel[2] = {0.0, 0.0};
            for (int q = 0; q < REFINE_MAX_STEPS; ++q) {
                HIPCHK(launch_csr_residual_dd(n, A.p, A.i, A.vx, A.vy, u, d_b.as<double2>(), d_rr.as<double2>(), st));
                HIPCHK(hipMemsetAsync(d_d.p, 0, vb, st));
                HIPCHK(hipMemsetAsync(lsq.S_buf[0], 0, sizeof(KrylovScalars) * 2, st));
                const SolveOut c = solve(d_rr.as<double2>(), d_d.as<double2>(), rtol_c);
                it_corr += c.iterations;
                sweeps += c.sweeps + 1;
                HIPCHK(launch_refine_update(n, u, d_d.as<double2>(), lsq.part_buf[0], st));
                HIPCHK(launch_finalize(lsq.part_buf[0], nwg, red, st));
                HIPCHK(hipMemcpyAsync(h_red, red, sizeof(double) * MAX_PARTIALS, hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
                steps += 1;
                for (int c2 = 0; c2 < 2; ++c2) rel[c2] = h_red[2 + c2] > 0.0 ? std::sqrt(h_red[c2] / h_red[2 + c2]) : (h_red[c2] > 0.0 ? HUGE_VAL : 0.0);
                if (refine_converged(h_red)) break;
            }
            it_total += it_corr;
            if (const tm_log_fn sink = g_log_sink) {
                sink(g_log_ctx, 2, 0, static_cast<double>(steps));
                sink(g_log_ctx, 3, 0, rel[0]);
                sink(g_log_ctx, 4, 0, rel[1]);
                sink(g_log_ctx, 5, 0, static_cast<double>(it_corr));
            }
        }
        hipLaunchKernelGGL(k_deinterleave, dim3(nwg), dim3(256), 0, st, n, u, tmp, tmp + n);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(x, tmp, sizeof(double) * n, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(y, tmp + n, sizeof(double) * n, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (stats) {
            std::memset(stats, 0, sizeof(*stats));
            stats->outer_iterations = 1;
            stats->inner_iterations = it_total;
            stats->operator_sweeps = sweeps;
            stats->scaled_residual_rms = std::sqrt((first.rr0[0] + first.rr0[1]) / (2.0 * n));
            stats->not_converged = first.converged ? 0 : 1;
            stats->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        }
        return first.converged ? TM_OK : TM_W_NOT_CONVERGED;
    });
}

// r = b - A x of a caller's system by k_csr_residual_dd (tm_refine.hip): the check a user runs on any solution
extern "C" int tm_csr_residual(uint64_t n64, const int32_t* Ap, const int32_t* Ai, const double* Ax_x, const double* Ax_y, const double* bx, const double* by,
                               const double* x, const double* y, double* rx, double* ry) {
    return guarded([&]() {
        if (!Ap || !Ai || !Ax_x || !bx || !by || !x || !y || !rx || !ry) throw TmError(TM_E_ARG, "null argument");
        if (n64 == 0 || n64 >= (uint64_t{1} << 31)) throw TmError(TM_E_SIZE, "system size out of range");
        const int n = static_cast<int>(n64);
        if (Ap[0] != 0 || Ap[n] < 0) throw TmError(TM_E_ARG, "InvalidMatrix: row pointers must start at 0");
        const size_t nnz = static_cast<size_t>(Ap[n]);
        for (int r = 0; r < n; ++r)
            if (Ap[r + 1] < Ap[r]) throw TmError(TM_E_ARG, "InvalidMatrix: row pointers must not decrease");
        for (size_t k = 0; k < nnz; ++k)
            if (Ai[k] < 0 || Ai[k] >= n) throw TmError(TM_E_ARG, "InvalidMatrix: column index out of range");
        int dev = 0;
        HIPCHK(hipGetDevice(&dev));
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, dev));
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) throw TmError(TM_E_HIP, std::string("libtm_hip is built for gfx950 (MI355X) only, found ") + prop.gcnArchName);

        const bool two = Ax_y != nullptr && Ax_y != Ax_x;
        const size_t vb = sizeof(double2) * static_cast<size_t>(n);
        DevBuf d_p(sizeof(int32_t) * (static_cast<size_t>(n) + 1), "csr p"), d_i(sizeof(int32_t) * nnz, "csr i"), d_vx(sizeof(double) * nnz, "csr vx"), d_vy(two ? sizeof(double) * nnz : 0, "csr vy");
        DevBuf d_b(vb, "csr b"), d_u(vb, "csr u"), d_tmp(sizeof(double) * 2 * static_cast<size_t>(n), "csr tmp");
        const int nwg = csr_nwg(n);
        hipStream_t st = nullptr;
        HIPCHK(hipMemcpyAsync(d_p.p, Ap, sizeof(int32_t) * (static_cast<size_t>(n) + 1), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_i.p, Ai, sizeof(int32_t) * nnz, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_vx.p, Ax_x, sizeof(double) * nnz, hipMemcpyHostToDevice, st));
        if (two) HIPCHK(hipMemcpyAsync(d_vy.p, Ax_y, sizeof(double) * nnz, hipMemcpyHostToDevice, st));
        double* tmp = d_tmp.as<double>();
        auto upload2 = [&](const double* a, const double* b, double2* out) {   // two host arrays -> one interleaved device vector
            HIPCHK(hipMemcpyAsync(tmp, a, sizeof(double) * n, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(tmp + n, b, sizeof(double) * n, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_interleave, dim3(nwg), dim3(256), 0, st, n, tmp, tmp + n, out);
            HIPCHK(hipGetLastError());
        };
        upload2(bx, by, d_b.as<double2>());
        upload2(x, y, d_u.as<double2>());
        HIPCHK(launch_csr_residual_dd(n, d_p.as<int32_t>(), d_i.as<int32_t>(), d_vx.as<double>(), two ? d_vy.as<double>() : d_vx.as<double>(), d_u.as<double2>(),
                                      d_b.as<double2>(), d_b.as<double2>(), st));   // in place: a row reads its own b before it stores
        hipLaunchKernelGGL(k_deinterleave, dim3(nwg), dim3(256), 0, st, n, d_b.as<double2>(), tmp, tmp + n);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(rx, tmp, sizeof(double) * n, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(ry, tmp + n, sizeof(double) * n, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return TM_OK;
    });
}
