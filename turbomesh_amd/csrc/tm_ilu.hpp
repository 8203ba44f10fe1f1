// ILU(0) of an assembled CSR system on the device, and the few CSR vector kernels around it (csrc/tm_csr.hip) -- shared by the linear-solver
// slot (tm_csr_solve, tm_csr_ilu0_probe) and by the handle's TM_INNER_REFERENCE_GMRES mode (Smoother::picard_reference), which keeps one
// IluState for its lifetime: analysis once, factorisation per outer iteration, two substitutions per inner iteration.
#pragma once
#include "tm_devbuf.hpp"
#include <array>
#include <vector>

namespace tmh {

struct IluDev {
    int n;
    const int32_t *p, *ci, *diag_pos;
    double *lux, *luy;       // the factors, in the pattern of A (unit lower part below the diagonal, U on and above it); luy == lux: one system
    const double2* dvec;     // a_ii per row and component: the forward substitution multiplies its right-hand side by it (see IluState::apply)
};

// host side: level sets of the lower (factorisation, forward substitution) and of the upper (backward substitution) dependency graph
struct IluLevels {
    std::vector<int32_t> order, ptr;              // rows sorted by level; ptr[l] .. ptr[l+1]
    std::vector<std::array<int, 2>> chunks;       // launches: [lv0, lv1); a chunk of several levels has only levels of <= 256 rows
    int max_width = 0;                            // rows of the widest level
    void build(int n, const int32_t* p, const int32_t* ci, bool lower);
};

// One substitution direction in level-packed form (k_ilu_subst_packed): position k = the k-th row in level order; slot s of that row at
// s * n + k, the row's strictly-lower (resp. strictly-upper) entries in CSR order -- the summation order is the bit-identity contract.
struct IluPackedDev {
    int n, nlev;
    const int32_t *ptr, *order;   // level pointers [nlev + 1], row of position k
    const int32_t* col;           // [width * n] column of the slot, -1 = the row has no such entry
    const double2* val;           // [width * n] (lux, luy) of the slot, refilled after every factorisation
    const double2* piv;           // [n] backward pass: the pivots (a zero or missing one counts as 1)
};
struct IluPacked {
    int width = 0;                // slots per row = the most entries any row has on this side of the diagonal; rounded up to 4, 8 or 16
    DevBuf d_col, d_src, d_val, d_piv;   // allocated by build()
    void build(int n, const int32_t* p, const int32_t* ci, const IluLevels& lv, bool lower);
};

// analysis on the host, factorisation level by level (k_ilu_levels), the two substitutions on the level-packed form
struct IluState {
    IluLevels L, U;
    DevBuf d_diag, d_lux, d_luy, d_ordL, d_ptrL, d_ordU, d_ptrU;
    IluPacked PL, PU;
    bool packed = false;          // false: a row has more than 16 entries on one side, or TM_ILU_PACKED=0 -- substitutions by k_ilu_levels
    IluDev M{};
    int n = 0;
    // use_packed: 1 / 0 = substitutions on the packed form / by k_ilu_levels; -1 = packed unless TM_ILU_PACKED=0 is in the environment
    IluState(int n, const int32_t* Ap, const int32_t* Ai, size_t nnz, bool two, int use_packed = -1);
    // the factor of (vx, vy) -- device arrays in A's pattern -- into lux / luy
    void factor(int n, const int32_t* d_p, const int32_t* d_i, const double* d_vx, const double* d_vy, size_t nnz, const double2* dvec, hipStream_t st);
    // out = U^-1 L^-1 (dvec .* rhs)   (dvec == nullptr in M: plain M^-1 rhs, BiCGStab.zig:384-422)
    // times_d = false: plain M^-1 rhs whatever dvec the state was factorised with.  rhs == out is fine (a row reads its own right-hand side
    // before it stores, and nothing else of rhs)
    void apply(const double2* rhs, double2* out, hipStream_t st, bool times_d = true);
};

// ---- CSR vector kernels, 256 rows per workgroup; partials: one row of MAX_PARTIALS per workgroup, csr_nwg(n) of them
inline int csr_nwg(int64_t n) { return static_cast<int>((n + 255) / 256); }
// dinv = 1 / a_ii per row and component, a missing or zero diagonal scales by 1 (BiCGStab.zig:155-175)
hipError_t launch_csr_dinv(int n, const int32_t* p, const int32_t* ci, const double* vx, const double* vy, double2* dinv, hipStream_t st);
// out = D^-1 (b - A in), partials: ||out||^2 per component
hipError_t launch_csr_scaled_residual(int n, const int32_t* p, const int32_t* ci, const double* vx, const double* vy, const double2* dinv, const double2* in,
                                      const double2* b, double2* out, double* partials, hipStream_t st);
// the same without the norm -- the fp64 residual kernel the double-double one is timed against (tools/refine_timing.py)
hipError_t launch_csr_scaled_residual_plain(int n, const int32_t* p, const int32_t* ci, const double* vx, const double* vy, const double2* dinv, const double2* in,
                                            const double2* b, double2* out, hipStream_t st);
hipError_t launch_csr_norm2(int n, const double2* v, double* partials, hipStream_t st);   // partials: ||v||^2 per component
hipError_t launch_csr_sub(int n, const double2* b, const double2* w, double2* r, hipStream_t st);          // r = b - w (GMRES.zig:313-315)
hipError_t launch_csr_diag_precond(int n, const double2* dinv, const double2* r, double2* z, hipStream_t st);   // z = r * dinv (GMRES.zig:427-430)

}  // namespace tmh
