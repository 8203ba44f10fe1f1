// Iterative refinement of a solve on an assembled CSR system (csrc/tm_refine.hip): the residual r = b - A x of both components in
// double-double arithmetic, rounded once to fp64, and the update x <- x + d with the norms the stop test of the refinement loop reads.
// Serves the two CSR layouts of the library through plain device pointers: the caller's system of tm_csr_solve (CsrDev, tm_csr.hip) and the
// handle's reference-order system (Smoother::AssembledCsr with the device right-hand side of picard_reference).
//
// VALID DOMAIN of the residual: finite inputs whose products a_ij * x_j neither overflow nor fall into the subnormal range (the error term
// fma(a, x, -a*x) of a product is exact only while it is representable).  Inside it every row satisfies
//     |r - (b - A x)_exact| <= 2^-53 |r| + (nnz + 1) 2^-104 (sum_j |a_ij x_j| + |b_i|)
// whatever the cancellation.  Outside it the result is the fp64 residual's, with no promise beyond that.
#pragma once
#include "tm_kernels.h"

namespace tmh {

constexpr int REFINE_MAX_STEPS = 3;   // refinement steps behind one inner solve (TM_OPT_REFINE)

// r = b - A x per component, one thread per row, 256 rows per workgroup; rows of any length, empty ones included.  vy == vx: one matrix
// for both components.  r may be b (a row reads its own b before it stores and nothing else of it); x must not alias r.
hipError_t launch_csr_residual_dd(int n, const int32_t* p, const int32_t* ci, const double* vx, const double* vy, const double2* x, const double2* b,
                                  double2* r, hipStream_t st);
// x += d in fp64; partials (one row of MAX_PARTIALS per workgroup, 256 rows each): ||d||^2 (x, y), ||x + d||^2 (x, y)
hipError_t launch_refine_update(int n, double2* x, const double2* d, double* partials, hipStream_t st);
// the step's verdict from the four sums above: ||d||_2 <= 2^-52 ||x||_2 in both components
inline bool refine_converged(const double* red) {
    const double u = 0x1p-52;
    return red[0] <= u * u * red[2] && red[1] <= u * u * red[3];
}

}  // namespace tmh
