// Spanwise stacking of 2-D cuts into 3-D blocks (include/tm_hip.h, "3-D from 2-D cuts"): what the host part (tm_stack_host.cpp:
// validation, weights, the CPU evaluation) and the device part (tm_stack.hip: K11 and its entry points) share.
#pragma once
#include "../../include/tm_hip.h"

#include <cstdint>
#include <vector>

struct tm_smoother;

namespace tmh {

// validated options of one call: the weight rows of the window and what the mapping needs
struct StackPlan {
    int ncuts = 0;
    int mapping = TM_STACK_PLANAR;
    uint64_t nlayers = 0;
    std::vector<double> span;      // z[ncuts]
    std::vector<double> weights;   // nlayers * ncuts, row = layer
    std::vector<double> layers;    // s[nlayers]
};

// throws TmError(TM_E_ARG) on any violation of the definition (TM_STACK_REVOLUTION included: these calls have no tables)
StackPlan stack_plan(const tm_stack_opt* opt);

// validated meridional tables of a TM_STACK_REVOLUTION call ("cuts on stream surfaces of revolution")
struct SurfPlan {
    std::vector<int> nknots;     // N_c
    std::vector<int> first;      // index of cut c's first knot in `knots`; its first coefficient is (first[c] - c) * 8 into `coef`
    std::vector<double> knots;   // u, cut after cut
    std::vector<double> coef;    // ax bx cx dx ar br cr dr per interval, cut after cut (what tm_stack_surface_tables returns)
    std::vector<double> rref;    // [ncuts]
};
// the plan of a *_surf call: TM_E_ARG unless opt->mapping == TM_STACK_REVOLUTION and the tables are as the header says
StackPlan stack_plan_surf(const tm_stack_opt* opt, const tm_stack_surfaces* surfaces, SurfPlan& surf);
// x_c, r_c, theta_c of every node of the block (node (i,j) at i*nj + j), cut c at c*ni*nj; outside[c] when given
void stack_surf_nodes_host(const StackPlan& plan, const SurfPlan& surf, const double* const* v, uint64_t ni, uint64_t nj, std::vector<double>& x,
                           std::vector<double>& r, std::vector<double>& th, uint64_t* outside);
// layer k from them: the planes X, R sin Theta, R cos Theta, element j*ni + i
void stack_layer_surf_host(const StackPlan& plan, const std::vector<double>& xc, const std::vector<double>& rc, const std::vector<double>& thc, uint64_t k,
                           uint64_t ni, uint64_t nj, double* x, double* y, double* z);
// TM_E_ARG unless [k_begin, k_begin + k_count) is a non-empty window of the plan's layers
void stack_check_window(const StackPlan& plan, uint64_t k_begin, uint64_t k_count);
// block `block` of the K descriptions: TM_E_ARG / TM_E_SIZE as the header says; returns (ni, nj)
void stack_check_cuts(const tm_mesh_desc* const* cuts, int ncuts, uint64_t block, uint64_t* ni, uint64_t* nj);

// layer k of the plan from the K cuts v[c] (node (i,j) at i*nj + j, interleaved x y): one plane each of x, y, z, element j*ni + i.
// The definition as a plain loop, summed over c = 0 .. K-1 like the kernel (tm_stack_block_host, tm_stack_quality_host)
void stack_layer_host(const StackPlan& plan, const double* const* v, uint64_t k, uint64_t ni, uint64_t nj, double* x, double* y, double* z);
// what the 3-D quality calls ask on top of the stacking calls: TM_E_SIZE unless the stack has cells
void stack_check_cells(const StackPlan& plan, uint64_t ni, uint64_t nj);

// live handles of the process (tm_api.cpp: entered by tm_smoother_create, removed by tm_smoother_destroy)
bool smoother_is_live(const tm_smoother* s);

}  // namespace tmh
