// The inner solvers' recurrences, each written once (internal): the lazy scalar queue and the stagnation watch of the BiCGStab solves, the
// textbook BiCGStab iteration in two halves, one restart cycle of GMRES(30).  What differs between the smoother handle, its refinement
// corrections and the CSR slot -- operator, preconditioner, reduction, poll -- comes in as callables; nothing here allocates.
#pragma once
#include "tm_kernels.h"
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <functional>

namespace tmh {

void hip_check(hipError_t e, const char* what);
#define TM_KRYLOV_CHK(x) hip_check((x), #x)

// The Krylov scalar block and the partial sums that feed it.  Small single-process systems are bound by dependent launches, so a scalar
// step gets no launch of its own (LazyScalars, tm_kernels.h): it waits here, at most two at a time, for the kernel that reads the scalars
// (scalars_for), which applies it and publishes the result to the other scalar block.  Three partial-sum buffers in rotation: a buffer a
// pending step refers to is read by the consumer's workgroups, the next producer writes elsewhere.  The owner sets the pointers;
// part_buf[1..2] and S_buf[1] are used only when `lazy`.
struct LazyScalarQueue {
    bool lazy = false;
    hipStream_t stream = nullptr;
    double* part_buf[3] = {nullptr, nullptr, nullptr};
    double* partials = nullptr;   // where the next producer writes its partial rows
    double* red = nullptr;
    KrylovScalars* S_buf[2] = {nullptr, nullptr};
    KrylovScalars* S = nullptr;   // the current scalar block
    std::function<void(int)> all_reduce;   // set on multi-rank handles: partials -> red summed over all ranks; every step is then eager

    // the partial rows just written feed scalar step `step`; STEP_TOL is never lazy
    void reduce_update(int nwg, int step, double rtol = 0.0, double atol = 0.0) {
        if (all_reduce) {   // the sums of all ranks are needed before the scalars can move
            all_reduce(nwg);
            TM_KRYLOV_CHK(launch_scalar_update(S, red, step, stream, rtol, atol));
            return;
        }
        if (lazy && step != STEP_TOL) {   // no launch: the step waits for the kernel that needs its result (scalars_for)
            if (npending == 2) flush();
            pending[npending++] = LazyStep{step, partials, nwg};
            part_rot = (part_rot + 1) % 3;
            partials = part_buf[part_rot];
            return;
        }
        flush();
        TM_KRYLOV_CHK(launch_finalize_scalar(partials, nwg, red, S, step, stream, rtol, atol));
    }
    // pending steps applied by their own launches (before the host reads the scalars, or a step that cannot wait)
    void flush() {
        for (int q = 0; q < npending; ++q) TM_KRYLOV_CHK(launch_finalize_scalar(pending[q].partials, pending[q].nwg, red, S, pending[q].step, stream));
        npending = 0;
    }
    void drop() { npending = 0; }   // pending steps of an iteration nobody reads
    // the scalars for a kernel that reads them: with pending steps, the kernel applies them itself and publishes the result to the
    // other scalar block, which is the current one from then on
    LazyScalars scalars_for() {
        LazyScalars L;
        L.S_in = S;
        if (npending == 0) return L;
        KrylovScalars* other = (S == S_buf[0]) ? S_buf[1] : S_buf[0];
        L.S_out = other;
        L.nsteps = npending;
        for (int q = 0; q < npending; ++q) L.st[q] = pending[q];
        npending = 0;
        S = other;
        return L;
    }

   private:
    LazyStep pending[2] = {{0, nullptr, 0}, {0, nullptr, 0}};
    int npending = 0, part_rot = 0;
};

// Stagnation watch of a diagonal-only BiCGStab solve: its default tolerance lies below the TRUE residual fp64 can reach (it is met by the
// recurrence residual drifting down: DESIGN.md section 5); should the recurrence residual of an active component ever fail to halve over
// max(4000, 4 sqrt(dof)) iterations, the solve is over -- reported as not converged (a warning), without a restart, instead of running to
// the iteration cap.
struct StallWatch {
    double best[2] = {0.0, 0.0};   // best ||r||^2 per component
    uint64_t since = 0, window = 4000;   // iteration of the last halving
    bool stalled = false;
    static uint64_t window_for(double dof) { return std::max<uint64_t>(4000, static_cast<uint64_t>(4.0 * std::sqrt(dof))); }
    void reset() {
        best[0] = best[1] = 0.0;
        since = 0;
        stalled = false;
    }
    // the scalars as they stood after iteration `at`; true = stalled.  `at > since`: a pipelined poll examines its copies one poll late and may
    // see an iteration that is not past the last halving (a blocking poll never does: there the test changes nothing)
    bool observe(const KrylovScalars& h, uint64_t at) {
        bool progress = false;
        for (int c = 0; c < 2; ++c) {
            if (h.done[c]) continue;
            if (!(best[c] > 0.0) || h.rr[c] < 0.25 * best[c]) {   // ||r||^2 down by 4 = the norm halved
                best[c] = h.rr[c];
                progress = true;
            }
        }
        if (progress) since = at;
        else if (at > since && at - since > window) stalled = true;
        return stalled;
    }
};

// The vectors of a BiCGStab solve.  p_hat / s_hat: the preconditioned directions; p / s themselves without a preconditioner.
struct BicgVectors {
    double2 *r, *p, *v, *s, *t, *p_hat, *s_hat;
    const double2* r_hat;
    int64_t n;
    int nwg_vec;
};

// The textbook BiCGStab iteration (one kernel per vector update) in two halves -- picard_bicgstab can take the first fused and the second not.
//   precondition(in, out): out = M^-1 in, called only when the solve has preconditioned directions
//   apply_op(in, out, dot, aux, step): out = A in with the partial sums `dot` (against `aux`) feeding scalar step `step`
// Direction half: p = r + beta (p - omega v), v = A M^-1 p, sigma = r_hat . v.
template <class Precond, class ApplyOp>
void bicgstab_direction(LazyScalarQueue& q, const BicgVectors& w, Precond&& precondition, ApplyOp&& apply_op) {
    TM_KRYLOV_CHK(launch_p_update(q.scalars_for(), w.r, w.p, w.v, w.n, w.nwg_vec, q.stream));
    if (w.p_hat != w.p) precondition(w.p, w.p_hat);   // right preconditioning (BiCGStab.zig:314-316, 340-342)
    apply_op(w.p_hat, w.v, DOT_AUX, w.r_hat, STEP_SIGMA);
}
// Correction half: s = r - alpha v, t = A M^-1 s, u += alpha p_hat + omega s_hat, r = s - omega t, the next rho.
template <class Precond, class ApplyOp>
void bicgstab_correction(LazyScalarQueue& q, const BicgVectors& w, double2* u, Precond&& precondition, ApplyOp&& apply_op) {
    TM_KRYLOV_CHK(launch_s_update(q.scalars_for(), w.r, w.v, w.s, w.n, w.nwg_vec, q.partials, q.stream));
    q.reduce_update(w.nwg_vec, STEP_SS);
    if (w.s_hat != w.s) {
        precondition(w.s, w.s_hat);
        apply_op(w.s_hat, w.t, DOT_AUX2, w.s, STEP_TSTT);   // t.s and t.t with the UNpreconditioned s
    } else {
        apply_op(w.s, w.t, DOT_IN, nullptr, STEP_TSTT);
    }
    TM_KRYLOV_CHK(launch_xr_update(q.scalars_for(), u, w.p_hat, w.s_hat, w.s, w.t, w.r, w.r_hat, w.n, w.nwg_vec, q.partials, q.stream));
    q.reduce_update(w.nwg_vec, STEP_RHO);
}

// The state of a GMRES(30) solve (csrc/tm_gmres.hip): scalars, the m + 1 basis vectors (leading dimension ld), the work vector
struct GmresSpace {
    GmresScalars* G;
    double2* V;
    int64_t ld;
    double2* W;
    int64_t n;
    double* partials;
    const double* red;
    hipStream_t stream;
    double2* v(int k) const { return V + static_cast<int64_t>(k) * ld; }
};

// One restart cycle (GMRES.zig:321-417) behind the caller's restart residual z in W and launch_gm_begin: v0 = z / beta, the columns, then
// the triangular solve and u += V y.  Returns whether a poll saw both components finished.
//   apply_op(v_j, W): W = M^-1 A v_j (and whatever the caller counts per application)
//   reduce():         partials (vec_nwg(n) rows) -> red, over all ranks where there are several
//   poll():           true = both components are done, after everything enqueued so far
// `it` counts the columns of the whole solve and stops the cycle at `max_it`.
template <class ApplyOp, class Reduce, class Poll>
bool gmres_cycle(const GmresSpace& g, double2* u, ApplyOp&& apply_op, Reduce&& reduce, Poll&& poll, uint32_t check_every, uint64_t& it, uint64_t max_it) {
    TM_KRYLOV_CHK(launch_gm_divide(g.v(0), g.W, g.G, g.n, g.stream));
    bool done = false;
    for (int j = 0; j < GMRES_M && it < max_it && !done; ++j) {
        apply_op(g.v(j), g.W);
        // modified Gram-Schmidt (GMRES.zig:338-345): h_ij = z . v_i, z -= h_ij v_i, i = 0 .. j -- the subtraction of step i - 1 and
        // the inner product of step i in one pass each; then h_{j+1,j} = ||z|| behind the last subtraction
        TM_KRYLOV_CHK(launch_gm_mgs(g.W, nullptr, g.v(0), nullptr, g.G, 0, g.n, g.partials, g.stream));
        reduce();
        for (int i = 1; i <= j; ++i) {
            TM_KRYLOV_CHK(launch_gm_mgs(g.W, g.v(i - 1), g.v(i), g.red, g.G, i - 1, g.n, g.partials, g.stream));
            reduce();
        }
        TM_KRYLOV_CHK(launch_gm_mgs(g.W, g.v(j), nullptr, g.red, g.G, j, g.n, g.partials, g.stream));
        reduce();
        TM_KRYLOV_CHK(launch_gm_column(g.G, g.red, g.stream));                  // rotations, g, |g_{j+1}|, flags (GMRES.zig:347-386)
        TM_KRYLOV_CHK(launch_gm_divide(g.v(j + 1), g.W, g.G, g.n, g.stream));   // v_{j+1} = z / h_next unless h_next <= 1e-30
        it += 1;
        if ((j + 1) % static_cast<int>(check_every) == 0 || j + 1 == GMRES_M || it == max_it) done = poll();
    }
    TM_KRYLOV_CHK(launch_gm_backsub(g.G, g.stream));                            // GMRES.zig:394-409
    TM_KRYLOV_CHK(launch_gm_update(u, g.V, g.ld, g.G, g.n, g.stream));          // x += V y, GMRES.zig:411-417
    return done;
}

#undef TM_KRYLOV_CHK

}  // namespace tmh
