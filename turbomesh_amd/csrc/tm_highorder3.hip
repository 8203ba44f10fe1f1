// K16's driver and entry points (include/tm_hip.h, "high-order hexahedra of stacked blocks"): tables and buffers, the launch of
// k_stack_elevate (tm_highorder3_kernel.hpp, instantiated per order in tm_highorder3_p*.hip), the fixed-order combination of the
// workgroups' records, and the copies back.
#include "tm_highorder3_dev.hpp"
#include "tm_dispatch.hpp"

#include <cstring>

namespace tmh {

__global__ __launch_bounds__(64) void k_ho3_finalize(const HoAcc* __restrict__ partials, int nwg, unsigned long long block, int Ei, int Ej, int Eg, int order,
                                                     tm_ho3_quality* __restrict__ out) {
    __shared__ HoAcc sh[64];
    records_reduce_wave<HoAcc, ho_init, ho_combine>(partials, 0, nwg, sh);
    if (threadIdx.x == 0) ho3_finish(sh[0], block, static_cast<uint64_t>(Ei), static_cast<uint64_t>(Ej), static_cast<uint64_t>(Eg), order, out);
}

static hipError_t ho3_launch_p(int p, int K, const Ho3Launch& a, hipStream_t st) {
    if (p < 1 || p > 4) return hipErrorInvalidValue;
    return dispatch_int<1, 4>(p, [&](auto P) { return ho3_launch<P()>(K, a, st); });
}

// Tables up, K16 and the finalize on `st`, planes / record / pairs back; returns when they have arrived.  The sizes have been checked.
void ho3_run(const StackPlan& p, const HoPlan& pl, StackCuts& cuts, uint64_t block, uint64_t ni, uint64_t nj, uint64_t g_begin, uint64_t g_count, double* x,
             double* y, double* z, tm_ho3_quality* q, double* sj, hipStream_t st, const SurfPlan* sf, uint64_t* outside, double2* pairs_dev) {
    const int K = p.ncuts, P = pl.order;
    const uint64_t Ei = (ni - 1) / P, Ej = (nj - 1) / P, Eg = (p.nlayers - 1) / P;
    const bool planes = x != nullptr, report = q || sj || pairs_dev;
    if (!planes && !report && !(sf && outside)) return;
    stack_fill_radii(p, cuts);
    StackSurfDev sd;
    if (sf) stack_surf_upload(p, *sf, cuts, sd, st);
    DevBuf d_outside;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the counters are copied out as they are");
    if (sf && outside) {
        d_outside.grow(sizeof(unsigned long long) * TM_STACK_MAX_CUTS, "stack outside counts");
        HIPCHK(hipMemsetAsync(d_outside.p, 0, sizeof(unsigned long long) * TM_STACK_MAX_CUTS, st));
    }
    std::vector<double> table = stack_weight_table(p, 0, p.nlayers, 2 * HO_MAX_TABLE);   // the weight rows, then T and D
    const size_t tab_at = static_cast<size_t>(p.nlayers) * (K + 1);
    std::memcpy(&table[tab_at], pl.tab, sizeof(double) * 2 * (P + 1) * (P + 1));
    const size_t plane = static_cast<size_t>(ni) * nj, n = planes ? plane * (g_count * P + 1) : 0, elements = static_cast<size_t>(Ei) * Ej * Eg;
    const dim3 grid((Ej + ho3_tile_ej(P) - 1) / ho3_tile_ej(P), (Ei + ho3_tile_ei(P) - 1) / ho3_tile_ei(P));
    if (grid.y > 65535u) throw TmError(TM_E_SIZE, "InconsistentSize: too many element rows for one launch");
    const size_t nwg = static_cast<size_t>(grid.x) * grid.y;   // the records buffer is sized from the very grid the launcher forms
    DevBuf d_table, d_out(sizeof(double) * 3 * n, "elevated planes"), d_pairs(sj && !pairs_dev ? sizeof(double2) * elements : 0, "element pairs"),
        d_rec(report ? sizeof(HoAcc) * (nwg + RECORDS_REDUCE_GROUPS) : 0, "elevation records"), d_q(sizeof(tm_ho3_quality), "elevation record");
    d_table.upload(table.data(), table.size(), st, "stack weights and elevation tables");
    Ho3Launch a{};
    a.cuts = cuts;
    a.surf = sd.surf;
    a.table = d_table.as<double>();
    a.tab = d_table.as<double>() + tab_at;
    a.mapping = p.mapping;
    a.ni = static_cast<int>(ni);
    a.nj = static_cast<int>(nj);
    a.Ei = static_cast<int>(Ei);
    a.Ej = static_cast<int>(Ej);
    a.g0 = report ? 0 : static_cast<int>(g_begin);   // the record and sj cover the block; without them only the window is evaluated
    a.g1 = report ? static_cast<int>(Eg) : (planes ? static_cast<int>(g_begin + g_count) : a.g0);
    a.gs0 = static_cast<int>(g_begin);
    a.gsn = planes ? static_cast<int>(g_count) : 0;
    a.identity = pl.identity ? 1 : 0;
    a.X = planes ? d_out.as<double>() : nullptr;
    a.Y = planes ? d_out.as<double>() + n : nullptr;
    a.Z = planes ? d_out.as<double>() + 2 * n : nullptr;
    a.pairs = pairs_dev ? pairs_dev : sj ? d_pairs.as<double2>() : nullptr;
    a.partials = report ? d_rec.as<HoAcc>() : nullptr;
    a.outside = d_outside.as<unsigned long long>();
    HIPCHK(ho3_launch_p(P, K, a, st));
    tm_ho3_quality rec{};
    if (report) {
        const Records<HoAcc> rec_in = records_first_stage(a.partials, nwg, st, ho_reduce_launch);
        hipLaunchKernelGGL(k_ho3_finalize, dim3(1), dim3(64), 0, st, rec_in.p, rec_in.n, static_cast<unsigned long long>(block), a.Ei, a.Ej, static_cast<int>(Eg), P,
                           d_q.as<tm_ho3_quality>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&rec, d_q.p, sizeof(rec), hipMemcpyDeviceToHost, st));
    }
    std::vector<double> jj(sj ? 2 * elements : 0);
    if (sj) HIPCHK(hipMemcpyAsync(jj.data(), d_pairs.p, sizeof(double2) * elements, hipMemcpyDeviceToHost, st));
    if (d_outside.p) HIPCHK(hipMemcpyAsync(outside, d_outside.p, sizeof(uint64_t) * K, hipMemcpyDeviceToHost, st));
    if (planes) {
        HIPCHK(hipMemcpyAsync(x, a.X, sizeof(double) * n, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(y, a.Y, sizeof(double) * n, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(z, a.Z, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));   // `table`, `sd` and the device buffers live until here
    if (sj) ho_sj_from_pairs(jj.data(), elements, rec.orientation, sj);
    if (q) *q = rec;
}

// the checks every entry point makes alike once the plan and the block's size are known; returns the validated elevation plan
static HoPlan ho3_checked(const StackPlan& p, const tm_ho_opt* opt, uint64_t block, uint64_t ni, uint64_t nj, uint64_t g_begin, uint64_t g_count, bool planes) {
    const HoPlan pl = ho3_plan(opt);
    ho3_check_block(pl, block, ni, nj);
    ho3_check_layers(pl, p.nlayers);
    ho3_check_window((p.nlayers - 1) / pl.order, g_begin, g_count, planes);
    return pl;
}

}  // namespace tmh

using namespace tmh;

extern "C" int tm_stack_elevate(const tm_mesh_desc* const* cuts, const tm_stack_opt* sopt, const tm_stack_surfaces* surfaces, const tm_ho_opt* opt, uint64_t block,
                                uint64_t g_begin, uint64_t g_count, double* x, double* y, double* z, tm_ho3_quality* q, double* sj, uint64_t* outside) {
    return guarded([&]() {
        if ((x == nullptr) != (y == nullptr) || (x == nullptr) != (z == nullptr)) throw TmError(TM_E_ARG, "x, y and z come together");
        SurfPlan sf;
        const SurfPlan* sfp = nullptr;
        const StackPlan p = stack_plan_any(sopt, surfaces, sf, &sfp);
        uint64_t ni = 0, nj = 0;
        stack_check_cuts(cuts, p.ncuts, block, &ni, &nj);
        const HoPlan pl = ho3_checked(p, opt, block, ni, nj, g_begin, g_count, x != nullptr);
        DevBuf in;
        StackCuts dc{};
        stack_upload_cuts(cuts, p.ncuts, block, ni, nj, in, dc);
        ho3_run(p, pl, dc, block, ni, nj, g_begin, g_count, x, y, z, q, sj, nullptr, sfp, outside);
        return TM_OK;
    });
}

extern "C" int tm_stack_smoothers_elevate(tm_smoother* const* cuts, const tm_stack_opt* sopt, const tm_stack_surfaces* surfaces, const tm_ho_opt* opt, uint64_t block,
                                          uint64_t g_begin, uint64_t g_count, double* x, double* y, double* z, tm_ho3_quality* q, double* sj, uint64_t* outside) {
    return guarded([&]() {
        if (!cuts) throw TmError(TM_E_ARG, "null argument");
        if ((x == nullptr) != (y == nullptr) || (x == nullptr) != (z == nullptr)) throw TmError(TM_E_ARG, "x, y and z come together");
        SurfPlan sf;
        const SurfPlan* sfp = nullptr;
        const StackPlan p = stack_plan_any(sopt, surfaces, sf, &sfp);
        StackCuts dc{};
        uint64_t ni = 0, nj = 0;
        stack_resident_cuts(cuts, p, block, dc, &ni, &nj);
        const HoPlan pl = ho3_checked(p, opt, block, ni, nj, g_begin, g_count, x != nullptr);
        std::vector<std::unique_ptr<StackEvent>> events;
        const hipStream_t st = stack_order_behind(cuts, p.ncuts, events);
        ho3_run(p, pl, dc, block, ni, nj, g_begin, g_count, x, y, z, q, sj, st, sfp, outside);   // synchronises st
        return TM_OK;
    });
}
