// Host side of K22 (include/tm_hip.h, "elliptic smoothing of stacked blocks"): the checks of a call, the record, and the host definition
// of the control field and of the sweeps.  No HIP call in this file: it works in a process without a device.
#include "tm_smooth3d.hpp"
#include "tm_api_util.hpp"

#include <cstring>
#include <string>
#include <vector>

namespace tmh {

S3Plan s3_plan(uint64_t ni, uint64_t nj, uint64_t nk, const double* x, const double* y, const double* z, const tm_smooth3d_opt* opt) {
    if (!x || !y || !z || !opt) throw TmError(TM_E_ARG, "null argument");
    if (ni < 2 || nj < 2 || nk < 2) throw TmError(TM_E_SIZE, "InconsistentSize: a block has at least 2 nodes in every direction");
    if (ni >= (uint64_t{1} << 31) || nj >= (uint64_t{1} << 31) || nk >= (uint64_t{1} << 31) || ni * nj >= (uint64_t{1} << 40) / nk)
        throw TmError(TM_E_SIZE, "block size out of range");
    if (opt->algorithm != TM_S3_LAPLACE && opt->algorithm != TM_S3_THOMAS_MIDDLECOFF && opt->algorithm != TM_S3_PRESCRIBED)
        throw TmError(TM_E_ARG, "unknown smoothing algorithm");
    if (!(opt->omega > 0.0 && opt->omega <= 1.0)) throw TmError(TM_E_ARG, "omega must lie in (0, 1]");
    if (!(opt->tol >= 0.0)) throw TmError(TM_E_ARG, "tol must be >= 0");
    if (opt->algorithm == TM_S3_PRESCRIBED && (!opt->f1 || !opt->f2 || !opt->f3)) throw TmError(TM_E_ARG, "TM_S3_PRESCRIBED takes the three planes f1, f2, f3");
    S3Plan p;
    p.n[0] = ni;
    p.n[1] = nj;
    p.n[2] = nk;
    p.nodes = p.n[0] * p.n[1] * p.n[2];
    p.interior = (ni - 2) * (nj - 2) * (nk - 2);
    p.algorithm = opt->algorithm;
    p.sweeps = opt->sweeps;
    p.omega = opt->omega;
    p.tol = opt->tol;
    return p;
}

void s3_fill_info(const S3Plan& p, uint64_t done, const S3Acc* first, const S3Acc* last, const double* control_max, tm_smooth3d_info* info) {
    std::memset(info, 0, sizeof *info);
    info->nodes = p.nodes;
    info->interior = p.interior;
    info->sweeps_done = done;
    info->last_max_node = S3_NO_NODE;
    for (int c = 0; c < 3; ++c) info->control_max[c] = control_max[c];
    if (!first || !last) return;
    info->frozen = last->frozen;
    info->first_neg = first->neg;
    info->first_pos = first->pos;
    info->first_zero_or_nan = first->zero_or_nan;
    info->last_neg = last->neg;
    info->last_pos = last->pos;
    info->last_zero_or_nan = last->zero_or_nan;
    info->first_sum_sq = first->sum_sq;
    info->last_sum_sq = last->sum_sq;
    if (last->max_node != S3_NO_NODE) {
        info->last_max_node = last->max_node;
        info->last_max_update = std::sqrt(last->max_sq);
    }
}

void s3_control_host(const S3Plan& p, const double* X, const double* Y, const double* Z, double* const* f) {
    const size_t ni = p.n[0], nj = p.n[1], nk = p.n[2];
    for (int d = 0; d < 3; ++d) {
        std::memset(f[d], 0, sizeof(double) * p.nodes);
        if (!p.interior) continue;
        std::vector<double> F(s3_face_count(d, p.n));
        for (size_t e = 0; e < F.size(); ++e) F[e] = s3_face_value(d, e, p.n, X, Y, Z);
        for (size_t k = 1; k + 1 < nk; ++k)
            for (size_t j = 1; j + 1 < nj; ++j)
                for (size_t i = 1; i + 1 < ni; ++i) {
                    const size_t t = d == 0 ? i : (d == 1 ? j : k), a = d == 0 ? j : i, b = d == 2 ? j : k;
                    f[d][(k * nj + j) * ni + i] = s3_blend(d, p.n, F.data(), t, a, b);
                }
    }
}

static void s3_control_max_host(const S3Plan& p, const double* const* f, double* cmax) {
    const size_t ni = p.n[0], nj = p.n[1], nk = p.n[2];
    for (int d = 0; d < 3; ++d) {
        cmax[d] = 0.0;
        for (size_t k = 1; k + 1 < nk; ++k)
            for (size_t j = 1; j + 1 < nj; ++j)
                for (size_t i = 1; i + 1 < ni; ++i) {
                    const double a = std::fabs(f[d][(k * nj + j) * ni + i]);
                    if (a > cmax[d]) cmax[d] = a;
                }
    }
}

template <bool CONTROL>
static S3Acc s3_sweep_host(const S3Plan& p, const double* const* in, double* const* out, const double* const* f) {
    const size_t ni = p.n[0], nj = p.n[1], nk = p.n[2];
    S3Acc acc;
    s3_init(acc);
    for (int c = 0; c < 3; ++c) std::memcpy(out[c], in[c], sizeof(double) * p.nodes);   // every node that is not interior: bit for bit
    for (size_t k = 1; k + 1 < nk; ++k)
        for (size_t j = 1; j + 1 < nj; ++j)
            for (size_t i = 1; i + 1 < ni; ++i) {
                const size_t o = (k * nj + j) * ni + i;
                S3Stencil s;
                for (int dk = -1; dk <= 1; ++dk)
                    for (int dj = -1; dj <= 1; ++dj)
                        for (int di = -1; di <= 1; ++di) {
                            if (dk != 0 && dj != 0 && di != 0) {
                                s.p[dk + 1][dj + 1][di + 1] = S3Vec{0.0, 0.0, 0.0};
                                continue;
                            }
                            const size_t q = ((k + dk) * nj + (j + dj)) * ni + (i + di);
                            s.p[dk + 1][dj + 1][di + 1] = S3Vec{in[0][q], in[1][q], in[2][q]};
                        }
                const S3Node n = s3_node<CONTROL>(s, CONTROL ? f[0][o] : 0.0, CONTROL ? f[1][o] : 0.0, CONTROL ? f[2][o] : 0.0, p.omega);
                out[0][o] = n.out.x;
                out[1][o] = n.out.y;
                out[2][o] = n.out.z;
                s3_count(acc, n, o);
            }
    return acc;
}

}  // namespace tmh

using namespace tmh;

extern "C" int tm_smooth3d_control_host(uint64_t ni, uint64_t nj, uint64_t nk, const double* x, const double* y, const double* z, double* f1, double* f2,
                                        double* f3) {
    return guarded([&]() {
        if (!f1 || !f2 || !f3) throw TmError(TM_E_ARG, "null argument");
        tm_smooth3d_opt o{};
        o.algorithm = TM_S3_THOMAS_MIDDLECOFF;
        o.omega = 1.0;
        const S3Plan p = s3_plan(ni, nj, nk, x, y, z, &o);
        double* const f[3] = {f1, f2, f3};
        s3_control_host(p, x, y, z, f);
        return TM_OK;
    });
}

extern "C" int tm_smooth3d_planes_host(uint64_t ni, uint64_t nj, uint64_t nk, double* x, double* y, double* z, const tm_smooth3d_opt* opt,
                                       tm_smooth3d_info* info) {
    return guarded([&]() {
        if (!info) throw TmError(TM_E_ARG, "null argument");
        const S3Plan p = s3_plan(ni, nj, nk, x, y, z, opt);
        const bool control = p.algorithm != TM_S3_LAPLACE;
        double cmax[3] = {0.0, 0.0, 0.0};
        std::vector<double> field;
        const double* f[3] = {nullptr, nullptr, nullptr};
        if (p.algorithm == TM_S3_THOMAS_MIDDLECOFF) {
            field.resize(3 * p.nodes);
            double* const fw[3] = {field.data(), field.data() + p.nodes, field.data() + 2 * p.nodes};
            s3_control_host(p, x, y, z, fw);
            for (int c = 0; c < 3; ++c) f[c] = fw[c];
        } else if (p.algorithm == TM_S3_PRESCRIBED) {
            f[0] = opt->f1;
            f[1] = opt->f2;
            f[2] = opt->f3;
        }
        if (control) s3_control_max_host(p, f, cmax);
        if (p.sweeps == 0 || p.interior == 0) {   // nothing moves: the planes stay as they are
            s3_fill_info(p, 0, nullptr, nullptr, cmax, info);
            return TM_OK;
        }
        std::vector<double> other(3 * p.nodes);
        double* a[3] = {x, y, z};
        double* b[3] = {other.data(), other.data() + p.nodes, other.data() + 2 * p.nodes};
        S3Acc first, last;
        uint64_t done = 0;
        while (done < p.sweeps) {
            last = control ? s3_sweep_host<true>(p, a, b, f) : s3_sweep_host<false>(p, a, b, f);
            for (int c = 0; c < 3; ++c) std::swap(a[c], b[c]);
            if (done++ == 0) first = last;
            if (s3_check_after(p, done) && s3_converged(p, last.sum_sq)) break;
        }
        if (a[0] != x)
            for (int c = 0; c < 3; ++c) std::memcpy(b[c], a[c], sizeof(double) * p.nodes);   // an odd count: the result lies in the other copy
        s3_fill_info(p, done, &first, &last, cmax, info);
        return TM_OK;
    });
}
