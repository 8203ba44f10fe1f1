// Host side of the high-order elevation (include/tm_hip.h, "high-order elements"): validation, Gauss-Lobatto nodes and the tables T, D
// in long double, tm_ho_check, and tm_ho_elevate_host -- the definition as a plain loop over the column function the kernel uses
// (tm_highorder.hpp).  No HIP call in this file: it works in a process without a device.
#include "tm_highorder.hpp"
#include "tm_api_util.hpp"
#include "tm_dispatch.hpp"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace tmh {

// ascending roots of (1 - x^2) P'_p(x) by Newton on g(x) = (x^2 - 1) P'_p(x) = p (x P_p - P_{p-1}), g' = p (p+1) P_p
static void gauss_lobatto(int p, long double* x) {
    const long double pi = 3.14159265358979323846264338327950288L;
    x[0] = -1.0L;
    x[p] = 1.0L;
    for (int a = 1; a < p; ++a) {
        long double z = -std::cos(pi * a / p);
        for (int it = 0; it < 100; ++it) {
            long double p0 = 1.0L, p1 = z;   // P_0, P_1 -> P_{p-1}, P_p by the three-term recurrence
            for (int k = 2; k <= p; ++k) {
                const long double pk = ((2 * k - 1) * z * p1 - (k - 1) * p0) / k;
                p0 = p1;
                p1 = pk;
            }
            const long double dz = (z * p1 - p0) / ((p + 1) * p1);
            z -= dz;
            if (std::fabs(dz) <= 1e-20L) break;
        }
        x[a] = z;
    }
}

HoPlan ho_plan(const tm_ho_opt* opt) {
    if (!opt) throw TmError(TM_E_ARG, "null high-order options");
    if (opt->order < 1 || opt->order > TM_HO_MAX_ORDER) throw TmError(TM_E_ARG, "the order must be 1 .. TM_HO_MAX_ORDER");
    HoPlan pl;
    const int p = pl.order = opt->order;
    pl.distribution = opt->distribution;
    long double u[TM_HO_MAX_ORDER + 1];
    switch (opt->distribution) {
    case TM_HO_EQUIDISTANT:
        for (int a = 0; a <= p; ++a) {
            u[a] = a;   // exactly: p * (a/p) is not a for p = 3, 5, 6, 7
            pl.nodes[a] = static_cast<double>(static_cast<long double>(a) / p);
        }
        break;
    case TM_HO_GAUSS_LOBATTO: {
        long double x[TM_HO_MAX_ORDER + 1];
        gauss_lobatto(p, x);
        for (int a = 0; a <= p; ++a) pl.nodes[a] = static_cast<double>((1.0L + x[a]) / 2.0L);   // the one rounding
        break;
    }
    case TM_HO_PRESCRIBED:
        if (!opt->nodes) throw TmError(TM_E_ARG, "TM_HO_PRESCRIBED without nodes");
        for (int a = 0; a <= p; ++a) {
            pl.nodes[a] = opt->nodes[a];
            if (!std::isfinite(pl.nodes[a])) throw TmError(TM_E_ARG, "prescribed nodes must be finite");
            if (a > 0 && !(pl.nodes[a] > pl.nodes[a - 1])) throw TmError(TM_E_ARG, "prescribed nodes must be strictly increasing");
        }
        if (pl.nodes[0] != 0.0 || pl.nodes[p] != 1.0) throw TmError(TM_E_ARG, "prescribed nodes must start at 0 and end at 1");
        break;
    default:
        throw TmError(TM_E_ARG, "unknown node distribution");
    }
    pl.nodes[0] = 0.0;
    pl.nodes[p] = 1.0;
    if (opt->distribution != TM_HO_EQUIDISTANT)
        for (int a = 0; a <= p; ++a) u[a] = static_cast<long double>(p) * static_cast<long double>(pl.nodes[a]);
    pl.identity = opt->distribution == TM_HO_EQUIDISTANT || p == 1;
    const int n1 = p + 1;
    double* T = pl.tab;
    double* D = pl.tab + n1 * n1;
    for (int a = 0; a <= p; ++a)
        for (int m = 0; m <= p; ++m) {
            long double t = 1.0L;
            for (int n = 0; n <= p; ++n)
                if (n != m) t *= (u[a] - n) / static_cast<long double>(m - n);
            long double d = 0.0L;
            for (int k = 0; k <= p; ++k) {
                if (k == m) continue;
                long double pr = 1.0L / static_cast<long double>(m - k);
                for (int n = 0; n <= p; ++n)
                    if (n != m && n != k) pr *= (u[a] - n) / static_cast<long double>(m - n);
                d += pr;
            }
            T[a * n1 + m] = static_cast<double>(t);
            D[a * n1 + m] = static_cast<double>(d);
        }
    return pl;
}

void ho_check_block(const HoPlan& pl, uint64_t block, uint64_t ni, uint64_t nj) {
    const uint64_t p = static_cast<uint64_t>(pl.order);
    if (ni < 2 || nj < 2 || ni * nj >= (uint64_t{1} << 31))
        throw TmError(TM_E_SIZE, "InconsistentSize: block " + std::to_string(block) + " needs at least 2 x 2 nodes (and fewer than 2^31)");
    if ((ni - 1) % p != 0 || (nj - 1) % p != 0)
        throw TmError(TM_E_SIZE, "InconsistentSize: block " + std::to_string(block) + " has " + std::to_string(ni - 1) + " x " + std::to_string(nj - 1) +
                                     " cells, not a multiple of the order " + std::to_string(p));
}

const tm_block& ho_block_of(const tm_mesh_desc* mesh, const HoPlan& pl, uint64_t block) {
    if (!mesh || !mesh->blocks || mesh->nblocks == 0) throw TmError(TM_E_ARG, "mesh description without blocks");
    if (block >= mesh->nblocks) throw TmError(TM_E_ARG, "block index past the mesh");
    const tm_block& b = mesh->blocks[block];
    if (!b.xy) throw TmError(TM_E_ARG, "block without coordinates");
    ho_check_block(pl, block, b.ni, b.nj);
    return b;
}

template <int P>
static void block_host(const HoPlan& pl, const double* xy, uint64_t ni, uint64_t nj, uint64_t block, double* x, double* y, tm_ho_quality* q, double* jj) {
    const QPoint* X = reinterpret_cast<const QPoint*>(xy);
    const int Ei = static_cast<int>((ni - 1) / P), Ej = static_cast<int>((nj - 1) / P);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const bool planes = x && y, want_y = planes && !pl.identity;
    if (planes && pl.identity)
        for (uint64_t j = 0; j < nj; ++j)
            for (uint64_t i = 0; i < ni; ++i) {
                x[j * ni + i] = X[i * nj + j].x;
                y[j * ni + i] = X[i * nj + j].y;
            }
    HoAcc acc;
    ho_init(acc);
    for (int e = 0; e < Ei; ++e)
        for (int f = 0; f < Ej; ++f) {
            const QPoint* base = X + static_cast<size_t>(e) * P * nj + static_cast<size_t>(f) * P;
            auto at = [&](int m, int n) -> const QPoint& { return base[static_cast<size_t>(m) * nj + n]; };
            const double inf = std::numeric_limits<double>::infinity();
            double jmin = inf, jmax = -inf;
            bool bad = false;
            for (int b = 0; b <= P; ++b) {
                double cmin, cmax;
                bool cbad;
                const bool own_b = ho_owns(b, P, f, Ej);
                auto put = [&](int a, double vx, double vy) {
                    if (own_b && ho_owns(a, P, e, Ei)) {
                        const size_t o = (static_cast<size_t>(f) * P + b) * ni + static_cast<size_t>(e) * P + a;
                        x[o] = vx;
                        y[o] = vy;
                    }
                };
                ho_column<P>(at, pl.T() + b * (P + 1), pl.D() + b * (P + 1), pl.T(), pl.D(), want_y, put, cmin, cmax, cbad);
                ho_take_column(jmin, jmax, bad, cmin, cmax, cbad);
            }
            const double area = ho_corner_area(at(0, 0), at(P, 0), at(P, P), at(0, P));
            const unsigned long long el = static_cast<unsigned long long>(e) * Ej + f;
            const int bin = ho_count_element(jmin, jmax, bad, area, el, acc);
            if (bin >= 0) acc.hist[bin / 10][bin % 10] += 1;
            if (jj) {
                jj[2 * (static_cast<size_t>(f) * Ei + e)] = bad ? nan : jmin;
                jj[2 * (static_cast<size_t>(f) * Ei + e) + 1] = bad ? nan : jmax;
            }
        }
    if (q) ho_finish(acc, block, Ei, Ej, P, q);
}

void ho_block_host(const HoPlan& pl, const double* xy, uint64_t ni, uint64_t nj, uint64_t block, double* x, double* y, tm_ho_quality* q, double* jj) {
    dispatch_int<1, 8>(pl.order, [&](auto P) { block_host<P()>(pl, xy, ni, nj, block, x, y, q, jj); });
}

void ho_sj_from_pairs(const double* jj, uint64_t elements, int orientation, double* sj) {
    for (uint64_t k = 0; k < elements; ++k) sj[k] = ho_sj(jj[2 * k], jj[2 * k + 1], jj[2 * k] != jj[2 * k], orientation);
}

void ho_quality_total(const tm_ho_quality* pb, uint64_t n, tm_ho_quality* t) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::memset(t, 0, sizeof(*t));
    t->min_scaled_jacobian = t->min_jacobian = t->max_jacobian = nan;
    bool first = true;
    for (uint64_t b = 0; b < n; ++b) {
        const tm_ho_quality& q = pb[b];
        if (q.elements == 0) continue;   // a block this rank does not own
        t->elements += q.elements;
        t->invalid += q.invalid;
        for (int k = 0; k < 10; ++k) t->hist[k] += q.hist[k];
        if (first) {
            t->orientation = q.orientation;
            t->order = q.order;
        } else {
            if (t->orientation != q.orientation) t->orientation = 0;
            if (t->order != q.order) t->order = 0;
        }
        first = false;
        if (q.min_scaled_jacobian == q.min_scaled_jacobian && !(t->min_scaled_jacobian <= q.min_scaled_jacobian)) {   // strict: ties stay with the lower block
            t->min_scaled_jacobian = q.min_scaled_jacobian;
            t->worst_block = q.worst_block;
            t->worst_e = q.worst_e;
            t->worst_f = q.worst_f;
        }
        if (q.min_jacobian == q.min_jacobian && !(t->min_jacobian <= q.min_jacobian)) t->min_jacobian = q.min_jacobian;
        if (q.max_jacobian == q.max_jacobian && !(t->max_jacobian >= q.max_jacobian)) t->max_jacobian = q.max_jacobian;
    }
}

}  // namespace tmh

using namespace tmh;

extern "C" int tm_ho_tables(const tm_ho_opt* opt, double* nodes, double* T, double* D) {
    return guarded([&]() {
        const HoPlan pl = ho_plan(opt);
        const int n1 = pl.order + 1;
        if (nodes) std::memcpy(nodes, pl.nodes, sizeof(double) * n1);
        if (T) std::memcpy(T, pl.T(), sizeof(double) * n1 * n1);
        if (D) std::memcpy(D, pl.D(), sizeof(double) * n1 * n1);
        return TM_OK;
    });
}

extern "C" int tm_ho_check(const tm_mesh_desc* mesh, const tm_ho_opt* opt) {
    return guarded([&]() {
        const HoPlan pl = ho_plan(opt);
        if (!mesh || !mesh->blocks || mesh->nblocks == 0) throw TmError(TM_E_ARG, "mesh description without blocks");
        if (mesh->nconns && !mesh->conns) throw TmError(TM_E_ARG, "null connection array");
        for (uint64_t b = 0; b < mesh->nblocks; ++b) ho_check_block(pl, b, mesh->blocks[b].ni, mesh->blocks[b].nj);
        const uint64_t p = static_cast<uint64_t>(pl.order);
        for (uint64_t c = 0; c < mesh->nconns; ++c)
            for (int s = 0; s < 2; ++s) {
                const tm_range& r = mesh->conns[c].r[s];
                if (r.start % p != 0 || r.end % p != 0)
                    throw TmError(TM_E_SIZE, "InconsistentSize: connection " + std::to_string(c) + " range " + std::to_string(s) + " (block " + std::to_string(r.block) +
                                                 ", nodes " + std::to_string(r.start) + " .. " + std::to_string(r.end) + ") does not lie on the element grid of order " +
                                                 std::to_string(p));
            }
        return TM_OK;
    });
}

extern "C" int tm_ho_elevate_host(const tm_mesh_desc* mesh, const tm_ho_opt* opt, uint64_t block, double* x, double* y, tm_ho_quality* q, double* sj) {
    return guarded([&]() {
        if ((x == nullptr) != (y == nullptr)) throw TmError(TM_E_ARG, "x and y come together");
        const HoPlan pl = ho_plan(opt);
        const tm_block& b = ho_block_of(mesh, pl, block);
        const uint64_t elements = ((b.ni - 1) / pl.order) * ((b.nj - 1) / pl.order);
        std::vector<double> jj(sj ? 2 * elements : 0);
        tm_ho_quality rec;
        ho_block_host(pl, b.xy, b.ni, b.nj, block, x, y, &rec, sj ? jj.data() : nullptr);
        if (sj) ho_sj_from_pairs(jj.data(), elements, rec.orientation, sj);
        if (q) *q = rec;
        return TM_OK;
    });
}

extern "C" int tm_ho_quality_total(const tm_ho_quality* per_block, uint64_t n, tm_ho_quality* total) {
    return guarded([&]() {
        if (!total || (n && !per_block)) throw TmError(TM_E_ARG, "null argument");
        ho_quality_total(per_block, n, total);
        return TM_OK;
    });
}
