// Stand-alone caller of the host twin of K22 (csrc/tm_smooth3d_host.cpp) on the edge shapes of tests/test_smooth3d_cpu.py, for a run under
// the host sanitizers.  CPU only: it links no kernel and makes no HIP call.  From turbomesh_amd/csrc:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -o smooth3d_host_check ../../tools/smooth3d_host_check.cpp tm_smooth3d_host.cpp
//   ./smooth3d_host_check
#include "../turbomesh_amd/csrc/tm_api_util.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

struct Block {
    uint64_t ni, nj, nk;
    std::vector<double> x, y, z;
};

static Block bent(uint64_t ni, uint64_t nj, uint64_t nk) {
    Block b{ni, nj, nk, {}, {}, {}};
    for (uint64_t k = 0; k < nk; ++k)
        for (uint64_t j = 0; j < nj; ++j)
            for (uint64_t i = 0; i < ni; ++i) {
                const double a = static_cast<double>(i) / (ni - 1), c = std::pow(static_cast<double>(j) / (nj - 1), 1.5), d = std::pow(static_cast<double>(k) / (nk - 1), 1.3);
                b.x.push_back(1.7 * a + 0.11 * std::sin(2.0 * c + 0.3) * (1 + a) + 0.06 * std::cos(2.0 * d) * c);
                b.y.push_back(0.9 * c + 0.07 * std::sin(3.0 * a) * (1.0 - c) + 0.08 * std::sin(2.5 * d + 0.2) * (1 + a));
                b.z.push_back(1.1 * d + 0.09 * std::sin(2.0 * a + 1.0) * (1.0 - d) + 0.04 * a * c);
            }
    return b;
}

static int failures = 0;
static void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAILED: %s (%s)\n", what, tm_last_error());
        ++failures;
    }
}

static bool faces_held(const Block& a, const Block& b) {
    for (uint64_t k = 0; k < a.nk; ++k)
        for (uint64_t j = 0; j < a.nj; ++j)
            for (uint64_t i = 0; i < a.ni; ++i) {
                if (i && j && k && i + 1 < a.ni && j + 1 < a.nj && k + 1 < a.nk) continue;
                const uint64_t o = (k * a.nj + j) * a.ni + i;
                if (std::memcmp(&a.x[o], &b.x[o], 8) || std::memcmp(&a.y[o], &b.y[o], 8) || std::memcmp(&a.z[o], &b.z[o], 8)) return false;
            }
    return true;
}

static tm_smooth3d_info run(Block& b, int algorithm, uint64_t sweeps, int want = TM_OK, const double* f = nullptr, double omega = 1.0, double tol = 0.0) {
    const Block before = b;
    tm_smooth3d_opt o{algorithm, 0, sweeps, omega, tol, f, f, f};
    tm_smooth3d_info info{};
    const int rc = tm_smooth3d_planes_host(b.ni, b.nj, b.nk, b.x.data(), b.y.data(), b.z.data(), &o, &info);
    expect(rc == want, "return code");
    expect(faces_held(before, b), "faces held");
    return info;
}

int main() {
    const uint64_t shapes[][3] = {{3, 3, 3}, {3, 6, 3}, {6, 3, 3}, {2, 5, 4}, {5, 2, 4}, {5, 4, 2}, {6, 5, 4}, {9, 8, 7}};
    for (const auto& s : shapes)
        for (int algorithm : {TM_S3_LAPLACE, TM_S3_THOMAS_MIDDLECOFF}) {
            Block b = bent(s[0], s[1], s[2]);
            const tm_smooth3d_info info = run(b, algorithm, 3);
            expect(info.interior == (s[0] - 2) * (s[1] - 2) * (s[2] - 2) && info.sweeps_done == (info.interior ? 3u : 0u), "record");
            std::vector<double> f1(b.x.size()), f2(b.x.size()), f3(b.x.size());
            expect(tm_smooth3d_control_host(b.ni, b.nj, b.nk, b.x.data(), b.y.data(), b.z.data(), f1.data(), f2.data(), f3.data()) == TM_OK, "control field");
            Block p = bent(s[0], s[1], s[2]);
            run(p, TM_S3_PRESCRIBED, 2, TM_OK, f1.data());
        }
    Block b = bent(6, 5, 4);
    expect(run(b, TM_S3_THOMAS_MIDDLECOFF, 0).sweeps_done == 0, "sweeps = 0");
    Block two = bent(6, 5, 5);   // two coincident layers
    const uint64_t plane = 6 * 5;
    for (uint64_t q = 0; q < plane; ++q) two.x[2 * plane + q] = two.x[plane + q], two.y[2 * plane + q] = two.y[plane + q], two.z[2 * plane + q] = two.z[plane + q];
    run(two, TM_S3_THOMAS_MIDDLECOFF, 2);
    Block line = bent(7, 6, 5);   // every node on one line: all frozen
    for (uint64_t k = 0, o = 0; k < 5; ++k)
        for (uint64_t j = 0; j < 6; ++j)
            for (uint64_t i = 0; i < 7; ++i, ++o) line.x[o] = static_cast<double>(i + j + k), line.y[o] = line.z[o] = 0.0;
    expect(run(line, TM_S3_LAPLACE, 2).frozen == 60, "a collapsed block is frozen");
    Block nan = bent(7, 7, 7);
    nan.y[(3 * 7 + 3) * 7 + 3] = std::nan("");
    expect(run(nan, TM_S3_LAPLACE, 1).frozen == 18, "a NaN node freezes its 18 neighbours");
    Block e = bent(6, 5, 4);
    run(e, TM_S3_LAPLACE, 1, TM_E_ARG, nullptr, 0.0);
    run(e, TM_S3_LAPLACE, 1, TM_E_ARG, nullptr, 1.5);
    run(e, TM_S3_PRESCRIBED, 1, TM_E_ARG);
    tm_smooth3d_opt o{TM_S3_LAPLACE, 0, 1, 1.0, 0.0, nullptr, nullptr, nullptr};
    tm_smooth3d_info info;
    expect(tm_smooth3d_planes_host(6, 5, 4, nullptr, e.y.data(), e.z.data(), &o, &info) == TM_E_ARG, "NULL plane");
    expect(tm_smooth3d_planes_host(1, 5, 4, e.x.data(), e.y.data(), e.z.data(), &o, &info) == TM_E_SIZE, "ni = 1");
    Block t = bent(9, 8, 7);
    expect(run(t, TM_S3_LAPLACE, 400, TM_OK, nullptr, 1.0, 1e-6).sweeps_done % 8 == 0, "early stop");
    std::printf("smooth3d_host_check: %d failures\n", failures);
    return failures ? 1 : 0;
}

// what the host twin needs from the library besides its own file (tm_api.cpp holds the library's)
extern "C" const char* tm_last_error(void) { return tmh::g_last_error.c_str(); }
