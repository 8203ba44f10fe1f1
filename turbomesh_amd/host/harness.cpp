// harness.cpp -- plays the role of the Zig caller (reference src/gui/main.zig:30-56, src/wasm/lib.zig:35-55):
// build edges -> Block2d.init (TFI on the MI355X) -> Mesh with connections -> smooth.mesh -> log like the reference.
//
//   tm_harness strip <nblocks> <ni> <nj> <iterations> [relax|bicgstab|mg] [until <tol>] [write <file.xyz>] [dump.bin]
//   tm_harness single <ni> <nj> <iterations> [relax|bicgstab|mg] [until <tol>] [write <file.xyz>] [dump.bin]
//   tm_harness tm <ni> <nj> <iterations>               the Thomas-Middlecoff control field on a clustered rectangle (exit 0: it kept the clustering)
//   tm_harness stack <ni> <nj> <ncuts> <nlayers>       config-5 cuts (amplitude 0.05 + 0.001 c), five relaxation sweeps per handle, stacked on the
//                                                      device by the natural cubic spline: a checksum per layer (exit 0: layers at cuts equal the cuts)
//   tm_harness certify <ni> <nj> <order>   Bezier certificate of those elements (kernel K14; exit 0: equal to the CPU's, counts add up)
//   tm_harness elevate <ni> <nj> <order>   curved elements of that order from a smoothed block (kernel K13; exit 0: corners unchanged, equal to the CPU's)
//   tm_harness stack-certify <ni> <nj> <ncuts> <nlayers> <order>   the same cuts: the certificate of those hexahedra (kernel K17; exit 0: counts add up, equal to the CPU's)
//   tm_harness stack-elevate <ni> <nj> <ncuts> <nlayers> <order>   the same cuts: curved hexahedra of that order from the stacked block (kernel K16; exit 0: corners unchanged, equal to the CPU's)
//   tm_harness stack-quality <ni> <nj> <ncuts> <nlayers>   the same cuts: the 3-D quality record of the stacked block (kernel K12; exit 0: equal to the CPU's)
//   tm_harness weld <ni> <nj> <nblocks>   the strip welded into one unstructured mesh from the resident coordinates (kernel K18; exit 0: equal to the CPU's)
//   tm_harness fv <ni> <nj> <nblocks> [nlayers]              its faces, owners and finite-volume metrics (kernel K21; exit 0: equal to the CPU's)
//   tm_harness weld-boundary <ni> <nj> <nblocks> [nlayers]   its boundary faces in patches and their measures (kernel K19; exit 0: equal to the CPU's)
//   tm_harness wall-distance <ni> <nj> <nblocks> [nlayers]   the wall distance of its nodes and the record (kernel K20; exit 0: equal to the host twin's)
//   tm_harness csr                                     the linear-solver slot (seam 2) on the reference's 5 x 5 known answer
//   tm_harness ranks <world> <rank> <idfile> <nblocks> <ni> <nj> <iterations> [relax|bicgstab] [dump.bin]
//        one process per GPU (start each with HIP_VISIBLE_DEVICES=<its GPU>): the strip's blocks are dealt to the ranks in order, the
//        interface rows travel by the library's own RCCL transport (tm_rccl_*); rank 0 writes the ncclUniqueId to <idfile>, the
//        others wait for it (the rendezvous a Zig caller would do over MPI or a file); dump.bin = this rank's OWNED blocks
//
// The synthetic edges are those of SURVEY.md 8d (config 2 / config 4), identical to turbomesh_amd/configs.py.
// dump.bin (optional): all block coordinates as raw f64 after smoothing, for the parity test.
#include "turbomesh.hpp"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>

using namespace core;
using discrete::Block2d;
using discrete::Edge;
using types::Vec2d;

static Edge uniformEdge(std::vector<Vec2d> pts) {
    Edge e;
    e.clustering = clustering::create(clustering::Uniform{}, pts.size());
    e.points = std::move(pts);
    return e;
}
static void snap(Block2d& b, const Edge& i_min, const Edge& i_max, const Edge& j_min, const Edge& j_max) {
    const std::size_t ni = b.points.size[0], nj = b.points.size[1];
    for (std::size_t i = 0; i < ni; ++i) {
        b.points.data[b.points.index(i, 0)] = i_min.points[i];
        b.points.data[b.points.index(i, nj - 1)] = i_max.points[i];
    }
    for (std::size_t j = 0; j < nj; ++j) {
        b.points.data[b.points.index(0, j)] = j_min.points[j];
        b.points.data[b.points.index(ni - 1, j)] = j_max.points[j];
    }
}

static discrete::Mesh buildStrip(std::size_t nblocks, std::size_t ni, std::size_t nj) {
    const double A = 0.1, two_pi = 2 * M_PI;
    const auto t = clustering::create(clustering::Uniform{}, nj);
    const auto s = clustering::create(clustering::Uniform{}, ni);
    auto curve = [&](std::size_t k) {
        std::vector<Vec2d> c(nj);
        for (std::size_t j = 0; j < nj; ++j) c[j] = Vec2d{{t[j], static_cast<double>(k) + A * (1.0 - 2.0 * static_cast<double>(k) / static_cast<double>(nblocks)) * std::sin(two_pi * t[j])}};
        c[0] = Vec2d{{0.0, static_cast<double>(k)}};
        c[nj - 1] = Vec2d{{1.0, static_cast<double>(k)}};
        return c;
    };
    discrete::Mesh mesh;
    for (std::size_t k = 0; k < nblocks; ++k) {
        const auto c0 = curve(k), c1 = curve(k + 1);
        std::vector<Vec2d> left(ni), right(ni);
        for (std::size_t i = 0; i < ni; ++i) {
            left[i] = Vec2d{{0.0, static_cast<double>(k) + s[i]}};
            right[i] = Vec2d{{1.0, static_cast<double>(k) + s[i]}};
        }
        left[0] = c0[0]; left[ni - 1] = c1[0];
        right[0] = c0[nj - 1]; right[ni - 1] = c1[nj - 1];
        const Edge i_min = uniformEdge(left), i_max = uniformEdge(right), j_min = uniformEdge(c0), j_max = uniformEdge(c1);
        Block2d b = Block2d::init(i_min, i_max, j_min, j_max);
        snap(b, i_min, i_max, j_min, j_max);
        mesh.addBlock("block_" + std::to_string(k), std::move(b));
    }
    for (std::size_t k = 0; k + 1 < nblocks; ++k)
        mesh.connections.push_back(boundary::Connection{{boundary::Range{k, boundary::Side::j_max, 0, nj - 1}, boundary::Range{k + 1, boundary::Side::j_min, 0, nj - 1}}, std::nullopt});
    return mesh;
}

static discrete::Mesh buildSingle(std::size_t ni, std::size_t nj, double A = 0.1) {
    const double two_pi = 2 * M_PI;
    const auto s = clustering::create(clustering::Uniform{}, ni);
    const auto t = clustering::create(clustering::Uniform{}, nj);
    std::vector<Vec2d> lo(ni), up(ni), le(nj), ri(nj);
    for (std::size_t i = 0; i < ni; ++i) {
        lo[i] = Vec2d{{s[i], A * std::sin(two_pi * s[i])}};
        up[i] = Vec2d{{s[i], 1.0 - A * std::sin(two_pi * s[i])}};
    }
    for (std::size_t j = 0; j < nj; ++j) {
        le[j] = Vec2d{{0.0, t[j]}};
        ri[j] = Vec2d{{1.0, t[j]}};
    }
    lo[0] = Vec2d{{0, 0}}; lo[ni - 1] = Vec2d{{1, 0}};
    up[0] = Vec2d{{0, 1}}; up[ni - 1] = Vec2d{{1, 1}};
    const Edge i_min = uniformEdge(lo), i_max = uniformEdge(up), j_min = uniformEdge(le), j_max = uniformEdge(ri);
    discrete::Mesh mesh;
    Block2d b = Block2d::init(i_min, i_max, j_min, j_max);
    snap(b, i_min, i_max, j_min, j_max);
    mesh.addBlock("block", std::move(b));
    return mesh;
}

// Seam 2 from a compiled caller: a system assembled on the host -- here the reference's own known answer, umfpack.zig:71-97
// (A x = b, x = 1..5, given there in CSC; CSR below) as the x-system and 2 b as the y-system -- solved through tm_csr_solve.
static int csrKat() {
    const int32_t Ap[] = {0, 2, 5, 8, 9, 12};     // rows: [2 3 . . .] [3 . 4 . 6] [. -1 -3 2 .] [. . 1 . .] [. 4 2 . 1]
    const int32_t Ai[] = {0, 1, 0, 2, 4, 1, 2, 3, 2, 1, 2, 4};
    const double Ax[] = {2, 3, 3, 4, 6, -1, -3, 2, 1, 4, 2, 1};
    const double bx[] = {8, 45, -3, 3, 19};
    double by[5], x[5] = {0, 0, 0, 0, 0}, y[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < 5; ++i) by[i] = 2 * bx[i];
    tm_solver_opt opt{};
    opt.tag = TM_SOLVER_HIP;
    opt.rtol = 1e-14;
    opt.max_inner = 200;
    opt.check_every = 1;
    tm_stats st{};
    const int rc = tm_csr_solve(5, Ap, Ai, Ax, nullptr, bx, by, x, y, &opt, &st);
    if (rc < 0) throw core::Error(rc, tm_last_error());
    double err = 0;
    for (int i = 0; i < 5; ++i) err = std::fmax(err, std::fmax(std::fabs(x[i] - (i + 1)), std::fabs(y[i] - 2 * (i + 1))));
    std::printf("csr kat: rc %d, inner iterations %llu, max error %.3e\n", rc, static_cast<unsigned long long>(st.inner_iterations), err);
    return (rc == 0 && err < 1e-9) ? 0 : 1;
}

// One rank of a multi-process run through the library's RCCL transport, from a compiled caller (what distributed.RcclHooks does
// from Python): unique id by file, communicator, hooks for this partition, handle, iterate, download the owned blocks.
static int runRank(int argc, char** argv) {
    if (argc < 9) throw Error(TM_E_ARG, "ranks <world> <rank> <idfile> <nblocks> <ni> <nj> <iterations> [relax|bicgstab] [dump.bin]");
    const int world = std::atoi(argv[2]), rank = std::atoi(argv[3]);
    const std::string idfile = argv[4];
    const std::size_t nb = std::strtoull(argv[5], nullptr, 10), ni = std::strtoull(argv[6], nullptr, 10), nj = std::strtoull(argv[7], nullptr, 10);
    const std::size_t iterations = std::strtoull(argv[8], nullptr, 10);
    if (world < 1 || rank < 0 || rank >= world || nb < static_cast<std::size_t>(world)) throw Error(TM_E_ARG, "ranks: need 0 <= rank < world <= nblocks");
    int a = 9;
    smoothing::solver::Option opt;
    if (a < argc && std::strcmp(argv[a], "relax") == 0) opt.inner = TM_INNER_RELAX;
    if (a < argc && (std::strcmp(argv[a], "relax") == 0 || std::strcmp(argv[a], "bicgstab") == 0)) ++a;
    opt.rtol = 1e-13;
    opt.max_inner = 5000;
    const char* librccl = std::getenv("TM_LIBRCCL");   // the copy the process should use; unset = default search
    unsigned char id[TM_RCCL_ID_BYTES];
    if (rank == 0) {
        check(tm_rccl_unique_id(librccl, id));
        const std::string tmp = idfile + ".tmp";
        std::FILE* f = std::fopen(tmp.c_str(), "wb");
        if (!f || std::fwrite(id, 1, sizeof(id), f) != sizeof(id)) throw Error(TM_E_ARG, "cannot write " + tmp);
        std::fclose(f);
        if (std::rename(tmp.c_str(), idfile.c_str()) != 0) throw Error(TM_E_ARG, "cannot publish " + idfile);
    } else {
        bool got = false;
        for (int tries = 0; tries < 6000 && !got; ++tries) {   // up to a minute
            if (std::FILE* f = std::fopen(idfile.c_str(), "rb")) {
                got = std::fread(id, 1, sizeof(id), f) == sizeof(id);
                std::fclose(f);
            }
            if (!got) std::this_thread::sleep_for(std::chrono::milliseconds(10));
        }
        if (!got) throw Error(TM_E_ARG, "no unique id appeared in " + idfile);
    }
    tm_rccl_comm* comm = nullptr;
    check(tm_rccl_comm_create(librccl, id, rank, world, &comm));
    discrete::Mesh mesh = buildStrip(nb, ni, nj);
    std::vector<int32_t> owner(nb);
    for (std::size_t b = 0; b < nb; ++b) owner[b] = static_cast<int32_t>(b * static_cast<std::size_t>(world) / nb);
    tm_stats st{};
    {
        smoothing::smooth::Desc d(mesh);   // the partition's exchange plan is derived from the same description the handle gets
        tm_comm_hooks hooks{};
        check(tm_rccl_hooks(comm, &d.desc, owner.data(), &hooks));
        smoothing::smooth::Smoother sm(mesh, opt, smoothing::wall_control_function::Algorithm::laplace(), &hooks);
        st = sm.iterate(iterations);
        sm.download();
    }
    tm_rccl_comm_destroy(comm);
    std::printf("rank %d of %d: outer %llu inner %llu not_converged %d last_residual %.17g\n", rank, world, static_cast<unsigned long long>(st.outer_iterations),
                static_cast<unsigned long long>(st.inner_iterations), st.not_converged, st.last_residual);
    if (a < argc) {
        std::FILE* f = std::fopen(argv[a], "wb");
        if (!f) throw Error(TM_E_ARG, "cannot open dump file");
        for (std::size_t b = 0; b < nb; ++b)
            if (owner[b] == rank) std::fwrite(mesh.blocks[b].points.data.data(), sizeof(Vec2d), mesh.blocks[b].points.data.size(), f);
        std::fclose(f);
    }
    return 0;
}

// tm_harness tm <ni> <nj> <iterations>: a rectangle whose i lines are tanh-clustered towards both ends and whose j lines towards the lower
// wall, x = x(i), y = y(j): under the Thomas-Middlecoff field this seed is a fixed point of the discrete equations (P = -x_ii / x_i exactly
// cancels the second difference), under Laplace it relaxes towards the uniform mesh.  Prints how far the nodes moved under either.
static int thomasMiddlecoff(std::size_t ni, std::size_t nj, std::size_t iterations) {
    std::vector<double> x(ni), y(nj);
    for (std::size_t i = 0; i < ni; ++i) x[i] = 0.5 * (1.0 + std::tanh(2.0 * (2.0 * static_cast<double>(i) / static_cast<double>(ni - 1) - 1.0)) / std::tanh(2.0));
    for (std::size_t j = 0; j < nj; ++j) y[j] = 1.0 + std::tanh(2.5 * (static_cast<double>(j) / static_cast<double>(nj - 1) - 1.0)) / std::tanh(2.5);
    auto build = [&]() {
        std::vector<Vec2d> lo(ni), up(ni), le(nj), ri(nj);
        for (std::size_t i = 0; i < ni; ++i) lo[i] = Vec2d{{x[i], y[0]}}, up[i] = Vec2d{{x[i], y[nj - 1]}};
        for (std::size_t j = 0; j < nj; ++j) le[j] = Vec2d{{x[0], y[j]}}, ri[j] = Vec2d{{x[ni - 1], y[j]}};
        Block2d b = Block2d::init(uniformEdge(lo), uniformEdge(up), uniformEdge(le), uniformEdge(ri));
        for (std::size_t i = 0; i < ni; ++i)
            for (std::size_t j = 0; j < nj; ++j) b.points.data[b.points.index(i, j)] = Vec2d{{x[i], y[j]}};
        discrete::Mesh mesh;
        mesh.addBlock("block_0", std::move(b));
        return mesh;
    };
    auto moved = [&](const discrete::Mesh& m) {
        double s = 0.0;
        for (std::size_t i = 0; i < ni; ++i)
            for (std::size_t j = 0; j < nj; ++j) {
                const Vec2d p = m.blocks[0].points.getIndex(i, j);
                s += (p.data[0] - x[i]) * (p.data[0] - x[i]) + (p.data[1] - y[j]) * (p.data[1] - y[j]);
            }
        return std::sqrt(s / static_cast<double>(2 * ni * nj));
    };
    smoothing::solver::Option opt;
    double rms[2], pmax = 0.0, qmax = 0.0;
    for (int k = 0; k < 2; ++k) {
        discrete::Mesh mesh = build();
        smoothing::smooth::Smoother sm(mesh, opt, k == 0 ? smoothing::wall_control_function::Algorithm::thomas_middlecoff() : smoothing::wall_control_function::Algorithm::laplace());
        if (k == 0)
            for (const Vec2d& pq : sm.controlFunction()) pmax = std::max(pmax, std::fabs(pq.data[0])), qmax = std::max(qmax, std::fabs(pq.data[1]));
        sm.iterate(iterations);
        sm.download();
        rms[k] = moved(mesh);
    }
    std::printf("thomas_middlecoff max|P| %.6f max|Q| %.6f rms_moved %.3e laplace rms_moved %.3e\n", pmax, qmax, rms[0], rms[1]);
    return rms[0] <= 1e-12 && rms[1] > 1e-2 ? 0 : 1;
}

// tm_harness stack <ni> <nj> <ncuts> <nlayers>: the spanwise cuts of SURVEY 8d config 5 (the config-2 block with amplitude
// 0.05 + 0.001 c), one handle per cut, five relaxation sweeps each; the cuts sit at span 0, 1, .. K-1, the layers are uniform over it.
// The 3-D block comes from the coordinates resident in the handles (stack::stack_block -> tm_stack_smoothers).
static int stackCuts(std::size_t ni, std::size_t nj, std::size_t ncuts, std::size_t nlayers) {
    if (ncuts < 2 || nlayers < 1) throw Error(TM_E_ARG, "stack <ni> <nj> <ncuts> <nlayers>: at least two cuts and one layer");
    smoothing::solver::Option opt;
    opt.inner = TM_INNER_RELAX;
    std::vector<discrete::Mesh> meshes;
    meshes.reserve(ncuts);
    for (std::size_t c = 0; c < ncuts; ++c) meshes.push_back(buildSingle(ni, nj, 0.05 + 0.001 * static_cast<double>(c)));
    std::vector<std::unique_ptr<smoothing::smooth::Smoother>> handles;
    std::vector<smoothing::smooth::Smoother*> cuts;
    for (std::size_t c = 0; c < ncuts; ++c) {
        handles.push_back(std::make_unique<smoothing::smooth::Smoother>(meshes[c], opt, smoothing::wall_control_function::Algorithm::laplace()));
        handles.back()->iterate(5);
        cuts.push_back(handles.back().get());
    }
    stack::Option so;
    for (std::size_t c = 0; c < ncuts; ++c) so.span.push_back(static_cast<double>(c));
    const double z1 = so.span.back();
    for (std::size_t k = 0; k < nlayers; ++k) so.layers.push_back(nlayers == 1 ? 0.0 : (k + 1 == nlayers ? z1 : z1 * (static_cast<double>(k) / static_cast<double>(nlayers - 1))));
    const stack::Block3d b = stack::stack_block(cuts, so, 0, 0, nlayers);
    for (auto& h : handles) h->download();
    const std::size_t n = ni * nj;
    std::size_t compared = 0;
    bool equal = true;
    for (std::size_t k = 0; k < nlayers; ++k) {
        double sx = 0, sy = 0;
        for (std::size_t q = 0; q < n; ++q) sx += b.x[k * n + q], sy += b.y[k * n + q];
        std::printf("stack: layer %zu s %.17g sum_x %.17g sum_y %.17g z %.17g\n", k, so.layers[k], sx, sy, b.z[k * n]);
        for (std::size_t c = 0; c < ncuts; ++c) {
            if (so.layers[k] != so.span[c]) continue;
            ++compared;
            for (std::size_t i = 0; i < ni; ++i)
                for (std::size_t j = 0; j < nj; ++j) {
                    const Vec2d p = meshes[c].blocks[0].points.getIndex(i, j);
                    const std::size_t o = (k * nj + j) * ni + i;
                    if (!(b.x[o] == p.data[0] && b.y[o] == p.data[1] && b.z[o] == so.span[c])) equal = false;
                }
        }
    }
    const bool ok = equal && compared >= (nlayers >= 2 ? 2u : 1u);
    std::printf("stack: layers at cuts equal the cuts: %s\n", ok ? "yes" : "no");
    return ok ? 0 : 1;
}

// tm_harness stack-revolution <ni> <nj> <ncuts> <nlayers>: the cuts of `stack`, read as cuts in the unrolled plane of coaxial cones
// r = (1 + c/4) + (x + 1/2)/2, x = u (nine knots over [-1/2, 3/2], all dyadic, so the knots lie on their cone exactly; natural splines
// through them): the layers from the coordinates resident in the handles (stack::stack_block -> tm_stack_smoothers_surf).  A layer at a
// cut must lie on the cut's cone, and the device's 3-D quality record must equal the CPU's report of those planes.
static int stackRevolution(std::size_t ni, std::size_t nj, std::size_t ncuts, std::size_t nlayers) {
    if (ncuts < 2 || nlayers < 2) throw Error(TM_E_ARG, "stack-revolution <ni> <nj> <ncuts> <nlayers>: at least two cuts and two layers");
    smoothing::solver::Option opt;
    opt.inner = TM_INNER_RELAX;
    std::vector<discrete::Mesh> meshes;
    meshes.reserve(ncuts);
    for (std::size_t c = 0; c < ncuts; ++c) meshes.push_back(buildSingle(ni, nj, 0.05 + 0.001 * static_cast<double>(c)));
    std::vector<std::unique_ptr<smoothing::smooth::Smoother>> handles;
    std::vector<smoothing::smooth::Smoother*> cuts;
    for (std::size_t c = 0; c < ncuts; ++c) {
        handles.push_back(std::make_unique<smoothing::smooth::Smoother>(meshes[c], opt, smoothing::wall_control_function::Algorithm::laplace()));
        handles.back()->iterate(5);
        cuts.push_back(handles.back().get());
    }
    stack::Option so;
    so.mapping = TM_STACK_REVOLUTION;
    stack::Surfaces sf;
    for (std::size_t c = 0; c < ncuts; ++c) {
        so.span.push_back(static_cast<double>(c));
        const double r0 = 1.0 + 0.25 * static_cast<double>(c);
        sf.rref.push_back(r0);
        std::vector<double> u, r;
        for (int n = 0; n < 9; ++n) u.push_back(-0.5 + 0.25 * n), r.push_back(r0 + 0.5 * (u.back() + 0.5));
        sf.u.push_back(u), sf.x.push_back(u), sf.r.push_back(r);
    }
    const double z1 = so.span.back();
    for (std::size_t k = 0; k < nlayers; ++k) so.layers.push_back(k + 1 == nlayers ? z1 : z1 * (static_cast<double>(k) / static_cast<double>(nlayers - 1)));
    std::vector<uint64_t> outside;
    const stack::Block3d b = stack::stack_block(cuts, so, sf, 0, 0, nlayers, &outside);
    const tm_quality3d q = stack::quality(cuts, so, sf, 0), qh = stack::quality(b);
    const std::size_t n = ni * nj;
    std::size_t compared = 0;
    bool on = true;
    for (std::size_t k = 0; k < nlayers; ++k) {
        double sx = 0, sr = 0;
        for (std::size_t p = 0; p < n; ++p) sx += b.x[k * n + p], sr += std::hypot(b.y[k * n + p], b.z[k * n + p]);
        std::printf("stack-revolution: layer %zu s %.17g sum_x %.17g sum_r %.17g\n", k, so.layers[k], sx, sr);
        for (std::size_t c = 0; c < ncuts; ++c) {
            if (so.layers[k] != so.span[c]) continue;
            ++compared;
            for (std::size_t p = 0; p < n; ++p) {
                const double x = b.x[k * n + p], r = std::hypot(b.y[k * n + p], b.z[k * n + p]), want = sf.rref[c] + 0.5 * (x + 0.5);
                if (!(std::fabs(r - want) <= 64 * 2.220446049250313e-16 * (std::fabs(want) + std::fabs(x) + 1.0))) on = false;
            }
        }
    }
    for (std::size_t c = 0; c < ncuts; ++c) std::printf("stack-revolution: cut %zu extrapolated nodes %llu\n", c, static_cast<unsigned long long>(outside[c]));
    tm_quality3d a = q, h = qh;
    a.total_volume = h.total_volume = 0.0;   // a sum, added in another order on the device
    const bool same = std::memcmp(&a, &h, sizeof(a)) == 0;
    std::printf("stack-revolution: quality cells %llu inverted %llu degenerate %llu min_scaled_jacobian %.17g device equals host: %s\n",
                static_cast<unsigned long long>(q.cells), static_cast<unsigned long long>(q.inverted), static_cast<unsigned long long>(q.degenerate),
                q.min_scaled_jacobian, same ? "yes" : "no");
    const bool ok = on && same && compared >= 2;
    std::printf("stack-revolution: layers at cuts lie on their surfaces: %s\n", on && compared >= 2 ? "yes" : "no");
    return ok ? 0 : 1;
}

// tm_harness stack-quality <ni> <nj> <ncuts> <nlayers>: the cuts of `stack`; the 3-D quality record of the stacked block from the
// coordinates resident in the handles (stack::quality -> tm_stack_smoothers_quality), compared with the CPU's report of the planes
// tm_stack_smoothers returns for the same handles (every field but the summed total_volume bit for bit).
static int stackQuality(std::size_t ni, std::size_t nj, std::size_t ncuts, std::size_t nlayers) {
    if (ncuts < 2 || nlayers < 2) throw Error(TM_E_ARG, "stack-quality <ni> <nj> <ncuts> <nlayers>: at least two cuts and two layers");
    smoothing::solver::Option opt;
    opt.inner = TM_INNER_RELAX;
    std::vector<discrete::Mesh> meshes;
    meshes.reserve(ncuts);
    for (std::size_t c = 0; c < ncuts; ++c) meshes.push_back(buildSingle(ni, nj, 0.05 + 0.001 * static_cast<double>(c)));
    std::vector<std::unique_ptr<smoothing::smooth::Smoother>> handles;
    std::vector<smoothing::smooth::Smoother*> cuts;
    for (std::size_t c = 0; c < ncuts; ++c) {
        handles.push_back(std::make_unique<smoothing::smooth::Smoother>(meshes[c], opt, smoothing::wall_control_function::Algorithm::laplace()));
        handles.back()->iterate(5);
        cuts.push_back(handles.back().get());
    }
    stack::Option so;
    for (std::size_t c = 0; c < ncuts; ++c) so.span.push_back(static_cast<double>(c));
    const double z1 = so.span.back();
    for (std::size_t k = 0; k < nlayers; ++k) so.layers.push_back(k + 1 == nlayers ? z1 : z1 * (static_cast<double>(k) / static_cast<double>(nlayers - 1)));
    const tm_quality3d q = stack::quality(cuts, so, 0);
    const tm_quality3d h = stack::quality(stack::stack_block(cuts, so, 0, 0, nlayers));
    std::printf("stack-quality: hexahedra %llu inverted %llu degenerate %llu orientation %d\n", static_cast<unsigned long long>(q.cells),
                static_cast<unsigned long long>(q.inverted), static_cast<unsigned long long>(q.degenerate), q.orientation);
    std::printf("stack-quality: min scaled jacobian %.17g at (i %llu, j %llu, k %llu) max aspect %.17g max growth k %.17g\n", q.min_scaled_jacobian,
                static_cast<unsigned long long>(q.worst_i), static_cast<unsigned long long>(q.worst_j), static_cast<unsigned long long>(q.worst_k), q.max_aspect, q.max_growth_k);
    std::printf("stack-quality: volume min %.17g max %.17g total %.17g\n", q.min_volume, q.max_volume, q.total_volume);
    std::printf("stack-quality: hist");
    for (int k = 0; k < 10; ++k) std::printf(" %llu", static_cast<unsigned long long>(q.hist[k]));
    std::printf("\n");
    tm_quality3d a = q, b = h;
    a.total_volume = b.total_volume = 0.0;
    const bool same = std::memcmp(&a, &b, sizeof(a)) == 0 && std::fabs(q.total_volume - h.total_volume) <= static_cast<double>(q.cells) * 0x1p-53 * std::fabs(h.total_volume);
    std::printf("stack-quality: device equals host: %s\n", same ? "yes" : "no");
    return same ? 0 : 1;
}

// tm_harness stack-smooth <ni> <nj> <nk> <sweeps>: three cuts of `stack` on nk layers; the block stacked from the coordinates resident in
// the handles and smoothed on the device with the Thomas-Middlecoff field (stack::smooth -> tm_stack_smoothers_smooth), compared with the
// CPU's sweeps of the planes tm_stack_smoothers returns for the same handles: planes and record bit for bit, the two sums within their bound.
static int stackSmooth(std::size_t ni, std::size_t nj, std::size_t nlayers, std::size_t sweeps) {
    if (nlayers < 2) throw Error(TM_E_ARG, "stack-smooth <ni> <nj> <nk> <sweeps>: at least two layers");
    const std::size_t ncuts = 3;
    smoothing::solver::Option opt;
    opt.inner = TM_INNER_RELAX;
    std::vector<discrete::Mesh> meshes;
    meshes.reserve(ncuts);
    for (std::size_t c = 0; c < ncuts; ++c) meshes.push_back(buildSingle(ni, nj, 0.05 + 0.02 * static_cast<double>(c)));
    std::vector<std::unique_ptr<smoothing::smooth::Smoother>> handles;
    std::vector<smoothing::smooth::Smoother*> cuts;
    for (std::size_t c = 0; c < ncuts; ++c) {
        handles.push_back(std::make_unique<smoothing::smooth::Smoother>(meshes[c], opt, smoothing::wall_control_function::Algorithm::laplace()));
        handles.back()->iterate(5);
        cuts.push_back(handles.back().get());
    }
    stack::Option so;
    for (std::size_t c = 0; c < ncuts; ++c) so.span.push_back(static_cast<double>(c));
    const double z1 = so.span.back();
    for (std::size_t k = 0; k < nlayers; ++k) so.layers.push_back(k + 1 == nlayers ? z1 : z1 * (static_cast<double>(k) / static_cast<double>(nlayers - 1)));
    stack::Smooth sm;
    sm.sweeps = sweeps;
    tm_smooth3d_info d;
    const stack::Block3d dev = stack::smooth(cuts, so, 0, sm, &d);
    stack::Block3d host = stack::stack_block(cuts, so, 0, 0, nlayers);
    const stack::Block3d before = host;
    const tm_smooth3d_info h = stack::smooth(host, sm, true);
    std::printf("stack-smooth: nodes %llu interior %llu sweeps %llu frozen %llu J<0 %llu -> %llu\n", static_cast<unsigned long long>(d.nodes),
                static_cast<unsigned long long>(d.interior), static_cast<unsigned long long>(d.sweeps_done), static_cast<unsigned long long>(d.frozen),
                static_cast<unsigned long long>(d.first_neg), static_cast<unsigned long long>(d.last_neg));
    std::printf("stack-smooth: sum of squared updates first %.17g last %.17g max update %.17g at node %llu\n", d.first_sum_sq, d.last_sum_sq, d.last_max_update,
                static_cast<unsigned long long>(d.last_max_node));
    std::printf("stack-smooth: max |f| %.17g %.17g %.17g\n", d.control_max[0], d.control_max[1], d.control_max[2]);
    const std::size_t n = dev.x.size();
    bool same = n == host.x.size() && std::memcmp(dev.x.data(), host.x.data(), 8 * n) == 0 && std::memcmp(dev.y.data(), host.y.data(), 8 * n) == 0 &&
                std::memcmp(dev.z.data(), host.z.data(), 8 * n) == 0;
    tm_smooth3d_info a = d, b = h;
    a.first_sum_sq = a.last_sum_sq = b.first_sum_sq = b.last_sum_sq = 0.0;
    const double bound = 2.0 * static_cast<double>(d.interior) * 0x1p-53;
    same = same && std::memcmp(&a, &b, sizeof(a)) == 0 && std::fabs(d.first_sum_sq - h.first_sum_sq) <= bound * h.first_sum_sq &&
           std::fabs(d.last_sum_sq - h.last_sum_sq) <= bound * h.last_sum_sq;
    bool held = true, moved = false;
    for (std::size_t k = 0; k < nlayers; ++k)
        for (std::size_t j = 0; j < nj; ++j)
            for (std::size_t i = 0; i < ni; ++i) {
                const std::size_t o = (k * nj + j) * ni + i;
                const bool face = i == 0 || j == 0 || k == 0 || i + 1 == ni || j + 1 == nj || k + 1 == nlayers;
                const bool eq = dev.x[o] == before.x[o] && dev.y[o] == before.y[o] && dev.z[o] == before.z[o];
                if (face && !eq) held = false;
                if (!face && !eq) moved = true;
            }
    std::printf("stack-smooth: faces held: %s\n", held ? "yes" : "no");
    std::printf("stack-smooth: device equals host: %s\n", same ? "yes" : "no");
    return same && held && (moved || sweeps == 0 || d.interior == 0) ? 0 : 1;
}

// tm_harness stack-elevate <ni> <nj> <ncuts> <nlayers> <order>: the cuts of `stack`; Gauss-Lobatto hexahedra of `order` from the
// coordinates resident in the handles (stack::elevate -> tm_stack_smoothers_elevate), compared with the CPU's evaluation of the downloaded
// coordinates (the planar mapping: planes, scaled Jacobians and the record bit for bit); the nodes at element corners must be the nodes
// tm_stack_smoothers returns for the same handles.
static int stackElevate(std::size_t ni, std::size_t nj, std::size_t ncuts, std::size_t nlayers, int order) {
    if (ncuts < 2 || nlayers < 2) throw Error(TM_E_ARG, "stack-elevate <ni> <nj> <ncuts> <nlayers> <order>: at least two cuts and two layers");
    smoothing::solver::Option opt;
    opt.inner = TM_INNER_RELAX;
    std::vector<discrete::Mesh> meshes;
    meshes.reserve(ncuts);
    for (std::size_t c = 0; c < ncuts; ++c) meshes.push_back(buildSingle(ni, nj, 0.05 + 0.001 * static_cast<double>(c)));
    std::vector<std::unique_ptr<smoothing::smooth::Smoother>> handles;
    std::vector<smoothing::smooth::Smoother*> cuts;
    std::vector<discrete::Mesh*> host_cuts;
    for (std::size_t c = 0; c < ncuts; ++c) {
        handles.push_back(std::make_unique<smoothing::smooth::Smoother>(meshes[c], opt, smoothing::wall_control_function::Algorithm::laplace()));
        handles.back()->iterate(5);
        cuts.push_back(handles.back().get());
        host_cuts.push_back(&meshes[c]);
    }
    stack::Option so;
    for (std::size_t c = 0; c < ncuts; ++c) so.span.push_back(static_cast<double>(c));
    const double z1 = so.span.back();
    for (std::size_t k = 0; k < nlayers; ++k) so.layers.push_back(k + 1 == nlayers ? z1 : z1 * (static_cast<double>(k) / static_cast<double>(nlayers - 1)));
    highorder::Option ho;
    ho.order = order;
    const std::size_t p = static_cast<std::size_t>(order > 0 ? order : 1), Eg = (nlayers - 1) / p;
    const stack::Elevated3d dev = stack::elevate(cuts, so, ho, 0, 0, Eg);
    const stack::Block3d fine = stack::stack_block(cuts, so, 0, 0, nlayers);
    for (auto& h : handles) h->download();
    const stack::Elevated3d host = stack::elevate(host_cuts, so, ho, 0, 0, Eg, true);
    const tm_ho3_quality& q = dev.quality;
    std::printf("stack-elevate: hexahedra %llu invalid %llu min sj %.17g at (e %llu, f %llu, g %llu) jacobian %.17g .. %.17g orientation %d order %d\n",
                static_cast<unsigned long long>(q.elements), static_cast<unsigned long long>(q.invalid), q.min_scaled_jacobian, static_cast<unsigned long long>(q.worst_e),
                static_cast<unsigned long long>(q.worst_f), static_cast<unsigned long long>(q.worst_g), q.min_jacobian, q.max_jacobian, q.orientation, q.order);
    bool corners = dev.nk == nlayers;
    for (std::size_t k = 0; corners && k < nlayers; k += p)
        for (std::size_t j = 0; j < nj; j += p)
            for (std::size_t i = 0; i < ni; i += p) {
                const std::size_t o = (k * nj + j) * ni + i;
                if (!(dev.x[o] == fine.x[o] && dev.y[o] == fine.y[o] && dev.z[o] == fine.z[o])) corners = false;
            }
    std::printf("stack-elevate: corners unchanged: %s\n", corners ? "yes" : "no");
    const auto same_bits = [](const std::vector<double>& a, const std::vector<double>& b) {
        return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0);
    };
    const bool same = same_bits(dev.x, host.x) && same_bits(dev.y, host.y) && same_bits(dev.z, host.z) && same_bits(dev.sj, host.sj) &&
                      std::memcmp(&dev.quality, &host.quality, sizeof(tm_ho3_quality)) == 0;
    std::printf("stack-elevate: device equals host: %s\n", same ? "yes" : "no");
    return corners && same ? 0 : 1;
}

// tm_harness stack-certify <ni> <nj> <ncuts> <nlayers> <order>: the cuts of `stack-elevate`; the certificate of the curved hexahedra from the
// coordinates resident in the handles (stack::certify -> tm_stack_smoothers_certify, kernel K17), compared with the CPU's evaluation of
// the downloaded coordinates (the planar mapping: record, status and bounds bit for bit).
static int stackCertify(std::size_t ni, std::size_t nj, std::size_t ncuts, std::size_t nlayers, int order) {
    if (ncuts < 2 || nlayers < 2) throw Error(TM_E_ARG, "stack-certify <ni> <nj> <ncuts> <nlayers> <order>: at least two cuts and two layers");
    smoothing::solver::Option opt;
    opt.inner = TM_INNER_RELAX;
    std::vector<discrete::Mesh> meshes;
    meshes.reserve(ncuts);
    for (std::size_t c = 0; c < ncuts; ++c) meshes.push_back(buildSingle(ni, nj, 0.05 + 0.001 * static_cast<double>(c)));
    std::vector<std::unique_ptr<smoothing::smooth::Smoother>> handles;
    std::vector<smoothing::smooth::Smoother*> cuts;
    std::vector<discrete::Mesh*> host_cuts;
    for (std::size_t c = 0; c < ncuts; ++c) {
        handles.push_back(std::make_unique<smoothing::smooth::Smoother>(meshes[c], opt, smoothing::wall_control_function::Algorithm::laplace()));
        handles.back()->iterate(5);
        cuts.push_back(handles.back().get());
        host_cuts.push_back(&meshes[c]);
    }
    stack::Option so;
    for (std::size_t c = 0; c < ncuts; ++c) so.span.push_back(static_cast<double>(c));
    const double z1 = so.span.back();
    for (std::size_t k = 0; k < nlayers; ++k) so.layers.push_back(k + 1 == nlayers ? z1 : z1 * (static_cast<double>(k) / static_cast<double>(nlayers - 1)));
    highorder::Option ho;
    ho.order = order;
    const stack::Certified3d dev = stack::certify(cuts, so, ho, 0);
    for (auto& h : handles) h->download();
    const stack::Certified3d host = stack::certify(host_cuts, so, ho, 0, 2, true);
    const tm_ho3_certificate& c = dev.certificate;
    std::printf("stack-certify: hexahedra %llu proven %llu invalid %llu undecided %llu hidden invalid %llu min scaled bound %.17g at (e %llu, f %llu, g %llu) orientation %d order %d depth %d\n",
                static_cast<unsigned long long>(c.elements), static_cast<unsigned long long>(c.proven), static_cast<unsigned long long>(c.invalid),
                static_cast<unsigned long long>(c.undecided), static_cast<unsigned long long>(c.hidden_invalid), c.min_scaled_bound,
                static_cast<unsigned long long>(c.worst_e), static_cast<unsigned long long>(c.worst_f), static_cast<unsigned long long>(c.worst_g), c.orientation, c.order,
                c.max_depth);
    const bool adds = c.proven + c.invalid + c.undecided == c.elements && c.elements == dev.Ei * dev.Ej * dev.Eg;
    std::printf("stack-certify: counts add up: %s\n", adds ? "yes" : "no");
    const bool same = dev.status == host.status && dev.bounds.size() == host.bounds.size() &&
                      (dev.bounds.empty() || std::memcmp(dev.bounds.data(), host.bounds.data(), sizeof(double) * dev.bounds.size()) == 0) &&
                      std::memcmp(&dev.certificate, &host.certificate, sizeof(tm_ho3_certificate)) == 0;
    std::printf("stack-certify: device equals host: %s\n", same ? "yes" : "no");
    return adds && same ? 0 : 1;
}

// tm_harness elevate <ni> <nj> <order>: the config-2 block, five relaxation sweeps; Gauss-Lobatto elements of `order` from the
// coordinates resident in the handle (highorder::elevate -> tm_smoother_elevate), compared with the CPU's evaluation of the
// downloaded coordinates (planes, scaled Jacobians and the record bit for bit); element corners must be the smoothed nodes.
static int elevateBlock(std::size_t ni, std::size_t nj, int order) {
    smoothing::solver::Option opt;
    opt.inner = TM_INNER_RELAX;
    discrete::Mesh mesh = buildSingle(ni, nj);
    highorder::Option ho;
    ho.order = order;
    highorder::check(mesh, ho);
    smoothing::smooth::Smoother sm(mesh, opt, smoothing::wall_control_function::Algorithm::laplace());
    sm.iterate(5);
    const highorder::Elevated dev = highorder::elevate(sm, ho, 0);
    sm.download();
    const highorder::Elevated host = highorder::elevate(mesh, ho, 0, true);
    const tm_ho_quality& q = dev.quality;
    std::printf("elevate: elements %llu invalid %llu min sj %.17g at (e %llu, f %llu) jacobian %.17g .. %.17g orientation %d order %d\n",
                static_cast<unsigned long long>(q.elements), static_cast<unsigned long long>(q.invalid), q.min_scaled_jacobian,
                static_cast<unsigned long long>(q.worst_e), static_cast<unsigned long long>(q.worst_f), q.min_jacobian, q.max_jacobian, q.orientation, q.order);
    bool corners = true;
    const std::size_t p = static_cast<std::size_t>(order);
    for (std::size_t i = 0; i < ni; i += p)
        for (std::size_t j = 0; j < nj; j += p) {
            const Vec2d v = mesh.blocks[0].points.getIndex(i, j);
            if (!(dev.x[j * ni + i] == v.data[0] && dev.y[j * ni + i] == v.data[1])) corners = false;
        }
    std::printf("elevate: corners unchanged: %s\n", corners ? "yes" : "no");
    const auto same_bits = [](const std::vector<double>& a, const std::vector<double>& b) {
        return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0);
    };
    const bool same = same_bits(dev.x, host.x) && same_bits(dev.y, host.y) && same_bits(dev.sj, host.sj) && std::memcmp(&dev.quality, &host.quality, sizeof(tm_ho_quality)) == 0;
    std::printf("elevate: device equals host: %s\n", same ? "yes" : "no");
    return corners && same ? 0 : 1;
}

// tm_harness certify <ni> <nj> <order>: the block of `elevate`, five relaxation sweeps; the certificate of its elements from the
// coordinates resident in the handle (highorder::certify -> tm_smoother_certify), compared with the CPU's evaluation of the downloaded
// coordinates (record, status and bounds bit for bit).
static int certifyBlock(std::size_t ni, std::size_t nj, int order) {
    smoothing::solver::Option opt;
    opt.inner = TM_INNER_RELAX;
    discrete::Mesh mesh = buildSingle(ni, nj);
    highorder::Option ho;
    ho.order = order;
    highorder::check(mesh, ho);
    smoothing::smooth::Smoother sm(mesh, opt, smoothing::wall_control_function::Algorithm::laplace());
    sm.iterate(5);
    const highorder::Certified dev = highorder::certify(sm, ho, 0);
    sm.download();
    const highorder::Certified host = highorder::certify(mesh, ho, 0, 3, true);
    const tm_ho_certificate& c = dev.certificate;
    std::printf("certify: elements %llu proven %llu invalid %llu undecided %llu hidden invalid %llu min scaled bound %.17g at (e %llu, f %llu) orientation %d order %d depth %d\n",
                static_cast<unsigned long long>(c.elements), static_cast<unsigned long long>(c.proven), static_cast<unsigned long long>(c.invalid),
                static_cast<unsigned long long>(c.undecided), static_cast<unsigned long long>(c.hidden_invalid), c.min_scaled_bound,
                static_cast<unsigned long long>(c.worst_e), static_cast<unsigned long long>(c.worst_f), c.orientation, c.order, c.max_depth);
    const bool adds = c.proven + c.invalid + c.undecided == c.elements && c.elements == dev.Ei * dev.Ej;
    std::printf("certify: counts add up: %s\n", adds ? "yes" : "no");
    const bool same = dev.status == host.status && dev.bounds.size() == host.bounds.size() &&
                      (dev.bounds.empty() || std::memcmp(dev.bounds.data(), host.bounds.data(), sizeof(double) * dev.bounds.size()) == 0) &&
                      std::memcmp(&dev.certificate, &host.certificate, sizeof(tm_ho_certificate)) == 0;
    std::printf("certify: device equals host: %s\n", same ? "yes" : "no");
    return adds && same ? 0 : 1;
}

// tm_harness weld <ni> <nj> <nblocks>: the config-4 strip, two Picard iterations; map and welded points from the coordinates resident in
// the handle (weld::points -> tm_smoother_weld), quadrilaterals from the map (weld::cells), compared with the CPU's map and cells; the
// strip welds to nblocks * ni * nj - (nblocks - 1) * nj nodes.
static int weldStrip(std::size_t ni, std::size_t nj, std::size_t nb) {
    discrete::Mesh mesh = buildStrip(nb, ni, nj);
    smoothing::smooth::Smoother sm(mesh, smoothing::solver::Option{}, smoothing::wall_control_function::Algorithm::laplace());
    sm.iterate(2);
    weld::Map dev;
    const weld::Points pts = weld::points(sm, &dev);
    const std::vector<int32_t> cells = weld::cells(mesh, dev);
    const weld::Map host = weld::map(mesh, true);
    const tm_weld_info& w = pts.info;
    std::printf("weld: %llu -> %llu nodes, classes of 2 / 3 / 4 / 5+: %llu / %llu / %llu / %llu, max_gap %.3e at node %llu, %zu quadrilaterals\n",
                static_cast<unsigned long long>(w.nodes_in), static_cast<unsigned long long>(w.nodes_out), static_cast<unsigned long long>(w.classes_2),
                static_cast<unsigned long long>(w.classes_3), static_cast<unsigned long long>(w.classes_4), static_cast<unsigned long long>(w.classes_5_up), w.max_gap,
                static_cast<unsigned long long>(w.gap_node), cells.size() / 4);
    const bool count = w.nodes_out == nb * ni * nj - (nb - 1) * nj && pts.x.size() == w.nodes_out && cells.size() == 4 * nb * (ni - 1) * (nj - 1);
    std::printf("weld: node and cell counts: %s\n", count ? "yes" : "no");
    const bool same = dev.map == host.map && host.info.nodes_out == w.nodes_out && host.info.classes_2 == w.classes_2 && cells == weld::cells(mesh, host, 1, 0, true);
    std::printf("weld: device equals host: %s\n", same ? "yes" : "no");
    return count && same ? 0 : 1;
}

// tm_harness weld-boundary <ni> <nj> <nblocks> [nlayers]: the boundary of the welded strip (kernel K19).  Without layers: faces and measured
// patches from the coordinates resident in the handle (weld::boundary(sm) -> tm_smoother_weld_boundary) against the CPU's faces and sums on
// the welded points.  With layers: the welded plane repeated at z = 0.1 k, faces and sums on the device against the CPU's.  The strip has
// 2 (nj - 1) + 2 nblocks (ni - 1) boundary edges in one loop.
static int weldBoundaryStrip(std::size_t ni, std::size_t nj, std::size_t nb, std::size_t nk) {
    discrete::Mesh mesh = buildStrip(nb, ni, nj);
    smoothing::smooth::Smoother sm(mesh, smoothing::solver::Option{}, smoothing::wall_control_function::Algorithm::laplace());
    sm.iterate(2);
    weld::Map map;
    const weld::Points pts = weld::points(sm, &map);
    std::vector<int32_t> orientation;
    for (const auto& q : sm.quality().per_block) orientation.push_back(q.orientation);
    weld::Boundary dev, host = weld::boundary(mesh, map, 1, nk, orientation, true);
    if (nk < 2) {
        dev = weld::boundary(sm);
        weld::measure(host, 1, pts.x, pts.y, nullptr, true);
    } else {
        std::vector<double> x, y, z;
        for (std::size_t k = 0; k < nk; ++k) {
            x.insert(x.end(), pts.x.begin(), pts.x.end());
            y.insert(y.end(), pts.y.begin(), pts.y.end());
            z.insert(z.end(), pts.x.size(), 0.1 * static_cast<double>(k));
        }
        dev = weld::boundary(mesh, map, 1, nk, orientation);
        weld::measure(dev, 1, x, y, &z);
        weld::measure(host, 1, x, y, &z, true);
    }
    const std::size_t edges = 2 * (nj - 1) + 2 * nb * (ni - 1);
    std::printf("weld-boundary: %llu faces of %llu nodes in %zu patches, %llu loop(s), %llu irregular nodes\n", static_cast<unsigned long long>(host.info.faces),
                static_cast<unsigned long long>(host.info.nodes_per_face), host.patches.size(), static_cast<unsigned long long>(host.info.loops),
                static_cast<unsigned long long>(host.info.irregular_nodes));
    const bool count = host.info.loops == 1 && host.info.irregular_nodes == 0 &&
                       host.info.faces == (nk < 2 ? edges : edges * (nk - 1) + 2 * nb * (ni - 1) * (nj - 1));
    std::printf("weld-boundary: face count and loops: %s\n", count ? "yes" : "no");
    bool same = dev.faces == host.faces && dev.face_patch == host.face_patch && dev.patches.size() == host.patches.size();
    double total = 0.0, normal[3] = {0.0, 0.0, 0.0};
    for (std::size_t q = 0; same && q < host.patches.size(); ++q) {
        const tm_weld_patch &a = dev.patches[q], &b = host.patches[q];
        std::printf("weld-boundary: patch %zu kind %d: %llu faces, measure %.15e (device) %.15e (host), moment %.15e\n", q, a.kind,
                    static_cast<unsigned long long>(a.faces), a.measure, b.measure, a.moment);
        // the terms of the measure are all positive: the two orders of summation differ by at most 2 (n - 1) 2^-53 of it
        same = same && a.faces == b.faces && std::fabs(a.measure - b.measure) <= 2.0 * static_cast<double>(a.faces) * 0x1p-53 * b.measure;
        total += a.moment;
        for (int d = 0; d < 3; ++d) normal[d] += a.normal[d];
    }
    std::printf("weld-boundary: sum of normals (%.3e, %.3e, %.3e), enclosed %s %.15e\n", normal[0], normal[1], normal[2], nk < 2 ? "area" : "volume",
                total / (nk < 2 ? 2.0 : 3.0));
    std::printf("weld-boundary: device equals host: %s\n", same ? "yes" : "no");
    return count && same ? 0 : 1;
}

// tm_harness wall-distance <ni> <nj> <nblocks> [nlayers]: the wall distance of the welded strip (kernel K20), every boundary face a wall.
// Without layers: from the coordinates resident in the handle (weld::wall_distance(sm) -> tm_smoother_wall_distance) against the host twin
// on the welded points.  With layers: the welded plane repeated at z = 0.1 k, device against host twin, culled against not culled.
static int wallDistanceStrip(std::size_t ni, std::size_t nj, std::size_t nb, std::size_t nk) {
    discrete::Mesh mesh = buildStrip(nb, ni, nj);
    smoothing::smooth::Smoother sm(mesh, smoothing::solver::Option{}, smoothing::wall_control_function::Algorithm::laplace());
    sm.iterate(2);
    weld::Map map;
    const weld::Points pts = weld::points(sm, &map);
    std::vector<int32_t> orientation;
    for (const auto& q : sm.quality().per_block) orientation.push_back(q.orientation);
    const weld::Boundary b = weld::boundary(mesh, map, 1, nk, orientation, true);
    std::vector<double> x = pts.x, y = pts.y, z;
    if (nk >= 2) {
        x.clear(), y.clear();
        for (std::size_t k = 0; k < nk; ++k) {
            x.insert(x.end(), pts.x.begin(), pts.x.end());
            y.insert(y.end(), pts.y.begin(), pts.y.end());
            z.insert(z.end(), pts.x.size(), 0.1 * static_cast<double>(k));
        }
    }
    const weld::WallDistance host = weld::wall_distance(mesh, b, nk, x, y, nk >= 2 ? &z : nullptr, 0, {}, true);
    const weld::WallDistance dev = nk < 2 ? weld::wall_distance(sm) : weld::wall_distance(mesh, b, nk, x, y, &z);
    const weld::WallDistance every = weld::wall_distance(mesh, b, nk, x, y, nk >= 2 ? &z : nullptr, 0, {}, false, TM_WALL_NO_CULL);
    const tm_wall_info& i = dev.info;
    std::printf("wall-distance: %llu points, %llu faces, %llu primitives in %llu groups, %llu image(s)\n", static_cast<unsigned long long>(i.points),
                static_cast<unsigned long long>(i.faces), static_cast<unsigned long long>(i.primitives), static_cast<unsigned long long>(i.groups),
                static_cast<unsigned long long>(i.images));
    std::printf("wall-distance: %llu on the wall, %llu NaN, %llu nearest to an image, maximum %.15e at node %llu\n", static_cast<unsigned long long>(i.on_wall),
                static_cast<unsigned long long>(i.nan_points), static_cast<unsigned long long>(i.nearest_via_image), i.max_distance,
                static_cast<unsigned long long>(i.max_point));
    std::printf("wall-distance: pairs evaluated %llu culled, %llu not culled, %llu on the host\n", static_cast<unsigned long long>(i.pairs_evaluated),
                static_cast<unsigned long long>(every.info.pairs_evaluated), static_cast<unsigned long long>(host.info.pairs_evaluated));
    auto equal = [](const weld::WallDistance& a, const weld::WallDistance& c) {
        return a.distance == c.distance && a.face == c.face && a.image == c.image && a.info.on_wall == c.info.on_wall && a.info.max_point == c.info.max_point &&
               a.info.max_distance == c.info.max_distance && a.info.nearest_via_image == c.info.nearest_via_image && a.info.nan_points == c.info.nan_points;
    };
    const bool same = equal(dev, host), cull = equal(dev, every);
    std::printf("wall-distance: device equals host: %s\n", same ? "yes" : "no");
    std::printf("wall-distance: culled equals not culled: %s\n", cull ? "yes" : "no");
    return same && cull && i.on_wall > 0 ? 0 : 1;
}

// tm_harness fv <ni> <nj> <nblocks> [nlayers]: the face-based view of the welded strip and its finite-volume metrics (kernel K21).  Without
// layers: also the record from the coordinates resident in the handle (weld::fv_report(sm) -> tm_smoother_fv_report).  With layers: the
// welded plane repeated at z = 0.1 k.  Lists, volumes, cosines and every extreme of the record are compared with the CPU's bit for bit;
// total_volume, summed in another order, within 2 (n - 1) 2^-53 sum |V|.
static int fvStrip(std::size_t ni, std::size_t nj, std::size_t nb, std::size_t nk) {
    discrete::Mesh mesh = buildStrip(nb, ni, nj);
    smoothing::smooth::Smoother sm(mesh, smoothing::solver::Option{}, smoothing::wall_control_function::Algorithm::laplace());
    sm.iterate(2);
    weld::Map map;
    const weld::Points pts = weld::points(sm, &map);
    std::vector<int32_t> orientation;
    for (const auto& q : sm.quality().per_block) orientation.push_back(q.orientation);
    std::vector<double> x = pts.x, y = pts.y, z;
    if (nk >= 2) {
        x.clear(), y.clear();
        for (std::size_t k = 0; k < nk; ++k) {
            x.insert(x.end(), pts.x.begin(), pts.x.end());
            y.insert(y.end(), pts.y.begin(), pts.y.end());
            z.insert(z.end(), pts.x.size(), 0.1 * static_cast<double>(k));
        }
    }
    const weld::Faces host = weld::faces(mesh, map, nk, orientation, true), dev = weld::faces(mesh, map, nk, orientation);
    const weld::FvMetrics mh = weld::fv_metrics(host, x, y, nk >= 2 ? &z : nullptr, true), md = weld::fv_metrics(dev, x, y, nk >= 2 ? &z : nullptr);
    const tm_fv_info& i = md.info;
    std::printf("fv: %llu cells, %llu internal and %llu boundary faces of %llu nodes\n", static_cast<unsigned long long>(i.cells),
                static_cast<unsigned long long>(i.internal_faces), static_cast<unsigned long long>(i.boundary_faces), static_cast<unsigned long long>(host.plan.nodes_per_face));
    std::printf("fv: volume %.15e .. %.15e, total %.15e, %llu cells with V <= 0, max closedness %.3e\n", i.min_volume, i.max_volume, i.total_volume,
                static_cast<unsigned long long>(i.negative_cells), i.max_closedness);
    std::printf("fv: min cos %.15f at face %llu, max skewness %.15f at face %llu\n", i.min_cos, static_cast<unsigned long long>(i.min_cos_face), i.max_skewness,
                static_cast<unsigned long long>(i.max_skewness_face));
    double mag = 0.0;
    for (double v : mh.volume) mag += std::fabs(v);
    auto equal = [&](const tm_fv_info& a, const tm_fv_info& b) {
        tm_fv_info c = a;
        c.total_volume = b.total_volume;
        return std::memcmp(&c, &b, sizeof(c)) == 0 && std::fabs(a.total_volume - b.total_volume) <= 2.0 * static_cast<double>(b.cells - 1) * 0x1p-53 * mag;
    };
    const std::size_t cells = nb * (ni - 1) * (nj - 1) * (nk >= 2 ? nk - 1 : 1);
    const bool count = i.cells == cells && i.internal_faces == ((nk >= 2 ? 6 : 4) * cells - i.boundary_faces) / 2 && i.negative_cells == 0;
    std::printf("fv: cell and face counts: %s\n", count ? "yes" : "no");
    bool same = dev.faces == host.faces && dev.owner == host.owner && dev.neighbour == host.neighbour && dev.cell_faces == host.cell_faces &&
                std::memcmp(md.volume.data(), mh.volume.data(), sizeof(double) * mh.volume.size()) == 0 &&
                std::memcmp(md.cos.data(), mh.cos.data(), sizeof(double) * mh.cos.size()) == 0 && equal(md.info, mh.info);
    if (nk < 2) same = same && equal(weld::fv_report(sm, orientation), mh.info);
    std::printf("fv: device equals host: %s\n", same ? "yes" : "no");
    return count && same ? 0 : 1;
}

int main(int argc, char** argv) {
    try {
        if (argc >= 5 && std::strcmp(argv[1], "fv") == 0)
            return fvStrip(std::strtoull(argv[2], nullptr, 10), std::strtoull(argv[3], nullptr, 10), std::strtoull(argv[4], nullptr, 10),
                           argc >= 6 ? std::strtoull(argv[5], nullptr, 10) : 0);
        if (argc >= 5 && std::strcmp(argv[1], "wall-distance") == 0)
            return wallDistanceStrip(std::strtoull(argv[2], nullptr, 10), std::strtoull(argv[3], nullptr, 10), std::strtoull(argv[4], nullptr, 10),
                                     argc >= 6 ? std::strtoull(argv[5], nullptr, 10) : 0);
        if (argc >= 5 && std::strcmp(argv[1], "weld-boundary") == 0)
            return weldBoundaryStrip(std::strtoull(argv[2], nullptr, 10), std::strtoull(argv[3], nullptr, 10), std::strtoull(argv[4], nullptr, 10),
                                     argc >= 6 ? std::strtoull(argv[5], nullptr, 10) : 0);
        if (argc >= 5 && std::strcmp(argv[1], "weld") == 0)
            return weldStrip(std::strtoull(argv[2], nullptr, 10), std::strtoull(argv[3], nullptr, 10), std::strtoull(argv[4], nullptr, 10));
        if (argc >= 5 && std::strcmp(argv[1], "certify") == 0)
            return certifyBlock(std::strtoull(argv[2], nullptr, 10), std::strtoull(argv[3], nullptr, 10), static_cast<int>(std::strtol(argv[4], nullptr, 10)));
        if (argc >= 5 && std::strcmp(argv[1], "elevate") == 0)
            return elevateBlock(std::strtoull(argv[2], nullptr, 10), std::strtoull(argv[3], nullptr, 10), static_cast<int>(std::strtol(argv[4], nullptr, 10)));
        if (argc >= 7 && std::strcmp(argv[1], "stack-certify") == 0)
            return stackCertify(std::strtoull(argv[2], nullptr, 10), std::strtoull(argv[3], nullptr, 10), std::strtoull(argv[4], nullptr, 10), std::strtoull(argv[5], nullptr, 10),
                                static_cast<int>(std::strtol(argv[6], nullptr, 10)));
        if (argc >= 7 && std::strcmp(argv[1], "stack-elevate") == 0)
            return stackElevate(std::strtoull(argv[2], nullptr, 10), std::strtoull(argv[3], nullptr, 10), std::strtoull(argv[4], nullptr, 10), std::strtoull(argv[5], nullptr, 10),
                                static_cast<int>(std::strtol(argv[6], nullptr, 10)));
        if (argc >= 6 && std::strcmp(argv[1], "stack-smooth") == 0)
            return stackSmooth(std::strtoull(argv[2], nullptr, 10), std::strtoull(argv[3], nullptr, 10), std::strtoull(argv[4], nullptr, 10), std::strtoull(argv[5], nullptr, 10));
        if (argc >= 6 && std::strcmp(argv[1], "stack-quality") == 0)
            return stackQuality(std::strtoull(argv[2], nullptr, 10), std::strtoull(argv[3], nullptr, 10), std::strtoull(argv[4], nullptr, 10), std::strtoull(argv[5], nullptr, 10));
        if (argc >= 6 && std::strcmp(argv[1], "stack-revolution") == 0)
            return stackRevolution(std::strtoull(argv[2], nullptr, 10), std::strtoull(argv[3], nullptr, 10), std::strtoull(argv[4], nullptr, 10), std::strtoull(argv[5], nullptr, 10));
        if (argc >= 6 && std::strcmp(argv[1], "stack") == 0)
            return stackCuts(std::strtoull(argv[2], nullptr, 10), std::strtoull(argv[3], nullptr, 10), std::strtoull(argv[4], nullptr, 10), std::strtoull(argv[5], nullptr, 10));
        if (argc >= 2 && std::strcmp(argv[1], "csr") == 0) return csrKat();
        if (argc >= 5 && std::strcmp(argv[1], "tm") == 0)
            return thomasMiddlecoff(std::strtoull(argv[2], nullptr, 10), std::strtoull(argv[3], nullptr, 10), std::strtoull(argv[4], nullptr, 10));
        if (argc >= 2 && std::strcmp(argv[1], "ranks") == 0) return runRank(argc, argv);
        if (argc < 5) {
            std::fprintf(stderr, "usage: %s strip <nblocks> <ni> <nj> <iterations> [relax|bicgstab|mg] [until <tol>] [write <file.xyz>] [dump.bin]\n       %s single <ni> <nj> <iterations> [relax|bicgstab|mg] [until <tol>] [write <file.xyz>] [dump.bin]\n       %s stack <ni> <nj> <ncuts> <nlayers>\n       %s stack-quality <ni> <nj> <ncuts> <nlayers>\n       %s stack-smooth <ni> <nj> <nk> <sweeps>\n       %s stack-elevate <ni> <nj> <ncuts> <nlayers> <order>\n       %s stack-certify <ni> <nj> <ncuts> <nlayers> <order>\n       %s stack-revolution <ni> <nj> <ncuts> <nlayers>\n       %s elevate <ni> <nj> <order>\n       %s certify <ni> <nj> <order>\n       %s weld <ni> <nj> <nblocks>\n       %s weld-boundary <ni> <nj> <nblocks> [nlayers]\n       %s wall-distance <ni> <nj> <nblocks> [nlayers]\n       %s fv <ni> <nj> <nblocks> [nlayers]\n", argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0]);
            return 2;
        }
        int a = 2;
        discrete::Mesh mesh;
        if (std::strcmp(argv[1], "strip") == 0) {
            const std::size_t nb = std::strtoull(argv[a++], nullptr, 10), ni = std::strtoull(argv[a++], nullptr, 10), nj = std::strtoull(argv[a++], nullptr, 10);
            mesh = buildStrip(nb, ni, nj);
        } else {
            const std::size_t ni = std::strtoull(argv[a++], nullptr, 10), nj = std::strtoull(argv[a++], nullptr, 10);
            mesh = buildSingle(ni, nj);
        }
        const std::size_t iterations = std::strtoull(argv[a++], nullptr, 10);
        smoothing::solver::Option opt;
        if (a < argc && std::strcmp(argv[a], "relax") == 0) opt.inner = TM_INNER_RELAX;
        if (a < argc && std::strcmp(argv[a], "mg") == 0) opt.inner = TM_INNER_MG_BICGSTAB;
        if (a < argc && std::strcmp(argv[a], "gmres") == 0) opt.inner = TM_INNER_GMRES;   // GMRES(30) on the device (GMRES.zig:300-423)
        if (a < argc && std::strcmp(argv[a], "auto") == 0) opt.inner = TM_INNER_AUTO;
        const bool tight_default = a < argc && (std::strcmp(argv[a], "gmres") == 0 || std::strcmp(argv[a], "auto") == 0);
        if (a < argc && (std::strcmp(argv[a], "relax") == 0 || std::strcmp(argv[a], "bicgstab") == 0 || std::strcmp(argv[a], "mg") == 0 || tight_default)) ++a;
        opt.rtol = tight_default ? 0.0 : 1e-13;   // gmres / auto: the library's own default tolerance
        opt.max_inner = tight_default ? 0 : 5000;
        // "until <tol>" after the solver name: iterate to a residual through the device-resident handle instead of a fixed count
        double until = 0.0;
        std::string plot3d;
        if (a + 1 < argc && std::strcmp(argv[a], "until") == 0) {
            until = std::strtod(argv[a + 1], nullptr);
            a += 2;
        }
        if (a + 1 < argc && std::strcmp(argv[a], "write") == 0) {
            plot3d = argv[a + 1];
            a += 2;
        }
        // the reference's two log lines per outer iteration (smooth.zig:105, 136-137)
        tm_set_log([](void*, int32_t what, uint64_t n, double v) {
            if (what == 0) std::printf("info(smoothing): iteration: %llu\n", static_cast<unsigned long long>(n));
            else std::printf("info(smoothing): \tresidual: %.17g\n", v);
        }, nullptr);
        tm_stats st{};
        auto report = [](const char* stage, const tm_quality& q) {
            std::printf("info(quality): %s: cells %llu inverted %llu degenerate %llu min scaled jacobian %.4f at (block %llu, i %llu, j %llu) angles %.2f..%.2f deg max aspect %.1f\n",
                        stage, static_cast<unsigned long long>(q.cells), static_cast<unsigned long long>(q.inverted), static_cast<unsigned long long>(q.degenerate),
                        q.min_scaled_jacobian, static_cast<unsigned long long>(q.worst_block), static_cast<unsigned long long>(q.worst_i),
                        static_cast<unsigned long long>(q.worst_j), q.min_angle_deg, q.max_angle_deg, q.max_aspect);
        };
        report("seed", mesh.quality().total);   // Mesh::quality: host coordinates, evaluated on the device
        if (until > 0.0 || !plot3d.empty()) {
            smoothing::smooth::Smoother sm(mesh, opt, smoothing::wall_control_function::Algorithm::laplace());
            if (until > 0.0) {
                const bool reached = sm.iterateUntil(until, iterations, &st);
                std::printf("reached %d\n", reached ? 1 : 0);
            } else {
                st = sm.iterate(iterations);
            }
            report("smoothed", sm.quality().total);   // Smoother::quality: the coordinates resident in the handle
            sm.download();
            if (!plot3d.empty()) sm.write(plot3d);
        } else {
            st = smoothing::smooth::mesh(mesh, iterations, opt, smoothing::wall_control_function::Algorithm::laplace());
            report("smoothed", mesh.quality().total);
        }
        tm_set_log(nullptr, nullptr);
        std::printf("info(smoothing): elapsed time for smoothing: %.2f s\n", st.seconds);   // smooth.zig:159
        std::printf("inner_iterations %llu operator_sweeps %llu not_converged %d scaled_residual_rms %.3e\n", static_cast<unsigned long long>(st.inner_iterations),
                    static_cast<unsigned long long>(st.operator_sweeps), st.not_converged, st.scaled_residual_rms);
        if (a < argc) {
            std::FILE* f = std::fopen(argv[a], "wb");
            if (!f) throw Error(TM_E_ARG, "cannot open dump file");
            for (const auto& b : mesh.blocks) std::fwrite(b.points.data.data(), sizeof(Vec2d), b.points.data.size(), f);
            std::fclose(f);
        }
        return 0;
    } catch (const core::Error& e) {
        std::fprintf(stderr, "error(%d): %s\n", e.code, e.what());
        return 1;
    }
}
