// turbomesh.hpp -- C++ host-side mirror of turbomesh's `core` module for the hot path, on top of the C-ABI of
// libtm_hip.so (include/tm_hip.h).  The reference's host language is Zig (no toolchain in this image); this header
// keeps its module / type / function names, argument meaning and error behaviour so a caller reads like the Zig code:
//
//   core::types      Vec2d, Mat2d (NaN-initialised, index = j + size[1]*i)      reference src/core/types.zig:6-101
//   core::clustering Uniform, Roberts, SingleHyperbolicClustering, create       src/core/clustering.zig:9-116
//   core::geometry   Line                                                        src/core/geometry.zig:17-41
//   core::boundary   Side, Range, Connection, Condition                          src/core/boundary.zig:8-187
//   core::discrete   Edge, EdgeView, Block2d, Mesh                               src/core/discrete.zig:12-217
//   core::tfi        linear2dBoundaryBlendedControlFunction, linear2d            src/core/tfi.zig:19-208
//   core::smoothing  solver::Option (+ .hip), wall_control_function::Algorithm, smooth::mesh
//                                                                                src/core/smoothing/{solver,wall_control_function,smooth}.zig
// Zig error unions become C++ exceptions of type core::Error carrying the tm_error code.
#pragma once
#include "../../include/tm_hip.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <variant>
#include <vector>

namespace core {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
inline void check(int rc) {
    if (rc < 0) throw Error(rc, tm_last_error());
}

namespace types {
using Index = std::size_t;   // types.zig:6
using Float = double;        // types.zig:7
struct Vec2d {               // types.zig:16-27
    Float data[2];
    static Vec2d init(Float a, Float b) { return Vec2d{{a, b}}; }
};
inline bool eqlApprox(Vec2d a, Vec2d b, Float tol) { return std::fabs(a.data[0] - b.data[0]) <= tol && std::fabs(a.data[1] - b.data[1]) <= tol; }
struct Mat2d {               // types.zig:78-101
    Index size[2];
    std::vector<Vec2d> data;
    static Mat2d init(Index n0, Index n1) {
        const Float nan = std::numeric_limits<Float>::quiet_NaN();
        Mat2d m{{n0, n1}, std::vector<Vec2d>(n0 * n1, Vec2d{{nan, nan}})};
        return m;
    }
    Index index(Index i, Index j) const { return j + size[1] * i; }
    Vec2d getIndex(Index i, Index j) const { return data[index(i, j)]; }
};
}  // namespace types

namespace clustering {   // clustering.zig
struct Uniform {};
struct Roberts { double alpha, beta; };
struct SingleHyperbolicClustering { double delta_s; };
using Function = std::variant<Uniform, Roberts, SingleHyperbolicClustering>;
inline std::vector<double> create(const Function& f, types::Index n) {   // clustering.zig:110-116
    std::vector<double> u(n);
    if (std::holds_alternative<Uniform>(f)) {
        for (types::Index i = 0; i < n; ++i) u[i] = static_cast<double>(i) / static_cast<double>(n - 1);
    } else if (const auto* r = std::get_if<Roberts>(&f)) {
        for (types::Index i = 0; i < n; ++i) {
            const double x = static_cast<double>(i) / static_cast<double>(n - 1);
            const double tmp = std::pow((r->beta + 1.0) / (r->beta - 1.0), (x - r->alpha) / (1.0 - r->alpha));
            const double tbar = (r->beta + 2.0 * r->alpha) * tmp - r->beta + 2.0 * r->alpha;
            u[i] = tbar / ((2.0 * r->alpha + 1.0) * (1.0 + tmp));
        }
    } else {
        const auto& h = std::get<SingleHyperbolicClustering>(f);
        const double n_1 = static_cast<double>(n - 1), y = 1.0 / (n_1 * h.delta_s);
        double delta;
        if (y < 2.7829681) {
            const double yb = y - 1.0;
            delta = std::sqrt(6.0 * yb) * (1.0 + yb * (-0.15 + yb * (0.057321429 + yb * (-0.024907295 + yb * (0.0077424461 - 0.0010794123 * yb)))));
        } else {
            const double w = 1.0 / y - 0.028527431, v = std::log(y);
            delta = v + (1.0 + 1.0 / v) * std::log(2.0 * v) - 0.02041793 + w * (0.24902722 + w * (1.9496443 + w * (-2.6294547 + 8.56795911 * w)));
        }
        for (types::Index i = 0; i < n; ++i) u[i] = static_cast<double>(i) / n_1;
        for (types::Index i = 1; i < n; ++i) u[i] = 1.0 + std::tanh(0.5 * delta * (u[i] - 1.0)) / std::tanh(0.5 * delta);
    }
    return u;
}
}  // namespace clustering

namespace geometry {   // geometry.zig:17-41
struct Line {
    types::Vec2d start, end;
    std::vector<types::Vec2d> interpolate(const std::vector<double>& u) const {
        std::vector<types::Vec2d> out(u.size());
        const double dx = end.data[0] - start.data[0], dy = end.data[1] - start.data[1];
        for (std::size_t i = 0; i < u.size(); ++i) out[i] = types::Vec2d{{start.data[0] + u[i] * dx, start.data[1] + u[i] * dy}};
        return out;
    }
};
}  // namespace geometry

namespace boundary {   // boundary.zig
enum class Side : uint32_t { i_min = 0, i_max = 1, j_min = 2, j_max = 3 };
enum class ConditionTag : uint32_t { wall = 0, inlet = 1, outlet = 2 };
struct Range {
    std::size_t block;
    Side side;
    std::size_t start, end;
    std::size_t len() const { return start > end ? start - end + 1 : end - start + 1; }
};
struct Connection {
    Range ranges[2];
    std::optional<types::Vec2d> periodicity;   // ?Vec2d
};
struct Condition {
    Range range;
    ConditionTag kind;
};
}  // namespace boundary

namespace tfi {   // tfi.zig
// tfi.zig:112-122: same argument order; the reference's asserts come back as core::Error
inline void linear2dBoundaryBlendedControlFunction(types::Mat2d& data, const std::vector<types::Vec2d>& x_i_min, const std::vector<types::Vec2d>& x_i_max,
                                                   const std::vector<types::Vec2d>& x_j_min, const std::vector<types::Vec2d>& x_j_max,
                                                   const std::vector<double>& s1, const std::vector<double>& s2, const std::vector<double>& t1,
                                                   const std::vector<double>& t2) {
    const std::size_t n = x_i_min.size(), m = x_j_min.size();
    if (x_i_max.size() != n || s1.size() != n || s2.size() != n || x_j_max.size() != m || t1.size() != m || t2.size() != m || data.size[0] != n ||
        data.size[1] != m)
        throw Error(TM_E_SIZE, "edge / clustering / block sizes do not agree (tfi.zig:125-133)");
    check(tm_tfi_block(&data.data[0].data[0], n, m, &x_i_min[0].data[0], &x_i_max[0].data[0], &x_j_min[0].data[0], &x_j_max[0].data[0], s1.data(),
                       s2.data(), t1.data(), t2.data()));
}
inline void linear2d(std::vector<types::Vec2d>& data, const std::vector<types::Vec2d>& e_i_min, const std::vector<types::Vec2d>& e_i_max,
                     const std::vector<types::Vec2d>& e_j_min, const std::vector<types::Vec2d>& e_j_max) {   // tfi.zig:19-67
    const std::size_t n = e_i_min.size(), m = e_j_min.size();
    if (e_i_max.size() != n || e_j_max.size() != m) throw Error(TM_E_SIZE, "error.InconsistentSize (tfi.zig:30)");
    data.resize(n * m);
    check(tm_tfi_linear2d(&data[0].data[0], n, m, &e_i_min[0].data[0], &e_i_max[0].data[0], &e_j_min[0].data[0], &e_j_max[0].data[0]));
}
}  // namespace tfi

namespace discrete {   // discrete.zig
struct Edge {          // :12-36
    std::vector<types::Vec2d> points;
    std::vector<double> clustering;
    static Edge init(types::Index n, const geometry::Line& curve, const clustering::Function& cl) {
        Edge e;
        e.clustering = clustering::create(cl, n);
        e.points = curve.interpolate(e.clustering);
        return e;
    }
};
struct EdgeView {      // :94-136
    const Edge* edge;
    std::size_t start, end;
    std::size_t len() const { return start > end ? start - end + 1 : end - start + 1; }
};
inline Edge combine(const std::vector<EdgeView>& edges) {   // Edge.combine, :38-91
    const double tol = 1e-10;
    for (std::size_t i = 0; i + 1 < edges.size(); ++i)
        if (!types::eqlApprox(edges[i].edge->points[edges[i].end], edges[i + 1].edge->points[edges[i + 1].start], tol))
            throw Error(TM_E_MISMATCH, "edges cannot be combined as end points do not match");
    std::size_t n = 0;
    for (const auto& e : edges) n += e.len();
    n -= edges.size() - 1;
    Edge out;
    out.points.resize(n);
    out.clustering.resize(n);
    std::size_t pos = 0;
    for (const auto& e : edges) {
        const std::size_t len = e.len();
        for (std::size_t k = 0; k < len; ++k) out.points[pos + k] = e.edge->points[e.start > e.end ? e.start - k : e.start + k];
        pos += len - 1;
    }
    pos = 0;
    double last_value = 0.0;
    for (const auto& e : edges) {
        const std::size_t first = e.start > e.end ? e.end : e.start, last = e.start > e.end ? e.start : e.end;
        out.clustering[pos] = last_value;
        const double base = e.edge->clustering[first];
        std::size_t k = 1;
        for (std::size_t i = first + 1; i <= last; ++i, ++k) out.clustering[pos + k] = last_value + (e.edge->clustering[i] - base);
        pos += k - 1;
        last_value = out.clustering[pos];
    }
    for (auto& v : out.clustering) v /= last_value;
    return out;
}
struct Block2d {       // :138-164
    types::Mat2d points;
    static Block2d init(const Edge& i_min, const Edge& i_max, const Edge& j_min, const Edge& j_max) {
        Block2d b{types::Mat2d::init(i_min.points.size(), j_min.points.size())};
        tfi::linear2dBoundaryBlendedControlFunction(b.points, i_min.points, i_max.points, j_min.points, j_max.points, i_min.clustering, i_max.clustering,
                                                    j_min.clustering, j_max.clustering);
        return b;
    }
};
struct Quality {       // mesh quality report (tm_hip.h "mesh quality"): one record per block and the total
    std::vector<tm_quality> per_block;
    tm_quality total{};
};
struct Mesh {          // :166-195
    std::vector<Block2d> blocks;
    std::vector<std::string> names;
    std::vector<boundary::Connection> connections;
    std::vector<boundary::Condition> boundary_conditions;
    void addBlock(const std::string& name, Block2d block) {
        blocks.push_back(std::move(block));
        names.push_back(name);
    }
    // folded / degenerate cells, scaled Jacobian, angles, aspect, growth, areas of the coordinates as they stand: evaluated on the
    // device (tm_mesh_quality) or, host = true, by the same definitions on the CPU (tm_mesh_quality_host)
    Quality quality(bool host = false);
};
}  // namespace discrete

namespace smoothing {
enum class Preconditioner { diagonal, ilu0 };   // preconditioner.zig
namespace solver {                              // solver.zig:10-27 + hip
enum class Tag : int32_t { gmres = 0, bicgstab = 1, umfpack = 2, petsc = 3, hip = 4 };
// inner strategies of the hip solver (TM_INNER_* of tm_hip.h); reference_gmres = the file's "gmres" as written: assembled system, GMRES(30) +
// ilu0 / diagonal, the reference's tolerances
enum Inner : int32_t { bicgstab = 0, relax = 1, mg_bicgstab = 2, auto_ = 3, gmres = 4, reference_gmres = 5 };
struct Option {
    Tag tag = Tag::hip;
    Preconditioner preconditioner = Preconditioner::diagonal;   // payload of gmres / bicgstab; with hip + reference_gmres: ilu0 -> TM_OPT_PRECOND_ILU0
    int32_t inner = TM_INNER_BICGSTAB;                          // payload of hip
    double rtol = 0, atol = 0, omega = 0;
    uint64_t max_inner = 0;
    uint32_t check_every = 0;
    bool single_sweep = false;
    bool refine = false;   // TM_OPT_REFINE: iterative refinement with a double-double residual (Picard modes; refused with relax, reference_gmres, rank hooks)
};
}  // namespace solver
namespace wall_control_function {               // wall_control_function.zig:10-20, 56-68
struct White { double ds_target; double theta_target = 1.5707963267948966; };
struct Algorithm {
    std::optional<White> white;   // nullopt = .laplace (or one of the two kinds below)
    // the two kinds the library adds for any topology (include/tm_hip.h): thomas_middlecoff = block-local field from the block's own edges,
    // evaluated on the device and frozen; prescribed = the caller's per-node field, one vector of ni*nj (P, Q) pairs per block, which
    // smooth::Smoother sets after create (smooth::mesh, the one-shot call, cannot take it)
    bool thomas_middlecoff_ = false;
    std::optional<std::vector<std::vector<types::Vec2d>>> prescribed_;
    static Algorithm laplace() { return Algorithm{}; }
    static Algorithm thomas_middlecoff() {
        Algorithm a;
        a.thomas_middlecoff_ = true;
        return a;
    }
    static Algorithm prescribed(std::vector<std::vector<types::Vec2d>> fields) {
        Algorithm a;
        a.prescribed_ = std::move(fields);
        return a;
    }
};
}  // namespace wall_control_function
namespace smooth {
namespace detail {
inline tm_range toRange(const boundary::Range& r) { return tm_range{r.block, static_cast<uint32_t>(r.side), 0, r.start, r.end}; }
inline void requirePlot3d(const std::string& filename) {   // discrete.zig:215 error.OutputFormatNotEnabled for what is not built in
    const auto dot = filename.rfind('.');
    const std::string ext = dot == std::string::npos ? "" : filename.substr(dot);
    if (ext != ".xyz" && ext != ".p3d" && ext != ".x") throw Error(TM_E_UNSUPPORTED, "OutputFormatNotEnabled: " + ext + " (PLOT3D .xyz / .p3d / .x is built in; .cgns needs the cgns library)");
}
inline void writeHeader(std::FILE* f, const discrete::Mesh& m) {   // int32 nblocks | (int32 ni, nj) per block
    const int32_t nb = static_cast<int32_t>(m.blocks.size());
    std::fwrite(&nb, 4, 1, f);
    for (const auto& b : m.blocks) {
        const int32_t sz[2] = {static_cast<int32_t>(b.points.size[0]), static_cast<int32_t>(b.points.size[1])};
        std::fwrite(sz, 4, 2, f);
    }
}
}
// POD description of a Mesh for the C ABI (the arrays live as long as this object)
struct Desc {
    std::vector<tm_block> blocks;
    std::vector<tm_connection> conns;
    std::vector<tm_condition> bcs;
    tm_mesh_desc desc{};
    explicit Desc(discrete::Mesh& mesh_data) {
        for (auto& b : mesh_data.blocks) blocks.push_back(tm_block{&b.points.data[0].data[0], b.points.size[0], b.points.size[1]});
        for (const auto& c : mesh_data.connections) {
            tm_connection tc{};
            tc.r[0] = detail::toRange(c.ranges[0]);
            tc.r[1] = detail::toRange(c.ranges[1]);
            tc.has_periodicity = c.periodicity ? 1 : 0;
            if (c.periodicity) {
                tc.periodicity[0] = c.periodicity->data[0];
                tc.periodicity[1] = c.periodicity->data[1];
            }
            conns.push_back(tc);
        }
        for (const auto& b : mesh_data.boundary_conditions) bcs.push_back(tm_condition{detail::toRange(b.range), static_cast<uint32_t>(b.kind), 0});
        desc = tm_mesh_desc{blocks.data(), blocks.size(), conns.data(), conns.size(), bcs.data(), bcs.size()};
    }
};
inline tm_solver_opt toOpt(const solver::Option& o) {
    return tm_solver_opt{static_cast<int32_t>(o.tag), o.inner, o.rtol, o.atol, o.max_inner, o.check_every, (o.single_sweep ? uint32_t{TM_OPT_SINGLE_SWEEP} : 0u) |
                             ((o.tag == solver::Tag::hip && o.inner == TM_INNER_REFERENCE_GMRES && o.preconditioner == Preconditioner::ilu0) ? uint32_t{TM_OPT_PRECOND_ILU0} : 0u) |
                             (o.refine ? uint32_t{TM_OPT_REFINE} : 0u),
                         o.omega};
}
inline tm_control_fn toControl(const wall_control_function::Algorithm& a) {
    if (a.white) return tm_control_fn{TM_CF_WHITE, 0, a.white->ds_target, a.white->theta_target};
    if (a.thomas_middlecoff_) return tm_control_fn{TM_CF_THOMAS_MIDDLECOFF, 0, 0.0, 0.0};
    if (a.prescribed_) return tm_control_fn{TM_CF_PRESCRIBED, 0, 0.0, 0.0};
    return tm_control_fn{TM_CF_LAPLACE, 0, 0.0, 0.0};
}

// smooth.zig:74-80: mutates mesh_data.blocks[b].points.data in place
inline tm_stats mesh(discrete::Mesh& mesh_data, std::size_t iterations, const solver::Option& solver_option,
                     const wall_control_function::Algorithm& control_function_algorithm) {
    Desc d(mesh_data);
    tm_solver_opt so = toOpt(solver_option);
    tm_control_fn cf = toControl(control_function_algorithm);
    tm_stats st{};
    check(tm_smooth_mesh(&d.desc, iterations, &so, &cf, &st));
    return st;
}

// b - A x of a caller's CSR system, both components, in double-double arithmetic rounded once to fp64 (tm_csr_residual)
inline void csrResidual(std::size_t n, const int32_t* Ap, const int32_t* Ai, const double* Ax_x, const double* Ax_y, const double* bx, const double* by,
                        const double* x, const double* y, double* rx, double* ry) {
    check(tm_csr_residual(n, Ap, Ai, Ax_x, Ax_y, bx, by, x, y, rx, ry));
}

// The same smoother with the mesh resident on the device between calls (tm_smoother_*): iterate a fixed count like the
// reference, or until the scaled nonlinear residual reaches a tolerance; write() = system.write (smooth.zig:396-414).
class Smoother {
   public:
    // hooks: the transport of a multi-process run (one process per GPU), e.g. filled by tm_rccl_hooks; nullptr = all blocks here
    Smoother(discrete::Mesh& mesh_data, const solver::Option& o, const wall_control_function::Algorithm& a, const tm_comm_hooks* hooks = nullptr)
        : mesh_(mesh_data), d_(mesh_data) {
        tm_solver_opt so = toOpt(o);
        tm_control_fn cf = toControl(a);
        check(tm_smoother_create(&d_.desc, &so, &cf, hooks, nullptr, &h_));
        if (a.prescribed_) {
            try {
                std::vector<types::Vec2d> flat;
                for (const auto& f : *a.prescribed_) flat.insert(flat.end(), f.begin(), f.end());
                if (flat.size() != tm_smoother_dof(h_)) throw Error(TM_E_SIZE, "prescribed control function: one (P, Q) pair per node of every block");
                setControlFunction(flat);
            } catch (...) {
                tm_smoother_destroy(h_);
                throw;
            }
        }
    }
    // the resident (P, Q) field, one pair per owned node in block order; set: prescribed and Thomas-Middlecoff handles; update: evaluate the
    // Thomas-Middlecoff field again from the coordinates resident now
    std::vector<types::Vec2d> controlFunction() {
        std::vector<types::Vec2d> pq(tm_smoother_dof(h_));
        check(tm_smoother_control_function(h_, &pq[0].data[0]));
        return pq;
    }
    void setControlFunction(const std::vector<types::Vec2d>& pq) { check(tm_smoother_set_control_function(h_, &pq[0].data[0])); }
    void updateControlFunction() { check(tm_smoother_update_control_function(h_)); }
    const tm_mesh_desc& desc() const { return d_.desc; }
    tm_smoother* handle() const { return h_; }   // for the calls that take a list of handles (stack::stack_block)
    ~Smoother() { tm_smoother_destroy(h_); }
    Smoother(const Smoother&) = delete;
    Smoother& operator=(const Smoother&) = delete;
    tm_stats iterate(std::size_t iterations) {
        tm_stats st{};
        check(tm_smoother_iterate(h_, iterations, &st));
        return st;
    }
    bool iterateUntil(double scaled_residual_tol, std::size_t max_iterations, tm_stats* stats = nullptr) {
        tm_stats st{};
        const int rc = tm_smoother_iterate_until(h_, max_iterations, scaled_residual_tol, &st);
        check(rc);
        if (stats) *stats = st;
        return rc == TM_OK;
    }
    void download() { check(tm_smoother_download(h_, &d_.desc)); }
    // b - A(X) xy against the system assembled from the resident coordinates, in double-double arithmetic rounded once to fp64
    // (tm_smoother_residual); xy = nullptr: the resident coordinates themselves.  2 * dof doubles each, global row order
    void residual(const double* xy, double* r_xy) { check(tm_smoother_residual(h_, xy, r_xy)); }
    // what the refinement of a handle created with Option::refine did (tm_smoother_refine_report)
    struct RefineReport {
        uint32_t steps[2];
        double last_update_rel[2];
        uint64_t correction_iterations;
    };
    RefineReport refineReport() const {
        RefineReport r{};
        check(tm_smoother_refine_report(h_, r.steps, r.last_update_rel, &r.correction_iterations));
        return r;
    }
    // quality report of the coordinates resident in the handle (reads them only)
    discrete::Quality quality() {
        discrete::Quality q;
        q.per_block.resize(mesh_.blocks.size());
        check(tm_smoother_quality(h_, q.per_block.data(), &q.total));
        return q;
    }
    // multi-block PLOT3D grid file (planes transposed on the device); `.cgns` needs the cgns library like the reference
    void write(const std::string& filename) {
        detail::requirePlot3d(filename);
        std::FILE* f = std::fopen(filename.c_str(), "wb");
        if (!f) throw Error(TM_E_ARG, "cannot open " + filename);
        detail::writeHeader(f, mesh_);
        std::vector<double> x, y;
        for (std::size_t b = 0; b < mesh_.blocks.size(); ++b) {
            const std::size_t n = mesh_.blocks[b].points.size[0] * mesh_.blocks[b].points.size[1];
            x.resize(n);
            y.resize(n);
            check(tm_smoother_export_soa(h_, b, x.data(), y.data(), nullptr, nullptr));
            std::fwrite(x.data(), sizeof(double), n, f);
            std::fwrite(y.data(), sizeof(double), n, f);
        }
        std::fclose(f);
    }

   private:
    discrete::Mesh& mesh_;
    Desc d_;
    tm_smoother* h_ = nullptr;
};
}  // namespace smooth
}  // namespace smoothing

// 3-D from 2-D cuts (tm_hip.h): layer k of a 3-D block = sum_c A[k][c] * cut c, weights from the span positions alone
namespace stack {
struct Option {
    std::vector<double> span;     // z of every cut, strictly increasing (the radius with the cylindrical mapping)
    std::vector<double> layers;   // s of every layer, inside [z_0, z_{K-1}]
    int32_t interpolation = TM_STACK_CUBIC;
    int32_t mapping = TM_STACK_PLANAR;
    tm_stack_opt c_struct() const { return tm_stack_opt{span.size(), span.data(), layers.size(), layers.data(), interpolation, mapping}; }
};
struct Block3d {                  // planes in PLOT3D order: element (k*nj + j)*ni + i
    std::size_t ni = 0, nj = 0, nk = 0;
    std::vector<double> x, y, z;
};
inline std::vector<double> weights(const Option& o) {
    std::vector<double> w(o.span.size() * o.layers.size() + 1);
    const tm_stack_opt so = o.c_struct();
    check(tm_stack_weights(&so, w.data()));
    w.resize(o.span.size() * o.layers.size());
    return w;
}
// layers [k_begin, k_begin + k_count) of `block` from the coordinates RESIDENT in one handle per cut (tm_stack_smoothers)
inline Block3d stack_block(const std::vector<smoothing::smooth::Smoother*>& cuts, const Option& o, std::size_t block, std::size_t k_begin, std::size_t k_count) {
    if (cuts.empty() || cuts.size() != o.span.size()) throw Error(TM_E_ARG, "one handle per span position");
    std::vector<tm_smoother*> h;
    for (const auto* c : cuts) h.push_back(c ? c->handle() : nullptr);
    const tm_mesh_desc& d = cuts[0]->desc();
    if (block >= d.nblocks) throw Error(TM_E_ARG, "block index past the mesh");
    Block3d b;
    b.ni = d.blocks[block].ni, b.nj = d.blocks[block].nj, b.nk = k_count;
    const std::size_t n = b.ni * b.nj * k_count;
    b.x.resize(n + 1), b.y.resize(n + 1), b.z.resize(n + 1);
    const tm_stack_opt so = o.c_struct();
    check(tm_stack_smoothers(h.data(), &so, block, k_begin, k_count, b.x.data(), b.y.data(), b.z.data()));
    b.x.resize(n), b.y.resize(n), b.z.resize(n);
    return b;
}
// the same from host coordinates, uploaded per call (tm_stack_block) or, host = true, evaluated on the CPU (tm_stack_block_host)
inline Block3d stack_block(const std::vector<discrete::Mesh*>& cuts, const Option& o, std::size_t block, std::size_t k_begin, std::size_t k_count, bool host = false) {
    if (cuts.empty() || cuts.size() != o.span.size()) throw Error(TM_E_ARG, "one mesh per span position");
    std::vector<std::unique_ptr<smoothing::smooth::Desc>> descs;
    std::vector<const tm_mesh_desc*> d;
    for (auto* m : cuts) {
        if (!m) throw Error(TM_E_ARG, "null mesh");
        descs.push_back(std::make_unique<smoothing::smooth::Desc>(*m));
        d.push_back(&descs.back()->desc);
    }
    if (block >= cuts[0]->blocks.size()) throw Error(TM_E_ARG, "block index past the mesh");
    Block3d b;
    b.ni = cuts[0]->blocks[block].points.size[0], b.nj = cuts[0]->blocks[block].points.size[1], b.nk = k_count;
    const std::size_t n = b.ni * b.nj * k_count;
    b.x.resize(n + 1), b.y.resize(n + 1), b.z.resize(n + 1);
    const tm_stack_opt so = o.c_struct();
    check((host ? tm_stack_block_host : tm_stack_block)(d.data(), &so, block, k_begin, k_count, b.x.data(), b.y.data(), b.z.data()));
    b.x.resize(n), b.y.resize(n), b.z.resize(n);
    return b;
}
// cuts on stream surfaces of revolution (tm_hip.h): one meridional table x(u), r(u) per cut, for Option::mapping == TM_STACK_REVOLUTION
struct Surfaces {
    std::vector<std::vector<double>> u, x, r;   // per cut: knots (strictly increasing), axial position, radius (> 0); 2 .. 256 entries
    std::vector<double> rref;                   // per cut, or empty: the span coordinates
    int32_t interpolation = TM_SURF_CUBIC;
    struct CStruct {                            // tm_stack_surfaces and the pointer lists it points into
        std::vector<uint64_t> nknots;
        std::vector<const double*> u, x, r;
        tm_stack_surfaces s{};
    };
    std::unique_ptr<CStruct> c_struct() const {
        if (u.size() != x.size() || u.size() != r.size()) throw Error(TM_E_ARG, "u, x, r: one table per cut each");
        auto c = std::make_unique<CStruct>();
        for (std::size_t k = 0; k < u.size(); ++k) {
            if (u[k].size() != x[k].size() || u[k].size() != r[k].size()) throw Error(TM_E_ARG, "the u, x and r columns of a cut differ in length");
            c->nknots.push_back(u[k].size());
            c->u.push_back(u[k].data()), c->x.push_back(x[k].data()), c->r.push_back(r[k].data());
        }
        if (!rref.empty() && rref.size() != u.size()) throw Error(TM_E_ARG, "one reference radius per cut");
        c->s = tm_stack_surfaces{u.size(), c->nknots.data(), c->u.data(), c->x.data(), c->r.data(), rref.empty() ? nullptr : rref.data(), interpolation, 0};
        return c;
    }
};
// per interval ax bx cx dx ar br cr dr, cut after cut (tm_stack_surface_tables: host only)
inline std::vector<double> surface_tables(const Option& o, const Surfaces& sf) {
    std::size_t n = 0;
    for (const auto& k : sf.u) n += k.empty() ? 0 : 8 * (k.size() - 1);
    std::vector<double> coef(n + 1);
    const tm_stack_opt so = o.c_struct();
    const auto cs = sf.c_struct();
    check(tm_stack_surface_tables(&so, &cs->s, coef.data()));
    coef.resize(n);
    return coef;
}
// stack_block on the surfaces (tm_stack_smoothers_surf); outside, when given, receives per cut the number of extrapolated nodes
inline Block3d stack_block(const std::vector<smoothing::smooth::Smoother*>& cuts, const Option& o, const Surfaces& sf, std::size_t block, std::size_t k_begin,
                           std::size_t k_count, std::vector<uint64_t>* outside = nullptr) {
    if (cuts.empty() || cuts.size() != o.span.size()) throw Error(TM_E_ARG, "one handle per span position");
    std::vector<tm_smoother*> h;
    for (const auto* c : cuts) h.push_back(c ? c->handle() : nullptr);
    const tm_mesh_desc& d = cuts[0]->desc();
    if (block >= d.nblocks) throw Error(TM_E_ARG, "block index past the mesh");
    Block3d b;
    b.ni = d.blocks[block].ni, b.nj = d.blocks[block].nj, b.nk = k_count;
    const std::size_t n = b.ni * b.nj * k_count;
    b.x.resize(n + 1), b.y.resize(n + 1), b.z.resize(n + 1);
    const tm_stack_opt so = o.c_struct();
    const auto cs = sf.c_struct();
    if (outside) outside->assign(cuts.size(), 0);
    check(tm_stack_smoothers_surf(h.data(), &so, &cs->s, block, k_begin, k_count, b.x.data(), b.y.data(), b.z.data(), outside ? outside->data() : nullptr));
    b.x.resize(n), b.y.resize(n), b.z.resize(n);
    return b;
}
// the same from host coordinates (tm_stack_block_surf; host = true: tm_stack_block_surf_host)
inline Block3d stack_block(const std::vector<discrete::Mesh*>& cuts, const Option& o, const Surfaces& sf, std::size_t block, std::size_t k_begin, std::size_t k_count,
                           bool host = false, std::vector<uint64_t>* outside = nullptr) {
    if (cuts.empty() || cuts.size() != o.span.size()) throw Error(TM_E_ARG, "one mesh per span position");
    std::vector<std::unique_ptr<smoothing::smooth::Desc>> descs;
    std::vector<const tm_mesh_desc*> d;
    for (auto* m : cuts) {
        if (!m) throw Error(TM_E_ARG, "null mesh");
        descs.push_back(std::make_unique<smoothing::smooth::Desc>(*m));
        d.push_back(&descs.back()->desc);
    }
    if (block >= cuts[0]->blocks.size()) throw Error(TM_E_ARG, "block index past the mesh");
    Block3d b;
    b.ni = cuts[0]->blocks[block].points.size[0], b.nj = cuts[0]->blocks[block].points.size[1], b.nk = k_count;
    const std::size_t n = b.ni * b.nj * k_count;
    b.x.resize(n + 1), b.y.resize(n + 1), b.z.resize(n + 1);
    const tm_stack_opt so = o.c_struct();
    const auto cs = sf.c_struct();
    if (outside) outside->assign(cuts.size(), 0);
    check((host ? tm_stack_block_surf_host : tm_stack_block_surf)(d.data(), &so, &cs->s, block, k_begin, k_count, b.x.data(), b.y.data(), b.z.data(),
                                                                  outside ? outside->data() : nullptr));
    b.x.resize(n), b.y.resize(n), b.z.resize(n);
    return b;
}
// 3-D quality of the blocks stacked on their surfaces, from the resident coordinates (tm_stack_smoothers_quality_surf)
inline tm_quality3d quality(const std::vector<smoothing::smooth::Smoother*>& cuts, const Option& o, const Surfaces& sf, std::size_t block) {
    if (cuts.empty() || cuts.size() != o.span.size()) throw Error(TM_E_ARG, "one handle per span position");
    std::vector<tm_smoother*> h;
    for (const auto* c : cuts) h.push_back(c ? c->handle() : nullptr);
    const tm_stack_opt so = o.c_struct();
    const auto cs = sf.c_struct();
    tm_quality3d q;
    check(tm_stack_smoothers_quality_surf(h.data(), &so, &cs->s, block, &q));
    return q;
}
// 3-D quality of stacked blocks (tm_hip.h): the hexahedra of `block` of the stack, evaluated on the device straight from the coordinates
// RESIDENT in one handle per cut (tm_stack_smoothers_quality: the 3-D block is never stored)
inline tm_quality3d quality(const std::vector<smoothing::smooth::Smoother*>& cuts, const Option& o, std::size_t block) {
    if (cuts.empty() || cuts.size() != o.span.size()) throw Error(TM_E_ARG, "one handle per span position");
    std::vector<tm_smoother*> h;
    for (const auto* c : cuts) h.push_back(c ? c->handle() : nullptr);
    const tm_stack_opt so = o.c_struct();
    tm_quality3d q;
    check(tm_stack_smoothers_quality(h.data(), &so, block, &q));
    return q;
}
// the same of any 3-D block held on the host, evaluated on the CPU (tm_quality3d_planes_host)
inline tm_quality3d quality(const Block3d& b, std::size_t block = 0) {
    tm_quality3d q;
    check(tm_quality3d_planes_host(b.x.data(), b.y.data(), b.z.data(), b.ni, b.nj, b.nk, block, &q, nullptr));
    return q;
}
// elliptic smoothing of stacked blocks (tm_hip.h, kernel K22): Jacobi sweeps of the 3-D Winslow equations with the six faces held
struct Smooth {
    int32_t algorithm = TM_S3_THOMAS_MIDDLECOFF;
    uint64_t sweeps = 0;
    double omega = 1.0, tol = 0.0;
    const double *f1 = nullptr, *f2 = nullptr, *f3 = nullptr;   // TM_S3_PRESCRIBED
    tm_smooth3d_opt c_struct() const { return tm_smooth3d_opt{algorithm, 0, sweeps, omega, tol, f1, f2, f3}; }
};
// a block held on the host, in place (tm_smooth3d_planes; host = true: tm_smooth3d_planes_host, no GPU)
inline tm_smooth3d_info smooth(Block3d& b, const Smooth& s, bool host = false) {
    const tm_smooth3d_opt so = s.c_struct();
    tm_smooth3d_info info;
    check((host ? tm_smooth3d_planes_host : tm_smooth3d_planes)(b.ni, b.nj, b.nk, b.x.data(), b.y.data(), b.z.data(), &so, &info));
    return info;
}
// all layers of `block` stacked from the coordinates RESIDENT in one handle per cut and smoothed on the device (tm_stack_smoothers_smooth):
// only the planes and the record cross to the host, no handle is modified
inline Block3d smooth(const std::vector<smoothing::smooth::Smoother*>& cuts, const Option& o, std::size_t block, const Smooth& s, tm_smooth3d_info* info = nullptr) {
    if (cuts.empty() || cuts.size() != o.span.size()) throw Error(TM_E_ARG, "one handle per span position");
    std::vector<tm_smoother*> h;
    for (const auto* c : cuts) h.push_back(c ? c->handle() : nullptr);
    const tm_mesh_desc& d = cuts[0]->desc();
    if (block >= d.nblocks) throw Error(TM_E_ARG, "block index past the mesh");
    Block3d b;
    b.ni = d.blocks[block].ni, b.nj = d.blocks[block].nj, b.nk = o.layers.size();
    const std::size_t n = b.ni * b.nj * b.nk;
    b.x.resize(n + 1), b.y.resize(n + 1), b.z.resize(n + 1);
    const tm_stack_opt so = o.c_struct();
    const tm_smooth3d_opt ss = s.c_struct();
    tm_smooth3d_info rec;
    check(tm_stack_smoothers_smooth(h.data(), &so, block, &ss, b.x.data(), b.y.data(), b.z.data(), &rec));
    b.x.resize(n), b.y.resize(n), b.z.resize(n);
    if (info) *info = rec;
    return b;
}
}  // namespace stack

// high-order elements (tm_hip.h): every p x p group of cells of a block is one curved element of order p; its nodes at the wanted
// distribution and its Jacobian come from the element's degree-p tensor-product interpolant
namespace highorder {
struct Option {
    int32_t order = 2;
    int32_t distribution = TM_HO_GAUSS_LOBATTO;
    std::vector<double> nodes;    // TM_HO_PRESCRIBED: order + 1 values, 0 first, 1 last, strictly increasing
    tm_ho_opt c_struct() const { return tm_ho_opt{order, distribution, nodes.empty() ? nullptr : nodes.data()}; }
};
struct Elevated {                 // planes with i fastest: element j*ni + i; sj[f*Ei + e], NaN for invalid elements
    std::size_t ni = 0, nj = 0, Ei = 0, Ej = 0;
    std::vector<double> x, y, sj;
    tm_ho_quality quality{};
};
namespace detail {
inline Elevated sized(std::size_t ni, std::size_t nj, const Option& o) {
    if (o.order < 1 || o.order > TM_HO_MAX_ORDER) throw Error(TM_E_ARG, "the order must be 1 .. TM_HO_MAX_ORDER");
    Elevated r;
    r.ni = ni, r.nj = nj, r.Ei = (ni - 1) / static_cast<std::size_t>(o.order), r.Ej = (nj - 1) / static_cast<std::size_t>(o.order);
    r.x.resize(ni * nj + 1), r.y.resize(ni * nj + 1), r.sj.resize(r.Ei * r.Ej + 1);
    return r;
}
inline void trim(Elevated& r) { r.x.resize(r.ni * r.nj), r.y.resize(r.ni * r.nj), r.sj.resize(r.Ei * r.Ej); }
}  // namespace detail
inline void check(discrete::Mesh& mesh, const Option& o) {
    smoothing::smooth::Desc d(mesh);
    const tm_ho_opt ho = o.c_struct();
    core::check(tm_ho_check(&d.desc, &ho));
}
// `block` from the coordinates RESIDENT in the handle (tm_smoother_elevate, kernel K13)
inline Elevated elevate(const smoothing::smooth::Smoother& s, const Option& o, std::size_t block) {
    const tm_mesh_desc& d = s.desc();
    if (block >= d.nblocks) throw Error(TM_E_ARG, "block index past the mesh");
    Elevated r = detail::sized(d.blocks[block].ni, d.blocks[block].nj, o);
    const tm_ho_opt ho = o.c_struct();
    core::check(tm_smoother_elevate(s.handle(), &ho, block, r.x.data(), r.y.data(), &r.quality, r.sj.data()));
    detail::trim(r);
    return r;
}
// the same from host coordinates, uploaded per call (tm_ho_elevate) or, host = true, evaluated on the CPU (tm_ho_elevate_host)
inline Elevated elevate(discrete::Mesh& mesh, const Option& o, std::size_t block, bool host = false) {
    if (block >= mesh.blocks.size()) throw Error(TM_E_ARG, "block index past the mesh");
    smoothing::smooth::Desc d(mesh);
    Elevated r = detail::sized(mesh.blocks[block].points.size[0], mesh.blocks[block].points.size[1], o);
    const tm_ho_opt ho = o.c_struct();
    core::check((host ? tm_ho_elevate_host : tm_ho_elevate)(&d.desc, &ho, block, r.x.data(), r.y.data(), &r.quality, r.sj.data()));
    detail::trim(r);
    return r;
}
// The certificate of `block`: every element judged on its whole area by the Bernstein coefficients of its Jacobian (tm_hip.h,
// "high-order elements: certificate").  status[f*Ei + e] is TM_HO_PROVEN / TM_HO_INVALID / TM_HO_UNDECIDED, bounds[2*(f*Ei + e)] = (lo, hi)
struct Certified {
    std::size_t Ei = 0, Ej = 0;
    std::vector<uint8_t> status;
    std::vector<double> bounds;
    tm_ho_certificate certificate{};
};
namespace detail {
inline Certified certified(std::size_t ni, std::size_t nj, const Option& o) {
    if (o.order < 1 || o.order > TM_HO_MAX_ORDER) throw Error(TM_E_ARG, "the order must be 1 .. TM_HO_MAX_ORDER");
    Certified r;
    r.Ei = (ni - 1) / static_cast<std::size_t>(o.order), r.Ej = (nj - 1) / static_cast<std::size_t>(o.order);
    r.status.resize(r.Ei * r.Ej + 1), r.bounds.resize(2 * r.Ei * r.Ej + 2);
    return r;
}
inline void trim(Certified& r) { r.status.resize(r.Ei * r.Ej), r.bounds.resize(2 * r.Ei * r.Ej); }
}  // namespace detail
// from the coordinates RESIDENT in the handle (tm_smoother_certify: K13's report, then kernel K14)
inline Certified certify(const smoothing::smooth::Smoother& s, const Option& o, std::size_t block, int max_depth = 3) {
    const tm_mesh_desc& d = s.desc();
    if (block >= d.nblocks) throw Error(TM_E_ARG, "block index past the mesh");
    Certified r = detail::certified(d.blocks[block].ni, d.blocks[block].nj, o);
    const tm_ho_opt ho = o.c_struct();
    core::check(tm_smoother_certify(s.handle(), &ho, max_depth, block, &r.certificate, r.status.data(), r.bounds.data()));
    detail::trim(r);
    return r;
}
// the same from host coordinates, uploaded per call (tm_ho_certify) or, host = true, evaluated on the CPU (tm_ho_certify_host)
inline Certified certify(discrete::Mesh& mesh, const Option& o, std::size_t block, int max_depth = 3, bool host = false) {
    if (block >= mesh.blocks.size()) throw Error(TM_E_ARG, "block index past the mesh");
    smoothing::smooth::Desc d(mesh);
    Certified r = detail::certified(mesh.blocks[block].points.size[0], mesh.blocks[block].points.size[1], o);
    const tm_ho_opt ho = o.c_struct();
    core::check((host ? tm_ho_certify_host : tm_ho_certify)(&d.desc, &ho, max_depth, block, &r.certificate, r.status.data(), r.bounds.data()));
    detail::trim(r);
    return r;
}
}  // namespace highorder

// high-order hexahedra of stacked blocks (tm_hip.h): the layers of a stacked block agglomerated into curved hexahedra of order p <= 4
namespace stack {
struct Elevated3d {               // planes in PLOT3D order: element (k*nj + j)*ni + i, nk = g_count*p + 1; sj[(g*Ej + f)*Ei + e] of the WHOLE block
    std::size_t ni = 0, nj = 0, nk = 0, Ei = 0, Ej = 0, Eg = 0;
    std::vector<double> x, y, z, sj;
    tm_ho3_quality quality{};
};
namespace detail {
inline Elevated3d sized(std::size_t ni, std::size_t nj, const Option& o, const highorder::Option& ho, std::size_t g_count) {
    if (ho.order < 1 || ho.order > TM_HO3_MAX_ORDER) throw Error(TM_E_ARG, "the order must be 1 .. TM_HO3_MAX_ORDER");
    const std::size_t p = static_cast<std::size_t>(ho.order);
    Elevated3d r;
    r.ni = ni, r.nj = nj, r.nk = g_count * p + 1, r.Ei = (ni - 1) / p, r.Ej = (nj - 1) / p, r.Eg = o.layers.empty() ? 0 : (o.layers.size() - 1) / p;
    const std::size_t n = ni * nj * r.nk;
    r.x.resize(n + 1), r.y.resize(n + 1), r.z.resize(n + 1), r.sj.resize(r.Ei * r.Ej * r.Eg + 1);
    return r;
}
inline void trim(Elevated3d& r) {
    const std::size_t n = r.ni * r.nj * r.nk;
    r.x.resize(n), r.y.resize(n), r.z.resize(n), r.sj.resize(r.Ei * r.Ej * r.Eg);
}
}  // namespace detail
// the span elements [g_begin, g_begin + g_count) of `block` from the coordinates RESIDENT in one handle per cut (tm_stack_smoothers_elevate,
// kernel K16: the fine 3-D block is never stored); sf: the meridional tables of TM_STACK_REVOLUTION, else null
inline Elevated3d elevate(const std::vector<smoothing::smooth::Smoother*>& cuts, const Option& o, const highorder::Option& ho, std::size_t block, std::size_t g_begin,
                          std::size_t g_count, const Surfaces* sf = nullptr, std::vector<uint64_t>* outside = nullptr) {
    if (cuts.empty() || cuts.size() != o.span.size()) throw Error(TM_E_ARG, "one handle per span position");
    std::vector<tm_smoother*> h;
    for (const auto* c : cuts) h.push_back(c ? c->handle() : nullptr);
    const tm_mesh_desc& d = cuts[0]->desc();
    if (block >= d.nblocks) throw Error(TM_E_ARG, "block index past the mesh");
    Elevated3d r = detail::sized(d.blocks[block].ni, d.blocks[block].nj, o, ho, g_count);
    const tm_stack_opt so = o.c_struct();
    const tm_ho_opt hopt = ho.c_struct();
    const auto cs = sf ? sf->c_struct() : nullptr;
    if (outside) outside->assign(cuts.size(), 0);
    check(tm_stack_smoothers_elevate(h.data(), &so, cs ? &cs->s : nullptr, &hopt, block, g_begin, g_count, r.x.data(), r.y.data(), r.z.data(), &r.quality, r.sj.data(),
                                     outside ? outside->data() : nullptr));
    detail::trim(r);
    return r;
}
// the same from host coordinates, uploaded per call (tm_stack_elevate) or, host = true, evaluated on the CPU (tm_stack_elevate_host)
inline Elevated3d elevate(const std::vector<discrete::Mesh*>& cuts, const Option& o, const highorder::Option& ho, std::size_t block, std::size_t g_begin,
                          std::size_t g_count, bool host = false, const Surfaces* sf = nullptr, std::vector<uint64_t>* outside = nullptr) {
    if (cuts.empty() || cuts.size() != o.span.size()) throw Error(TM_E_ARG, "one mesh per span position");
    std::vector<std::unique_ptr<smoothing::smooth::Desc>> descs;
    std::vector<const tm_mesh_desc*> d;
    for (auto* m : cuts) {
        if (!m) throw Error(TM_E_ARG, "null mesh");
        descs.push_back(std::make_unique<smoothing::smooth::Desc>(*m));
        d.push_back(&descs.back()->desc);
    }
    if (block >= cuts[0]->blocks.size()) throw Error(TM_E_ARG, "block index past the mesh");
    Elevated3d r = detail::sized(cuts[0]->blocks[block].points.size[0], cuts[0]->blocks[block].points.size[1], o, ho, g_count);
    const tm_stack_opt so = o.c_struct();
    const tm_ho_opt hopt = ho.c_struct();
    const auto cs = sf ? sf->c_struct() : nullptr;
    if (outside) outside->assign(cuts.size(), 0);
    check((host ? tm_stack_elevate_host : tm_stack_elevate)(d.data(), &so, cs ? &cs->s : nullptr, &hopt, block, g_begin, g_count, r.x.data(), r.y.data(), r.z.data(),
                                                            &r.quality, r.sj.data(), outside ? outside->data() : nullptr));
    detail::trim(r);
    return r;
}
// the certificate of the curved hexahedra of `block` (tm_hip.h, "high-order hexahedra: certificate"; kernel K17): status[(g*Ej + f)*Ei + e],
// bounds (lo, hi) per element in the same order
struct Certified3d {
    std::size_t Ei = 0, Ej = 0, Eg = 0;
    std::vector<uint8_t> status;
    std::vector<double> bounds;
    tm_ho3_certificate certificate{};
};
namespace detail {
inline Certified3d certified(std::size_t ni, std::size_t nj, const Option& o, const highorder::Option& ho) {
    if (ho.order < 1 || ho.order > TM_HO3_MAX_ORDER) throw Error(TM_E_ARG, "the order must be 1 .. TM_HO3_MAX_ORDER");
    const std::size_t p = static_cast<std::size_t>(ho.order);
    Certified3d r;
    r.Ei = (ni - 1) / p, r.Ej = (nj - 1) / p, r.Eg = o.layers.empty() ? 0 : (o.layers.size() - 1) / p;
    r.status.resize(r.Ei * r.Ej * r.Eg + 1), r.bounds.resize(2 * r.Ei * r.Ej * r.Eg + 2);
    return r;
}
inline void trim(Certified3d& r) { r.status.resize(r.Ei * r.Ej * r.Eg), r.bounds.resize(2 * r.Ei * r.Ej * r.Eg); }
}  // namespace detail
// from the coordinates RESIDENT in one handle per cut (tm_stack_smoothers_certify)
inline Certified3d certify(const std::vector<smoothing::smooth::Smoother*>& cuts, const Option& o, const highorder::Option& ho, std::size_t block, int max_depth = 2,
                           const Surfaces* sf = nullptr, std::vector<uint64_t>* outside = nullptr) {
    if (cuts.empty() || cuts.size() != o.span.size()) throw Error(TM_E_ARG, "one handle per span position");
    std::vector<tm_smoother*> h;
    for (const auto* c : cuts) h.push_back(c ? c->handle() : nullptr);
    const tm_mesh_desc& d = cuts[0]->desc();
    if (block >= d.nblocks) throw Error(TM_E_ARG, "block index past the mesh");
    Certified3d r = detail::certified(d.blocks[block].ni, d.blocks[block].nj, o, ho);
    const tm_stack_opt so = o.c_struct();
    const tm_ho_opt hopt = ho.c_struct();
    const auto cs = sf ? sf->c_struct() : nullptr;
    if (outside) outside->assign(cuts.size(), 0);
    check(tm_stack_smoothers_certify(h.data(), &so, cs ? &cs->s : nullptr, &hopt, max_depth, block, &r.certificate, r.status.data(), r.bounds.data(),
                                     outside ? outside->data() : nullptr));
    detail::trim(r);
    return r;
}
// the same from host coordinates, uploaded per call (tm_stack_certify) or, host = true, evaluated on the CPU (tm_stack_certify_host)
inline Certified3d certify(const std::vector<discrete::Mesh*>& cuts, const Option& o, const highorder::Option& ho, std::size_t block, int max_depth = 2,
                           bool host = false, const Surfaces* sf = nullptr, std::vector<uint64_t>* outside = nullptr) {
    if (cuts.empty() || cuts.size() != o.span.size()) throw Error(TM_E_ARG, "one mesh per span position");
    std::vector<std::unique_ptr<smoothing::smooth::Desc>> descs;
    std::vector<const tm_mesh_desc*> d;
    for (auto* m : cuts) {
        if (!m) throw Error(TM_E_ARG, "null mesh");
        descs.push_back(std::make_unique<smoothing::smooth::Desc>(*m));
        d.push_back(&descs.back()->desc);
    }
    if (block >= cuts[0]->blocks.size()) throw Error(TM_E_ARG, "block index past the mesh");
    Certified3d r = detail::certified(cuts[0]->blocks[block].points.size[0], cuts[0]->blocks[block].points.size[1], o, ho);
    const tm_stack_opt so = o.c_struct();
    const tm_ho_opt hopt = ho.c_struct();
    const auto cs = sf ? sf->c_struct() : nullptr;
    if (outside) outside->assign(cuts.size(), 0);
    check((host ? tm_stack_certify_host : tm_stack_certify)(d.data(), &so, cs ? &cs->s : nullptr, &hopt, max_depth, block, &r.certificate, r.status.data(),
                                                            r.bounds.data(), outside ? outside->data() : nullptr));
    detail::trim(r);
    return r;
}
}  // namespace stack

// welded unstructured mesh (tm_hip.h, kernel K18): one node numbering across the connections of a mesh, welded points and cells
namespace weld {
struct Map {
    std::vector<int32_t> map;     // welded id per node, plane order (block after block, j*ni + i)
    tm_weld_info info{};
};
struct Points {                   // nodes_out values per component
    std::vector<double> x, y;
    tm_weld_info info{};
};
inline Map map(discrete::Mesh& mesh, bool host = false) {
    smoothing::smooth::Desc d(mesh);
    Map r;
    std::size_t n = 0;
    for (const auto& b : mesh.blocks) n += b.points.size[0] * b.points.size[1];
    r.map.resize(n + 1);
    core::check((host ? tm_weld_map_host : tm_weld_map)(&d.desc, r.map.data(), &r.info));
    r.map.resize(n);
    return r;
}
// from the coordinates RESIDENT in the handle (tm_smoother_weld): the interleaved blocks are read in place
inline Points points(const smoothing::smooth::Smoother& s, Map* map_out = nullptr) {
    const tm_mesh_desc& d = s.desc();
    std::size_t n = 0;
    for (uint64_t b = 0; b < d.nblocks; ++b) n += d.blocks[b].ni * d.blocks[b].nj;
    Points r;
    r.x.resize(n + 1), r.y.resize(n + 1);
    if (map_out) map_out->map.resize(n + 1);
    core::check(tm_smoother_weld(s.handle(), map_out ? map_out->map.data() : nullptr, r.x.data(), r.y.data(), &r.info));
    r.x.resize(r.info.nodes_out), r.y.resize(r.info.nodes_out);
    if (map_out) map_out->map.resize(n), map_out->info = r.info;
    return r;
}
// quadrilaterals of `order` (nk <= 1) or hexahedra across nk layers: (order+1)^2 or (order+1)^3 ids per element, VTK's Lagrange order
inline std::vector<int32_t> cells(discrete::Mesh& mesh, const Map& m, int order = 1, std::size_t nk = 0, bool host = false) {
    if (order < 1 || order > TM_HO_MAX_ORDER) throw Error(TM_E_ARG, "the order must be 1 .. TM_HO_MAX_ORDER");
    smoothing::smooth::Desc d(mesh);
    const std::size_t p = static_cast<std::size_t>(order), Eg = nk >= 2 ? (nk - 1) / p : 1, npe = nk >= 2 ? (p + 1) * (p + 1) * (p + 1) : (p + 1) * (p + 1);
    std::size_t n = 0;
    for (const auto& b : mesh.blocks) n += ((b.points.size[0] - 1) / p) * ((b.points.size[1] - 1) / p) * Eg;
    std::vector<int32_t> c(n * npe + 1);
    core::check((host ? tm_weld_cells_host : tm_weld_cells)(&d.desc, m.map.data(), m.info.nodes_out, order, nk, c.data()));
    c.resize(n * npe);
    return c;
}
// boundary of the welded mesh (tm_hip.h, kernel K19): the faces over the welded ids in patches, and the sums per patch
struct Boundary {
    tm_weld_boundary_info info{};
    std::vector<tm_weld_patch> patches;      // kind, source, partner, translation, the CSR; measure / normal / moment once measured
    std::vector<int32_t> faces, face_patch;  // info.faces * info.nodes_per_face ids; the patch of every face
    std::vector<int32_t> origin;             // block, side (4 / 5: hub / shroud), e, g per face
};
// orientation: +-1 per block from the quality report (Mesh::quality, with layers the 3-D report), empty = +1; nk >= 2: the stacked mesh
inline Boundary boundary(discrete::Mesh& mesh, const Map& m, int order = 1, std::size_t nk = 0, const std::vector<int32_t>& orientation = {}, bool host = false) {
    smoothing::smooth::Desc d(mesh);
    Boundary r;
    core::check(tm_weld_boundary_plan(&d.desc, order, nk, &r.info, nullptr));
    r.patches.resize(r.info.patches);
    core::check(tm_weld_boundary_plan(&d.desc, order, nk, &r.info, r.patches.data()));
    if (!orientation.empty() && orientation.size() != mesh.blocks.size()) throw Error(TM_E_ARG, "one orientation per block");
    r.faces.resize(r.info.faces * r.info.nodes_per_face + 1), r.face_patch.resize(r.info.faces + 1), r.origin.resize(4 * r.info.faces + 1);
    core::check((host ? tm_weld_boundary_faces_host : tm_weld_boundary_faces)(&d.desc, m.map.data(), m.info.nodes_out, order, nk,
                                                                              orientation.empty() ? nullptr : orientation.data(), r.faces.data(), r.face_patch.data(),
                                                                              r.origin.data()));
    r.faces.resize(r.info.faces * r.info.nodes_per_face), r.face_patch.resize(r.info.faces), r.origin.resize(4 * r.info.faces);
    return r;
}
// measure, normal and moment of every patch on welded planes (x, y and, for a stacked mesh, z: npoints values each)
inline void measure(Boundary& b, int order, const std::vector<double>& x, const std::vector<double>& y, const std::vector<double>* z = nullptr, bool host = false) {
    const double* planes[3] = {x.data(), y.data(), z ? z->data() : nullptr};
    core::check((host ? tm_weld_faces_measure_host : tm_weld_faces_measure)(z ? 3 : 2, order, b.info.faces, b.faces.data(), b.face_patch.data(), b.patches.size(), x.size(),
                                                                            z ? 3 : 2, planes, b.patches.data()));
}
// from the coordinates RESIDENT in the handle (tm_smoother_weld_boundary): faces and measured patches, the welded points stay on the device
inline Boundary boundary(const smoothing::smooth::Smoother& s, int order = 1, const std::vector<int32_t>& orientation = {}) {
    Boundary r;
    core::check(tm_weld_boundary_plan(&s.desc(), order, 0, &r.info, nullptr));
    r.patches.resize(r.info.patches);
    r.faces.resize(r.info.faces * r.info.nodes_per_face + 1), r.face_patch.resize(r.info.faces + 1);
    core::check(tm_smoother_weld_boundary(s.handle(), order, orientation.empty() ? nullptr : orientation.data(), r.faces.data(), r.face_patch.data(), r.patches.data()));
    r.faces.resize(r.info.faces * r.info.nodes_per_face), r.face_patch.resize(r.info.faces);
    return r;
}
// wall distance of the welded mesh (tm_hip.h, kernel K20): per welded node the distance to the nearest face of the patches whose kind
// bit is set, the index of that face in Boundary::faces and the image under which it is nearest
struct WallDistance {
    std::vector<double> distance;
    std::vector<int32_t> face, image;
    tm_wall_info info{};
};
constexpr uint32_t wall_kinds_plane = (1u << TM_BC_WALL) | (1u << TM_PATCH_UNASSIGNED);
constexpr uint32_t wall_kinds_stacked = wall_kinds_plane | (1u << TM_PATCH_HUB) | (1u << TM_PATCH_SHROUD);
// b: the Boundary of order 1 (nk as it was made); x, y and, for a stacked mesh, z: the welded planes; images empty: the periodic
// translations of the mesh (tm_wall_select), otherwise the caller's (image 0 the identity)
inline WallDistance wall_distance(discrete::Mesh& mesh, const Boundary& b, std::size_t nk, const std::vector<double>& x, const std::vector<double>& y,
                                  const std::vector<double>* z = nullptr, uint32_t kinds = 0, std::vector<tm_wall_image> images = {}, bool host = false,
                                  uint32_t flags = 0) {
    smoothing::smooth::Desc d(mesh);
    if (kinds == 0) kinds = nk >= 2 ? wall_kinds_stacked : wall_kinds_plane;
    uint64_t nf = 0, ni = 0;
    core::check(tm_wall_select(&d.desc, nk, kinds, &nf, nullptr, &ni, nullptr));
    std::vector<int32_t> index(nf + 1);
    std::vector<tm_wall_image> plan(ni + 1);
    core::check(tm_wall_select(&d.desc, nk, kinds, &nf, index.data(), &ni, plan.data()));
    plan.resize(ni);
    if (images.empty()) images = plan;
    const std::size_t npf = b.info.nodes_per_face;
    std::vector<int32_t> faces(nf * npf + 1);
    for (uint64_t f = 0; f < nf; ++f)
        for (std::size_t k = 0; k < npf; ++k) faces[f * npf + k] = b.faces[static_cast<std::size_t>(index[f]) * npf + k];
    WallDistance r;
    r.distance.resize(x.size() + 1), r.face.resize(x.size() + 1), r.image.resize(x.size() + 1);
    const double* planes[3] = {x.data(), y.data(), z ? z->data() : nullptr};
    core::check((host ? tm_wall_distance_host : tm_wall_distance)(z ? 3 : 2, nf, faces.data(), x.size(), planes, images.size(), images.data(), flags, r.distance.data(),
                                                                  r.face.data(), r.image.data(), &r.info));
    r.distance.resize(x.size()), r.face.resize(x.size()), r.image.resize(x.size());
    for (int32_t& f : r.face)
        if (f >= 0) f = index[static_cast<std::size_t>(f)];
    return r;
}
// from the coordinates RESIDENT in the handle (tm_smoother_wall_distance): only the outputs cross
inline WallDistance wall_distance(const smoothing::smooth::Smoother& s, uint32_t kinds = wall_kinds_plane, uint32_t flags = 0) {
    const tm_mesh_desc& d = s.desc();
    std::size_t n = 0;
    for (uint64_t b = 0; b < d.nblocks; ++b) n += d.blocks[b].ni * d.blocks[b].nj;
    WallDistance r;
    r.distance.resize(n + 1), r.face.resize(n + 1), r.image.resize(n + 1);
    core::check(tm_smoother_wall_distance(s.handle(), kinds, flags, nullptr, r.distance.data(), r.face.data(), r.image.data(), &r.info));
    r.distance.resize(r.info.points), r.face.resize(r.info.points), r.image.resize(r.info.points);
    return r;
}
// faces of the welded mesh (tm_hip.h, kernel K21): interior faces with owner and neighbour in upper-triangular order, then the boundary
// of order 1 in its order; cell_faces: per cell of cells(mesh, m, 1, nk) and local side the face index
struct Faces {
    tm_fv_plan plan{};
    std::vector<int32_t> faces, owner, neighbour, cell_faces;
};
inline Faces faces(discrete::Mesh& mesh, const Map& m, std::size_t nk = 0, const std::vector<int32_t>& orientation = {}, bool host = false) {
    smoothing::smooth::Desc d(mesh);
    Faces r;
    core::check(tm_weld_faces_plan(&d.desc, nk, &r.plan));
    if (!orientation.empty() && orientation.size() != mesh.blocks.size()) throw Error(TM_E_ARG, "one orientation per block");
    const std::size_t n = r.plan.internal_faces + r.plan.boundary_faces;
    r.faces.resize(n * r.plan.nodes_per_face + 1), r.owner.resize(n + 1), r.neighbour.resize(r.plan.internal_faces + 1), r.cell_faces.resize(r.plan.cells * r.plan.faces_per_cell + 1);
    core::check((host ? tm_weld_faces_host : tm_weld_faces)(&d.desc, m.map.data(), m.info.nodes_out, nk, orientation.empty() ? nullptr : orientation.data(), r.faces.data(),
                                                            r.owner.data(), r.neighbour.data(), r.cell_faces.data()));
    r.faces.resize(n * r.plan.nodes_per_face), r.owner.resize(n), r.neighbour.resize(r.plan.internal_faces), r.cell_faces.resize(r.plan.cells * r.plan.faces_per_cell);
    return r;
}
// finite-volume metrics of such lists on welded planes (x, y and, for a stacked mesh, z); the optional per-cell and per-face fields
struct FvMetrics {
    tm_fv_info info{};
    std::vector<double> volume, cos;
};
inline FvMetrics fv_metrics(const Faces& f, const std::vector<double>& x, const std::vector<double>& y, const std::vector<double>* z = nullptr, bool host = false) {
    FvMetrics r;
    r.volume.resize(f.plan.cells + 1), r.cos.resize(f.owner.size() + 1);
    tm_fv_fields out{};
    out.volume = r.volume.data(), out.cos = r.cos.data();
    const double* planes[3] = {x.data(), y.data(), z ? z->data() : nullptr};
    core::check((host ? tm_fv_metrics_host : tm_fv_metrics)(z ? 3 : 2, f.plan.cells, f.plan.internal_faces, f.plan.boundary_faces, f.faces.data(), f.owner.data(),
                                                            f.neighbour.data(), f.cell_faces.data(), x.size(), planes, &out, &r.info));
    r.volume.resize(f.plan.cells), r.cos.resize(f.owner.size());
    return r;
}
// the record of the coordinates RESIDENT in the handle (tm_smoother_fv_report): only the record crosses
inline tm_fv_info fv_report(const smoothing::smooth::Smoother& s, const std::vector<int32_t>& orientation = {}) {
    tm_fv_info info{};
    core::check(tm_smoother_fv_report(s.handle(), orientation.empty() ? nullptr : orientation.data(), &info));
    return info;
}
}  // namespace weld

namespace discrete {
inline Quality Mesh::quality(bool host) {
    smoothing::smooth::Desc d(*this);
    Quality q;
    q.per_block.resize(blocks.size());
    check((host ? tm_mesh_quality_host : tm_mesh_quality)(&d.desc, q.per_block.data(), &q.total));
    return q;
}
// Mesh.write (discrete.zig:197-216): one plane per coordinate with i fastest (cgns.zig:75-104), transposed on the device
inline void write(const Mesh& m, const std::string& filename) {
    smoothing::smooth::detail::requirePlot3d(filename);
    std::FILE* f = std::fopen(filename.c_str(), "wb");
    if (!f) throw Error(TM_E_ARG, "cannot open " + filename);
    smoothing::smooth::detail::writeHeader(f, m);
    std::vector<double> x, y;
    for (const auto& b : m.blocks) {
        const std::size_t n = b.points.size[0] * b.points.size[1];
        x.resize(n);
        y.resize(n);
        check(tm_export_soa(&b.points.data[0].data[0], b.points.size[0], b.points.size[1], x.data(), y.data()));
        std::fwrite(x.data(), sizeof(double), n, f);
        std::fwrite(y.data(), sizeof(double), n, f);
    }
    std::fclose(f);
}
}  // namespace discrete
}  // namespace core
