// K9  mesh quality: one pass over a block gives its whole report (folded / degenerate cells, scaled Jacobian with its worst cell
//     and histogram, corner angles, aspect ratio, edge growth, areas).  gfx950, wave64.  Definitions: include/tm_hip.h; the
//     per-cell arithmetic is tm_quality.h, shared with the host loop, so device and host agree bit for bit.
//
// Layout.  Node (i,j) sits at i*nj + j, so a wave's lanes run along j and the wave MARCHES along i, one coalesced 16 B/lane load
// per node row, the previous row kept in registers.  The j+1 neighbour, and the i-edge of column j+1, come from the next lane by
// a DPP wave shift (the shifts of tm_kernels.hip); every edge length is ONE square root, shared by the two cells and the growth pair
// that use it.  Strips: a wave holds 64 node columns and owns the 62 cell columns [62 s, 62 s + 62): cell l needs lanes l and l + 1,
// the growth pair of the j-edges around node l needs lanes l - 1 .. l + 1, so neighbouring strips overlap by two columns (3 % of
// the loads, served by L2) and no wave needs a halo load or a square root for a neighbour's edge.  Row chunks: a workgroup (4 waves
// = 4 strips) takes `rows` cell rows; it re-reads the node row it shares with the chunk above and the one above that (the growth
// pair of the i-edges across the seam).  Extremes are idempotent, so an overlap only matters for counts and sums: cells are counted
// by their owner alone.
//
// Reductions: in-lane over the march, in-wave by shuffles, across the 4 waves through LDS, one QAcc record per workgroup; the
// histogram by integer LDS atomics.  k_quality_finalize (one launch, one workgroup per block) combines the records in fixed order
// and picks the orientation's candidate set (q_finish).  No floating-point atomics anywhere: results do not depend on scheduling.
#include "tm_quality_dev.hpp"
#include "tm_smoother.hpp"

#include <algorithm>
#include <cstring>

namespace tmh {

#define HIPCHK(x) hip_check((x), #x)

// the wave shifts of tm_kernels.hip (v_mov_b32_dpp wave_shl:1 / wave_shr:1): value of the next / previous lane, lane 63 / 0 keep their own
__device__ __forceinline__ double q_lane_next(double v) {
    int2 s = __builtin_bit_cast(int2, v), r;
    r.x = __builtin_amdgcn_update_dpp(s.x, s.x, 0x130 /* wave_shl:1 */, 0xf, 0xf, false);
    r.y = __builtin_amdgcn_update_dpp(s.y, s.y, 0x130, 0xf, 0xf, false);
    return __builtin_bit_cast(double, r);
}
__device__ __forceinline__ double q_lane_prev(double v) {
    int2 s = __builtin_bit_cast(int2, v), r;
    r.x = __builtin_amdgcn_update_dpp(s.x, s.x, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
    r.y = __builtin_amdgcn_update_dpp(s.y, s.y, 0x138, 0xf, 0xf, false);
    return __builtin_bit_cast(double, r);
}

constexpr int Q_THREADS = 256, Q_WAVES = Q_THREADS / 64, Q_STRIP = 62;

// Cell rows per workgroup.  Every workgroup does the same work, so a grid a little larger than what the device holds at a time runs as
// two rounds, the second one on a few CUs.  Large blocks therefore get the chunk height that fills whole rounds of 1024 workgroups
// (4 per CU on the 256 CUs of an MI355X; 69 rows at 4096^2: two re-read rows in 71 are 3 %).  The kernel as compiled takes 148 VGPRs,
// which holds 3 waves per SIMD = 768 workgroups: bringing it to 128 registers, or sizing the rounds by 768, is tuning left open.
// Blocks of fewer than 512 cell rows (the example meshes) take 4 rows: a lone wave needs ~1.2 us per row, so their launches are bound
// by the length of the march.
constexpr int Q_RESIDENT_WORKGROUPS = 256 * 4;
int quality_rows(int ni, int nj) {
    const int cells = ni - 1;
    if (cells < 512) return std::min(cells, 4);
    const long long gx = ((nj - 1 + Q_STRIP - 1) / Q_STRIP + Q_WAVES - 1) / Q_WAVES;
    const long long rounds = (gx * ((cells + 95) / 96) + Q_RESIDENT_WORKGROUPS - 1) / Q_RESIDENT_WORKGROUPS;   // chunks of up to ~96 rows
    const long long chunks = std::max<long long>(1, rounds * Q_RESIDENT_WORKGROUPS / gx);
    return static_cast<int>(std::max<long long>(16, (cells + chunks - 1) / chunks));
}
dim3 quality_grid(int ni, int nj) {
    const int strips = (nj - 1 + Q_STRIP - 1) / Q_STRIP, rows = quality_rows(ni, nj);
    return dim3((strips + Q_WAVES - 1) / Q_WAVES, (ni - 1 + rows - 1) / rows);
}
int quality_nwg(int ni, int nj) {
    const dim3 g = quality_grid(ni, nj);
    return static_cast<int>(g.x * g.y);
}

__device__ __forceinline__ unsigned long long q_shfl(unsigned long long v, int off) { return __shfl_down(v, off, 64); }

// partials: one record per workgroup (may be null when only the field is wanted); field: per-cell min of o*s, element j*(ni-1) + i
// (i fastest, like the export planes), or null.
__global__ __launch_bounds__(Q_THREADS) void k_quality(const double2* __restrict__ X, int ni, int nj, int rows, QAcc* __restrict__ partials,
                                                       double* __restrict__ field, int orientation) {
    __shared__ unsigned sh_hist[20];
    __shared__ QAcc sh_acc[Q_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < 20) sh_hist[threadIdx.x] = 0;
    __syncthreads();

    const int j0 = (static_cast<int>(blockIdx.x) * Q_WAVES + wave) * Q_STRIP;
    const int jj = j0 + lane;
    const int jc = jj < nj ? jj : nj - 1;   // lanes past the block read its last column; what they compute is masked below
    const int r0 = static_cast<int>(blockIdx.y) * rows;
    const int r1 = r0 + rows < ni - 1 ? r0 + rows : ni - 1;   // cell rows [r0, r1) = node rows r0 .. r1
    const bool own_cell = lane < Q_STRIP && jj + 1 < nj;               // cell (., jj): lanes l and l + 1 hold its columns
    const bool own_pair_j = lane >= 1 && lane <= Q_STRIP && jj + 1 < nj;   // j-edges (jj-1, jj) and (jj, jj+1)

    QAcc acc;
    q_init(acc);
    if (j0 < nj - 1 && r0 < r1) {   // wave-uniform: the strip has cells
        const double2* col = X + jc;
        auto node = [&](int i) {
            const double2 v = col[static_cast<size_t>(i) * nj];
            return QPoint{v.x, v.y};
        };
        auto next_of = [&](const QPoint& p) { return QPoint{q_lane_next(p.x), q_lane_next(p.y)}; };
        double l_i_prev = 0.0;   // i-edge above the current one (a zero length is skipped by q_growth: no pair on the first row of the block)
        QPoint prev = node(r0);
        if (r0 > 0) {
            double l2;
            q_edge(node(r0 - 1), prev, l2, l_i_prev);
        }
        QPoint prevN = next_of(prev);
        double l2_j_prev, l_j_prev;
        q_edge(prev, prevN, l2_j_prev, l_j_prev);
        const double l_jP0 = q_lane_prev(l_j_prev);   // shifts with every lane active, the selection afterwards
        if (r0 == 0 && own_pair_j) q_growth(l_jP0, l_j_prev, acc.gj);   // the other chunks' first row is their neighbour's last
        unsigned long long cell = static_cast<unsigned long long>(r0) * (nj - 1) + jj;
        QPoint cur = node(r0 + 1);
        for (int i = r0 + 1; i <= r1; ++i) {
            const QPoint nxt = node(i < r1 ? i + 1 : i);   // in flight while this row is evaluated
            const QPoint curN = next_of(cur);
            double l2_i, l_i, l2_j, l_j;
            q_edge(prev, cur, l2_i, l_i);
            q_edge(cur, curN, l2_j, l_j);
            const double l2_iN = q_lane_next(l2_i), l_iN = q_lane_next(l_i);
            const double l_jP = q_lane_prev(l_j);
            // cell (i-1, jj): A = prev, B = cur, C = curN, D = prevN
            const QCell c = q_cell(prev, cur, curN, prevN, l2_i, l_i, l2_iN, l_iN, l2_j_prev, l_j_prev, l2_j, l_j);
            if (own_cell) {
                const int bin = q_count_cell(c, cell, acc);
                if (bin >= 0) atomicAdd(&sh_hist[bin], 1u);
                if (field) field[static_cast<size_t>(jj) * (ni - 1) + (i - 1)] = q_field_value(c, orientation);
            }
            q_growth(l_i_prev, l_i, acc.gi);   // every lane holds a column of the block (clamped lanes repeat the last one)
            if (own_pair_j) q_growth(l_jP, l_j, acc.gj);
            prev = cur;
            prevN = curN;
            l2_j_prev = l2_j;
            l_j_prev = l_j;
            l_i_prev = l_i;
            cur = nxt;
            cell += static_cast<unsigned long long>(nj - 1);
        }
    }
    if (!partials) return;

    // in-wave, fixed tree
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        acc.deg += q_shfl(acc.deg, off);
        acc.jle0 += q_shfl(acc.jle0, off);
        acc.jge0 += q_shfl(acc.jge0, off);
        q_take_min(acc.smin, acc.imin, __shfl_down(acc.smin, off, 64), q_shfl(acc.imin, off));
        q_take_max(acc.smax, acc.imax, __shfl_down(acc.smax, off, 64), q_shfl(acc.imax, off));
        double v;
        v = __shfl_down(acc.cmin, off, 64);
        if (v < acc.cmin) acc.cmin = v;
        v = __shfl_down(acc.cmax, off, 64);
        if (v > acc.cmax) acc.cmax = v;
        v = __shfl_down(acc.aspect, off, 64);
        if (v > acc.aspect) acc.aspect = v;
        v = __shfl_down(acc.gi, off, 64);
        if (v > acc.gi) acc.gi = v;
        v = __shfl_down(acc.gj, off, 64);
        if (v > acc.gj) acc.gj = v;
        v = __shfl_down(acc.amin, off, 64);
        if (v < acc.amin) acc.amin = v;
        v = __shfl_down(acc.amax, off, 64);
        if (v > acc.amax) acc.amax = v;
        acc.asum += __shfl_down(acc.asum, off, 64);
        acc.aabs += __shfl_down(acc.aabs, off, 64);
    }
    if (lane == 0) sh_acc[wave] = acc;   // hist is zero in every lane: the bins are in sh_hist
    __syncthreads();
    if (threadIdx.x == 0) {
        QAcc t = sh_acc[0];
        for (int w = 1; w < Q_WAVES; ++w) q_combine(t, sh_acc[w]);
        for (int k = 0; k < 20; ++k) t.hist[k / 10][k % 10] = sh_hist[k];
        partials[static_cast<size_t>(blockIdx.y) * gridDim.x + blockIdx.x] = t;
    }
}

// one workgroup (one wave) per block combines the block's records in the fixed order of records_reduce_wave, so the sums are the same on every run
__global__ __launch_bounds__(64) void k_quality_finalize(const QAcc* __restrict__ partials, const QBlockDesc* __restrict__ desc, tm_quality* __restrict__ out) {
    __shared__ QAcc sh[64];
    const QBlockDesc d = desc[blockIdx.x];
    records_reduce_wave<QAcc, q_init, q_combine>(partials + d.first, 0, d.nwg, sh);
    if (threadIdx.x == 0) q_finish(sh[0], d.block, static_cast<uint64_t>(d.ni), static_cast<uint64_t>(d.nj), &out[blockIdx.x]);
}

// ------------------------------------------------------------------ host driver
QualityDev::~QualityDev() { release(); }
void QualityDev::release() {
    for (DevBuf* b : {&partials, &desc, &out, &field}) b->release();
    if (h_out) (void)hipHostFree(h_out);
    h_out = nullptr;
    desc_host.clear();
    blocks_cap = 0;
}

void QualityDev::run(const std::vector<QualityBlock>& blocks, hipStream_t st, tm_quality* host_out) {
    if (blocks.empty()) return;
    // the records buffer is sized from the very grids that write it
    std::vector<QBlockDesc> d(blocks.size());
    size_t nrec = 0;
    for (size_t k = 0; k < blocks.size(); ++k) {
        d[k] = QBlockDesc{static_cast<long long>(nrec), quality_nwg(blocks[k].ni, blocks[k].nj), blocks[k].ni, blocks[k].nj, 0, blocks[k].block};
        nrec += static_cast<size_t>(d[k].nwg);
    }
    partials.grow(sizeof(QAcc) * nrec, "quality records");
    if (blocks_cap < blocks.size()) {
        desc.grow(sizeof(QBlockDesc) * blocks.size(), "quality block table");
        out.grow(sizeof(tm_quality) * blocks.size(), "quality results");
        blocks_cap = blocks.size();
        if (h_out) (void)hipHostFree(h_out);
        h_out = nullptr;
        desc_host.clear();
        if (hipHostMalloc(reinterpret_cast<void**>(&h_out), sizeof(tm_quality) * blocks.size(), hipHostMallocDefault) != hipSuccess) throw TmError(TM_E_MEMORY, "hipHostMalloc failed (quality results)");
    }
    if (desc_host.size() != d.size() || std::memcmp(desc_host.data(), d.data(), sizeof(QBlockDesc) * d.size()) != 0) {
        HIPCHK(hipMemcpy(desc.p, d.data(), sizeof(QBlockDesc) * d.size(), hipMemcpyHostToDevice));   // blocking: d is a local
        desc_host = d;
    }
    for (size_t k = 0; k < blocks.size(); ++k) {
        const dim3 grid = quality_grid(blocks[k].ni, blocks[k].nj);
        if (d[k].first + static_cast<long long>(grid.x) * grid.y > static_cast<long long>(partials.cap / sizeof(QAcc)))
            throw TmError(TM_E_OVERFLOW, "quality records buffer smaller than the launch grid");
        hipLaunchKernelGGL(k_quality, grid, dim3(Q_THREADS), 0, st, blocks[k].xy, blocks[k].ni, blocks[k].nj, quality_rows(blocks[k].ni, blocks[k].nj), partials.as<QAcc>() + d[k].first,
                           static_cast<double*>(nullptr), 0);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_quality_finalize, dim3(static_cast<unsigned>(blocks.size())), dim3(64), 0, st, partials.as<QAcc>(), desc.as<QBlockDesc>(), out.as<tm_quality>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_out, out.p, sizeof(tm_quality) * blocks.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (host_out) {
        std::memcpy(host_out, h_out, sizeof(tm_quality) * blocks.size());
        for (size_t k = 0; k < blocks.size(); ++k) quality_angles(&host_out[k]);
    }
}

void QualityDev::run_field(const QualityBlock& b, int orientation, hipStream_t st, double* host_field) {
    const size_t cells = static_cast<size_t>(b.ni - 1) * (b.nj - 1);
    field.grow(sizeof(double) * cells, "quality cell plane");
    hipLaunchKernelGGL(k_quality, quality_grid(b.ni, b.nj), dim3(Q_THREADS), 0, st, b.xy, b.ni, b.nj, quality_rows(b.ni, b.nj), static_cast<QAcc*>(nullptr), field.as<double>(), orientation);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(host_field, field.p, sizeof(double) * cells, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
}

// ------------------------------------------------------------------ handle: the coordinates resident in X
static std::vector<QualityBlock> owned_quality_blocks(const Smoother& s) {
    std::vector<QualityBlock> v;
    for (size_t k = 0; k < s.lp.owned_blocks.size(); ++k) {
        const int64_t b = s.lp.owned_blocks[k];
        v.push_back(QualityBlock{s.X + s.lp.local_start[k], static_cast<int>(s.topo.ni[b]), static_cast<int>(s.topo.nj[b]), static_cast<uint64_t>(b)});
    }
    return v;
}

void Smoother::quality_host(tm_quality* per_block, tm_quality* total) {
    for (int64_t b = 0; b < topo.nblocks(); ++b)
        if (topo.ni[b] < 2 || topo.nj[b] < 2) throw TmError(TM_E_SIZE, "InconsistentSize: a block needs at least 2 x 2 nodes");
    if (!qdev) qdev = new QualityDev();
    const std::vector<QualityBlock> blocks = owned_quality_blocks(*this);
    std::vector<tm_quality> own(blocks.size()), all(static_cast<size_t>(topo.nblocks()));
    qdev->run(blocks, stream, own.data());
    std::memset(all.data(), 0, sizeof(tm_quality) * all.size());   // blocks of other ranks stay zero
    for (size_t k = 0; k < blocks.size(); ++k) all[blocks[k].block] = own[k];
    if (per_block) std::memcpy(per_block, all.data(), sizeof(tm_quality) * all.size());
    if (total) quality_total(all.data(), all.size(), total);
}

void Smoother::quality_field_host(int64_t block, double* out) {
    const auto it = std::lower_bound(lp.owned_blocks.begin(), lp.owned_blocks.end(), block);
    if (block < 0 || it == lp.owned_blocks.end() || *it != block) throw TmError(TM_E_ARG, "block is not owned by this rank");
    if (topo.ni[block] < 2 || topo.nj[block] < 2) throw TmError(TM_E_SIZE, "InconsistentSize: a block needs at least 2 x 2 nodes");
    if (!qdev) qdev = new QualityDev();
    const QualityBlock b{X + lp.local_start[it - lp.owned_blocks.begin()], static_cast<int>(topo.ni[block]), static_cast<int>(topo.nj[block]), static_cast<uint64_t>(block)};
    tm_quality q;
    qdev->run({b}, stream, &q);   // the orientation first (a cheap pass beside the copy of the plane)
    qdev->run_field(b, q.orientation, stream, out);
}

}  // namespace tmh
