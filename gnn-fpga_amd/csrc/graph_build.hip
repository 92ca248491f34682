// graph_build.hip - track-segment graphs from detector hits on the GPU.
//
// The reference builds one graph per (event, phi sector) on the host: split_phi_sectors (gnn/prepareGraphs.py:87-106),
// then construct_graph (gnn/graph.py:37-142), which merges every hit of layer l1 with every hit of layer l2 in pandas,
// keeps the pairs that pass a phi-slope and a z0 cut, and builds two dense [N, E] uint8 matrices to find their
// indices.  gnn-fpga_amd/graph_build.py is the numpy specification of what is computed here, and why it is float32;
// the selected set is bit-identical to the reference's: the cut arithmetic (keep_pair, builder_common.h) is the same
// float32 operations in the same order, with contraction to FMA off (the pragma), IEEE division, and the sector test
// in float64 as pandas does it.
//
//   gnn_graph_build_sizes
//     k_gb_key       one lane per hit: its event (binary search of event_ptr), sector, (graph, layer) bucket; counts
//                    per bucket (atomics: counts only)
//     scan           bucket counts -> bucket offsets (buckets graph-major: hit_ptr[g] = boff[g * L])
//     k_gb_scatter   one lane per hit: a slot in its bucket (atomic order)
//     k_gb_rank      one lane per slot: the hit's rank in its bucket by input row -> frame order in every (graph,
//                    layer), whatever order the atomics arrived in; stages r, centred phi, z in that order (SoA)
//     k_gb_tasks     one lane per (graph, pair): rows = its l1 hits (0 when l2 has none), tasks of kRows rows
//     scan           rows and tasks (two arrays, one launch) -> row_base, task_base
//     k_gb_pairs<0>  one workgroup per task, one lane per l1 hit; the l2 hits are staged in LDS as SoA tiles of kTile
//                    and every lane reads the same word (a broadcast); counts the kept partners per row
//     scan           row counts -> each row's first segment
//     k_gb_final     one lane per graph: hit_ptr, seg_ptr, the sizes and the status word
//   gnn_graph_build_fill
//     k_gb_features  one lane per hit: its position in its graph (frame order: a binary search per layer bucket),
//                    X = float32(float64(v) / scale), hit_index
//     k_gb_pairs<1>  the same pair test again; each lane writes its row's src, dst, y from the row's offset
//   gnn_cut_study  (the all-pair histograms of gnn/GraphConstructionDev.ipynb cell 20 and
//                   gnn/GraphConstructionDev_mu200.ipynb cell 18; gnn-fpga_amd/cut_study.py is the specification)
//     the staging of gnn_graph_build_sizes, unchanged: k_gb_key .. k_gb_tasks and both scans (stage_gb)
//     k_cs_pairs     the task loop of k_gb_pairs with a histogram where the cut test is: the l2 tiles carry the
//                    particle id, each pair's (|phi_slope| bin, |z0| bin) cell of its class (fake / true) is counted in
//                    an LDS table of 32-bit counters (LDS atomics), the last-by-last cell - where an all-pairs loop puts
//                    most pairs - in a register and reduced over the wave; the table is added to the int64 counts with
//                    64-bit atomics when the task ends.  Integer sums only: every run gives the same bits.
// Nothing is ordered by atomics: two builds of one input give the same bits.
#include "common.h"

#include <cmath>

#pragma clang fp contract(off)

#include "builder_common.h"

namespace gnn {
namespace {

constexpr int kMaxPairs = 128;
constexpr int kRows = 128;                             // l1 hits per task (one per lane)
constexpr int kTile = 512;                             // l2 hits per LDS tile
constexpr int kTaskWgPerCu = 8;
constexpr int kMaxCells = 4096;                        // (NS + 1) * (NZ + 1) histogram cells per class: 32 KB of LDS
constexpr int64_t kStudyHitsEnd = (int64_t)1 << 25;    // kRows * (hits of one layer) must fit a 32-bit LDS counter

struct PairTab {                                       // by value: layer_pairs and the cut each pair takes
    int32_t l1[kMaxPairs], l2[kMaxPairs];
    float cut[kMaxPairs];
};

// np.linspace(-pi, pi, S + 1)[i]: i * step + start, the last one = stop (numpy's own steps, no FMA)
__device__ __forceinline__ double sector_edge(int i, int S, double step)
{
    return i == S ? M_PI : __dadd_rn(__dmul_rn((double)i, step), -M_PI);
}

__device__ __forceinline__ int sector_of(float phi, int S, double step)
{
    const double p = phi;
    if (!(p > -4.0 && p < 4.0)) return -1;             // NaN, or outside [-pi, pi]
    const int c = (int)floor((p + M_PI) / step);
    for (int k = max(c - 1, 0); k <= min(c + 1, S - 1); ++k)
        if (p > sector_edge(k, S, step) && p < sector_edge(k + 1, S, step)) return k;
    return -1;                                         // on an edge: in no sector (strict bounds)
}

struct GbWs {
    int32_t *status;                                   // head: [status | pad] [total segments u64] ...
    unsigned long long *total;
    int32_t *bcnt, *bfill, *boff;                      // [B], [B], [B + 1]
    int32_t *gpc, *rbase, *tbase;                      // [2 * gp_stride], [GP + 1], [GP + 1]
    int32_t *hkey, *unsorted, *lrow, *lout;            // [n] each
    float *lr, *lphi, *lz;                             // [n] each
    int32_t *rcnt, *roff;                              // [RB], [RB + 1]
    int32_t *sums;
    int64_t G, B, GP, gp_stride, RB, head_bytes;
    size_t bytes;
};

// row bound: a hit is an l1 row once for every pair whose first layer is its layer
int64_t row_bound(int64_t n_hits, const int32_t *pairs, int n_pairs)
{
    int mult = 0;
    for (int p = 0; p < n_pairs; ++p) {
        int m = 0;
        for (int q = 0; q < n_pairs; ++q) m += pairs[2 * q] == pairs[2 * p];
        mult = max(mult, m);
    }
    return n_hits * mult;
}

GbWs carve_gb(char *base, int64_t n, int64_t E, int L, int P, int S, int64_t RB)
{
    GbWs w;
    w.G = E * S;
    w.B = w.G * L;
    w.GP = w.G * P;
    w.gp_stride = (w.GP + 64) & ~(int64_t)63;
    w.RB = RB;
    Carver c{base};
    // [head 256 B | bcnt | bfill]: cleared by ONE memset
    w.head_bytes = 256 + 2 * w.B * (int64_t)sizeof(int32_t);
    char *head = c.take<char>(w.head_bytes);
    w.status = reinterpret_cast<int32_t *>(head);
    w.total = head ? reinterpret_cast<unsigned long long *>(head + 8) : nullptr;
    w.bcnt = head ? reinterpret_cast<int32_t *>(head + 256) : nullptr;
    w.bfill = w.bcnt ? w.bcnt + w.B : nullptr;
    w.boff = c.take<int32_t>(w.B + 1);
    w.gpc = c.take<int32_t>(2 * w.gp_stride);
    w.rbase = c.take<int32_t>(w.GP + 1);
    w.tbase = c.take<int32_t>(w.GP + 1);
    w.hkey = c.take<int32_t>(n);
    w.unsorted = c.take<int32_t>(n);
    w.lrow = c.take<int32_t>(n);
    w.lout = c.take<int32_t>(n);
    w.lr = c.take<float>(n);
    w.lphi = c.take<float>(n);
    w.lz = c.take<float>(n);
    w.rcnt = c.take<int32_t>(RB);
    w.roff = c.take<int32_t>(RB + 1);
    w.sums = c.take<int32_t>(scan_sums_words(max(max(w.B, w.GP), RB)));
    w.bytes = c.bytes();
    return w;
}

__global__ __launch_bounds__(kBlock) void k_gb_key(const float *__restrict__ phi, const int32_t *__restrict__ layer,
                                                   int64_t n, const int64_t *__restrict__ ep, int64_t E, int S, int L,
                                                   double step, int32_t *__restrict__ hkey, int32_t *__restrict__ bcnt,
                                                   int32_t *__restrict__ status)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    check_event_ptr(ep, E, n, i, status);
    if (i >= n) return;
    const int64_t lo = last_le(ep, E, i);              // the event
    const int l = layer[i];
    int key = -1;
    if (l < 0 || l >= L) {
        atomicOr(status, kStatusLayer);
    } else if (event_owns(ep, lo, i)) {
        const int s = sector_of(phi[i], S, step);
        if (s >= 0) {
            key = (int)((lo * S + s) * L + l);
            atomicAdd(bcnt + key, 1);
        }
    }
    hkey[i] = key;
}

__global__ __launch_bounds__(kBlock) void k_gb_scatter(const int32_t *__restrict__ hkey, int64_t n,
                                                       const int32_t *__restrict__ boff, int32_t *__restrict__ bfill,
                                                       int32_t *__restrict__ unsorted)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int key = hkey[i];
    if (key >= 0) unsorted[boff[key] + atomicAdd(bfill + key, 1)] = (int)i;
}

// rank in the bucket = number of its hits with a smaller input row (buckets are a graph's hits on one layer: ~100-1000)
__global__ __launch_bounds__(kBlock) void k_gb_rank(const float *__restrict__ r, const float *__restrict__ phi,
                                                    const float *__restrict__ z, int64_t n,
                                                    const int32_t *__restrict__ hkey, const int32_t *__restrict__ boff,
                                                    const int32_t *__restrict__ bcnt, int64_t B, int S, int L,
                                                    double step, float half, const int32_t *__restrict__ unsorted,
                                                    int32_t *__restrict__ lrow, float *__restrict__ lr,
                                                    float *__restrict__ lphi, float *__restrict__ lz)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n || j >= boff[B]) return;
    const int row = unsorted[j], key = hkey[row];
    const int b0 = boff[key], m = bcnt[key];
    int rank = 0;
    for (int k = 0; k < m; ++k) rank += unsorted[b0 + k] < row;
    const int slot = b0 + rank;
    const int s = (key / L) % S;
    lrow[slot] = row;
    lr[slot] = r[row];
    lphi[slot] = (phi[row] - (float)sector_edge(s, S, step)) - half;   // gnn/prepareGraphs.py:103, float32
    lz[slot] = z[row];
}

__global__ __launch_bounds__(kBlock) void k_gb_tasks(const int32_t *__restrict__ bcnt, int64_t GP, int P, int L,
                                                     PairTab pt, int32_t *__restrict__ gpc, int64_t gp_stride)
{
    const int64_t gp = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gp >= GP) return;
    const int64_t g = gp / P;
    const int p = (int)(gp - g * P);
    const int n1 = bcnt[g * L + pt.l1[p]], n2 = bcnt[g * L + pt.l2[p]];
    const int rows = n2 > 0 ? n1 : 0;
    gpc[gp] = rows;
    gpc[gp_stride + gp] = (rows + kRows - 1) / kRows;
}

// FILL = 0: kept partners per row -> rcnt (and the total); FILL = 1: src, dst, y of every row from roff
template <int FILL>
__global__ __launch_bounds__(kRows) void k_gb_pairs(int64_t GP, int P, int L, PairTab pt, float z0_max,
                                                    const int32_t *__restrict__ tbase, const int32_t *__restrict__ rbase,
                                                    const int32_t *__restrict__ bcnt, const int32_t *__restrict__ boff,
                                                    const float *__restrict__ lr, const float *__restrict__ lphi,
                                                    const float *__restrict__ lz, int32_t *__restrict__ rcnt,
                                                    unsigned long long *__restrict__ total,
                                                    const int32_t *__restrict__ roff, const int32_t *__restrict__ lout,
                                                    const int32_t *__restrict__ lrow, const int64_t *__restrict__ pid,
                                                    int32_t *__restrict__ src, int32_t *__restrict__ dst,
                                                    float *__restrict__ y)
{
    __shared__ float sr[kTile], sp[kTile], sz[kTile];
    __shared__ int32_t so[FILL ? kTile : 1];
    __shared__ int64_t sid[FILL ? kTile : 1];
    const int n_tasks = tbase[GP];
    const bool with_y = FILL && y != nullptr;
    unsigned long long acc = 0;
    for (int t = blockIdx.x; t < n_tasks; t += gridDim.x) {
        const int64_t gp = last_le(tbase, GP, t), g = gp / P;   // the (graph, pair) of the task
        const int p = (int)(gp - g * P);
        const int k1 = (int)(g * L + pt.l1[p]), k2 = (int)(g * L + pt.l2[p]);
        const int n1 = bcnt[k1], n2 = bcnt[k2], b1 = boff[k1], b2 = boff[k2];
        const float cut = pt.cut[p];
        const int j = (t - tbase[gp]) * kRows + (int)threadIdx.x;
        const bool valid = j < n1;
        float r1 = 0.f, p1 = 0.f, z1 = 0.f;
        int out1 = 0, o = 0, cnt = 0;
        int64_t id1 = 0;
        if (valid) {
            r1 = lr[b1 + j];
            p1 = lphi[b1 + j];
            z1 = lz[b1 + j];
            if (FILL) {
                out1 = lout[b1 + j];
                o = roff[rbase[gp] + j];
                if (with_y) id1 = pid[lrow[b1 + j]];
            }
        }
        for (int t0 = 0; t0 < n2; t0 += kTile) {
            const int m = min(kTile, n2 - t0);
            __syncthreads();                           // the previous tile has been read
            for (int k = threadIdx.x; k < m; k += kRows) {
                sr[k] = lr[b2 + t0 + k];
                sp[k] = lphi[b2 + t0 + k];
                sz[k] = lz[b2 + t0 + k];
                if (FILL) {
                    so[k] = lout[b2 + t0 + k];
                    if (with_y) sid[k] = pid[lrow[b2 + t0 + k]];
                }
            }
            __syncthreads();
            if (valid) {
                for (int k = 0; k < m; ++k) {
                    if (keep_pair(r1, p1, z1, sr[k], sp[k], sz[k], cut, z0_max)) {   // gnn/graph.py:43-66
                        if (FILL) {
                            src[o] = out1;
                            dst[o] = so[k];
                            if (with_y) y[o] = id1 == sid[k] ? 1.0f : 0.0f;
                            ++o;
                        } else {
                            ++cnt;
                        }
                    }
                }
            }
        }
        if (!FILL && valid) {
            rcnt[rbase[gp] + j] = cnt;
            acc += (unsigned)cnt;
        }
    }
    if (!FILL) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) acc += __shfl_xor(acc, s, 64);
        if ((threadIdx.x & 63) == 0 && acc) atomicAdd(total, acc);
    }
}

// the number of edges <= v (np.searchsorted(edges, v, side="right")); NaN counts as above every edge
__device__ __forceinline__ int bin_of(const float *edges, int n, float v)
{
    if (v != v) return n;
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (edges[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the histogram twin of k_gb_pairs<0>: the same tasks, rows and tiles; counts [P][2][NS + 1][NZ + 1] (zeroed before)
__global__ __launch_bounds__(kRows) void k_cs_pairs(int64_t GP, int P, int L, PairTab pt,
                                                    const int32_t *__restrict__ tbase,
                                                    const int32_t *__restrict__ bcnt, const int32_t *__restrict__ boff,
                                                    const float *__restrict__ lr, const float *__restrict__ lphi,
                                                    const float *__restrict__ lz, const int32_t *__restrict__ lrow,
                                                    const int64_t *__restrict__ pid,
                                                    const float *__restrict__ slope_edges, int NS,
                                                    const float *__restrict__ z0_edges, int NZ,
                                                    unsigned long long *__restrict__ counts)
{
    __shared__ float sr[kTile], sp[kTile], sz[kTile];
    __shared__ int64_t sid[kTile];
    extern __shared__ unsigned int cs_dyn[];           // sized by the launch: the table, then the edges
    const int WZ = NZ + 1, cells = (NS + 1) * WZ;
    unsigned int *hist = cs_dyn;                       // [class][slope bin][z0 bin]
    float *sedge = reinterpret_cast<float *>(cs_dyn + 2 * cells);   // [slope edges | z0 edges]
    const float *es = sedge, *ez = sedge + NS;
    for (int k = threadIdx.x; k < NS + NZ; k += kRows) sedge[k] = k < NS ? slope_edges[k] : z0_edges[k - NS];
    for (int k = threadIdx.x; k < 2 * cells; k += kRows) hist[k] = 0;
    __syncthreads();
    const float last_s = es[NS - 1], last_z = ez[NZ - 1];
    const int n_tasks = tbase[GP];
    for (int t = blockIdx.x; t < n_tasks; t += gridDim.x) {
        const int64_t gp = last_le(tbase, GP, t), g = gp / P;   // the (graph, pair) of the task
        const int p = (int)(gp - g * P);
        const int k1 = (int)(g * L + pt.l1[p]), k2 = (int)(g * L + pt.l2[p]);
        const int n1 = bcnt[k1], n2 = bcnt[k2], b1 = boff[k1], b2 = boff[k2];
        const int j = (t - tbase[gp]) * kRows + (int)threadIdx.x;
        const bool valid = j < n1;
        float r1 = 0.f, p1 = 0.f, z1 = 0.f;
        int64_t id1 = 0;
        if (valid) {
            r1 = lr[b1 + j];
            p1 = lphi[b1 + j];
            z1 = lz[b1 + j];
            id1 = pid[lrow[b1 + j]];
        }
        unsigned int far_fake = 0, far_true = 0;       // the last-by-last cell: both cuts failed
        for (int t0 = 0; t0 < n2; t0 += kTile) {
            const int m = min(kTile, n2 - t0);
            __syncthreads();                           // the previous tile has been read
            for (int k = threadIdx.x; k < m; k += kRows) {
                sr[k] = lr[b2 + t0 + k];
                sp[k] = lphi[b2 + t0 + k];
                sz[k] = lz[b2 + t0 + k];
                sid[k] = pid[lrow[b2 + t0 + k]];
            }
            __syncthreads();
            if (valid) {
                for (int k = 0; k < m; ++k) {
                    float slope, z0;
                    pair_slope_z0(r1, p1, z1, sr[k], sp[k], sz[k], slope, z0);   // gnn/graph.py:57-62
                    const float a = fabsf(slope), b = fabsf(z0);
                    const bool same = id1 == sid[k];
                    if (!(a < last_s) && !(b < last_z)) {                        // NaN too
                        far_true += same;
                        far_fake += !same;
                    } else {
                        atomicAdd(&hist[(same ? cells : 0) + bin_of(es, NS, a) * WZ + bin_of(ez, NZ, b)], 1u);
                    }
                }
            }
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            far_fake += __shfl_xor(far_fake, s, 64);
            far_true += __shfl_xor(far_true, s, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            if (far_fake) atomicAdd(&hist[cells - 1], far_fake);
            if (far_true) atomicAdd(&hist[2 * cells - 1], far_true);
        }
        __syncthreads();
        // (a task sees at most kRows * n2 pairs and check_study keeps n2 below 2^25: 32 bits hold them)
        for (int k = threadIdx.x; k < 2 * cells; k += kRows) {
            const unsigned int c = hist[k];
            if (c) {
                atomicAdd(counts + (int64_t)p * 2 * cells + k, (unsigned long long)c);
                hist[k] = 0;
            }
        }
        __syncthreads();
    }
}

__global__ void k_cs_final(const int32_t *__restrict__ status, int64_t *__restrict__ status_out)
{
    *status_out = *status;
}

__global__ __launch_bounds__(kBlock) void k_gb_final(int64_t G, int P, int L, const int32_t *__restrict__ boff,
                                                     const int32_t *__restrict__ rbase, const int32_t *__restrict__ tbase,
                                                     const int32_t *__restrict__ roff, const int32_t *__restrict__ status,
                                                     const unsigned long long *__restrict__ total,
                                                     gnn_graph_build_sizes_t *sizes, int64_t *__restrict__ hit_ptr,
                                                     int64_t *__restrict__ seg_ptr)
{
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g > G) return;
    const bool ovf = *total > 0x7FFFFFFFull;
    const int64_t hp = boff[g * L], sp = ovf ? 0 : roff[rbase[g * P]];
    hit_ptr[g] = hp;
    seg_ptr[g] = sp;
    if (g < G) {
        atomicMax(reinterpret_cast<unsigned long long *>(&sizes->max_graph_hits),
                  (unsigned long long)(boff[(g + 1) * L] - hp));
        if (!ovf)
            atomicMax(reinterpret_cast<unsigned long long *>(&sizes->max_graph_segments),
                      (unsigned long long)(roff[rbase[(g + 1) * P]] - sp));
    } else {
        sizes->n_graphs = G;
        sizes->n_hits = hp;
        sizes->n_segments = (int64_t)*total;
        sizes->n_rows = rbase[G * P];
        sizes->n_tasks = tbase[G * P];
        sizes->status = *status | (ovf ? kStatusInt32 : 0);
    }
}

__global__ __launch_bounds__(kBlock) void k_gb_features(int64_t n_out, int L, const int32_t *__restrict__ hkey,
                                                        const int32_t *__restrict__ boff, const int32_t *__restrict__ bcnt,
                                                        const int32_t *__restrict__ lrow, const float *__restrict__ lr,
                                                        const float *__restrict__ lphi, const float *__restrict__ lz,
                                                        double sc_r, double sc_phi, double sc_z,
                                                        int32_t *__restrict__ lout, float *__restrict__ X,
                                                        int64_t *__restrict__ hit_index)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n_out) return;
    const int row = lrow[j];
    const int64_t g = hkey[row] / L;
    int pos = boff[g * L];                             // + hits of the graph with a smaller input row, layer by layer
    for (int l = 0; l < L; ++l) {
        int a = boff[g * L + l], b = a + bcnt[g * L + l];
        const int b0 = a;
        while (a < b) {
            const int mid = (a + b) >> 1;
            if (lrow[mid] < row) a = mid + 1; else b = mid;
        }
        pos += a - b0;
    }
    lout[j] = pos;
    hit_index[pos] = row;
    X[3 * (int64_t)pos + 0] = feature(lr[j], sc_r);    // gnn/graph.py:118, the divide in float64
    X[3 * (int64_t)pos + 1] = feature(lphi[j], sc_phi);
    X[3 * (int64_t)pos + 2] = feature(lz[j], sc_z);
}

int check_common(const char *who, int64_t n_hits, int64_t n_events, const int32_t *pairs, int32_t n_pairs,
                 int32_t n_layers, int32_t n_phi_sectors, int64_t *rb)
{
    if (n_hits < 0 || n_events < 1 || n_pairs < 0 || n_layers < 1 || n_phi_sectors < 1 || (n_pairs > 0 && !pairs))
        return fail(GNN_ERR_BADARG, "%s: bad argument (n_hits %lld, n_events %lld, n_pairs %d, n_layers %d, "
                    "n_phi_sectors %d)", who, (long long)n_hits, (long long)n_events, n_pairs, n_layers, n_phi_sectors);
    for (int p = 0; p < 2 * n_pairs; ++p)
        if (pairs[p] < 0 || pairs[p] >= n_layers)
            return fail(GNN_ERR_BADARG, "%s: layer_pairs entry %d = %d outside [0, %d)", who, p, pairs[p], n_layers);
    if (n_pairs > kMaxPairs) return fail(GNN_ERR_UNSUPPORTED, "%s: more than %d layer pairs", who, kMaxPairs);
    *rb = row_bound(n_hits, pairs, n_pairs);
    const int64_t G = n_events * n_phi_sectors;
    if (n_hits >= kInt32End || n_events >= kInt32End || G * n_layers >= kInt32End || G * n_pairs >= kInt32End ||
        *rb >= kInt32End)
        return fail(GNN_ERR_UNSUPPORTED, "%s: sizes outside the int32 index range", who);
    return 0;
}

PairTab pair_tab(const int32_t *pairs, int n_pairs, float psm, float pso)
{
    PairTab pt = {};
    for (int p = 0; p < n_pairs; ++p) {
        pt.l1[p] = pairs[2 * p];
        pt.l2[p] = pairs[2 * p + 1];
        pt.cut[p] = pairs[2 * p] < 5 ? psm : pso;      // gnn/graph.py:65: chosen by the pair's first layer
    }
    return pt;
}

int check_study(const char *who, int64_t n_hits, int32_t n_slope_edges, int32_t n_z0_edges)
{
    if (n_slope_edges < 1 || n_z0_edges < 1)
        return fail(GNN_ERR_BADARG, "%s: each axis needs at least one edge (got %d and %d)", who, n_slope_edges,
                    n_z0_edges);
    if (((int64_t)n_slope_edges + 1) * ((int64_t)n_z0_edges + 1) > kMaxCells)
        return fail(GNN_ERR_UNSUPPORTED, "%s: (%d + 1) x (%d + 1) histogram cells, at most %d fit the LDS table", who,
                    n_slope_edges, n_z0_edges, kMaxCells);
    if (n_hits >= kStudyHitsEnd)
        return fail(GNN_ERR_UNSUPPORTED, "%s: %lld hits, a study call takes fewer than 2^25 (study the data in chunks "
                    "and add the counts)", who, (long long)n_hits);
    return 0;
}

// the staging the sizes pass and the cut study share: sectors, the (graph, layer) buckets in frame order with r, centred
// phi and z staged in that order, and the (graph, pair) rows and tasks
int stage_gb(const char *who, const GbWs &w, const PairTab &pt, const float *r, const float *phi, const float *z,
             const int32_t *layer, int64_t n, const int64_t *event_ptr, int64_t n_events, int n_pairs, int n_layers,
             int n_phi_sectors, hipStream_t s)
{
    const double step = (M_PI - -M_PI) / n_phi_sectors;
    const float half = (float)(step / 2);
    const hipError_t err = hipMemsetAsync(w.status, 0, (size_t)w.head_bytes, s);
    if (err != hipSuccess) return fail(-(int)err, "%s: memset failed: %s", who, hipGetErrorString(err));
    GNN_LAUNCH("k_gb_key", k_gb_key, max(grid_for(max(n, n_events)), 1u), kBlock, s, phi, layer, n, event_ptr, n_events,
               n_phi_sectors, n_layers, step, w.hkey, w.bcnt, w.status);
    if (int rc = scan_counts(w.bcnt, 0, 1, w.boff, nullptr, w.B, w.sums, s)) return rc;
    if (n > 0) {
        GNN_LAUNCH("k_gb_scatter", k_gb_scatter, grid_for(n), kBlock, s, w.hkey, n, w.boff, w.bfill, w.unsorted);
        GNN_LAUNCH("k_gb_rank", k_gb_rank, grid_for(n), kBlock, s, r, phi, z, n, w.hkey, w.boff, w.bcnt, w.B,
                   n_phi_sectors, n_layers, step, half, w.unsorted, w.lrow, w.lr, w.lphi, w.lz);
    }
    if (w.GP > 0)
        GNN_LAUNCH("k_gb_tasks", k_gb_tasks, grid_for(w.GP), kBlock, s, w.bcnt, w.GP, n_pairs, n_layers, pt, w.gpc,
                   w.gp_stride);
    return scan_counts(w.gpc, w.gp_stride, 2, w.rbase, w.tbase, w.GP, w.sums, s);
}

}  // namespace
}  // namespace gnn

using namespace gnn;

extern "C" {

size_t gnn_graph_build_workspace_bytes(int64_t n_hits, int64_t n_events, const int32_t *layer_pairs, int32_t n_pairs,
                                       int32_t n_layers, int32_t n_phi_sectors)
{
    int64_t rb = 0;
    if (check_common("gnn_graph_build_workspace_bytes", n_hits, n_events, layer_pairs, n_pairs, n_layers,
                     n_phi_sectors, &rb))
        return 0;
    return carve_gb(nullptr, n_hits, n_events, n_layers, n_pairs, n_phi_sectors, rb).bytes;
}

int gnn_graph_build_sizes(const float *r, const float *phi, const float *z, const int32_t *layer, int64_t n_hits,
                          const int64_t *event_ptr, int64_t n_events, const int32_t *layer_pairs, int32_t n_pairs,
                          int32_t n_layers, int32_t n_phi_sectors, float phi_slope_max, float phi_slope_outer_max,
                          float z0_max, void *workspace, size_t workspace_bytes, gnn_graph_build_sizes_t *sizes_out,
                          int64_t *hit_ptr, int64_t *seg_ptr, void *stream)
{
    ProfChain chain_;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int64_t rb = 0;
    if (int rc = check_common("gnn_graph_build_sizes", n_hits, n_events, layer_pairs, n_pairs, n_layers, n_phi_sectors,
                              &rb))
        return rc;
    if ((n_hits > 0 && (!r || !phi || !z || !layer)) || !event_ptr || !sizes_out || !hit_ptr || !seg_ptr)
        return fail(GNN_ERR_BADARG, "gnn_graph_build_sizes: pointer missing");
    if (int rc = check_workspace(workspace, workspace_bytes,
                                 carve_gb(nullptr, n_hits, n_events, n_layers, n_pairs, n_phi_sectors, rb).bytes))
        return rc;
    GbWs w = carve_gb(align_ws(workspace), n_hits, n_events, n_layers, n_pairs, n_phi_sectors, rb);
    const PairTab pt = pair_tab(layer_pairs, n_pairs, phi_slope_max, phi_slope_outer_max);
    hipError_t err = hipMemsetAsync(sizes_out, 0, sizeof(gnn_graph_build_sizes_t), s);
    if (err == hipSuccess && rb > 0) err = hipMemsetAsync(w.rcnt, 0, (size_t)rb * 4, s);
    if (err != hipSuccess) return fail(-(int)err, "gnn_graph_build_sizes: memset failed: %s", hipGetErrorString(err));
    if (int rc = stage_gb("gnn_graph_build_sizes", w, pt, r, phi, z, layer, n_hits, event_ptr, n_events, n_pairs,
                          n_layers, n_phi_sectors, s))
        return rc;
    const int64_t task_bound = rb / kRows + w.GP;
    if (task_bound > 0) {
        const unsigned grid = (unsigned)min(task_bound, (int64_t)device_cus() * kTaskWgPerCu);
        GNN_LAUNCH("k_gb_count", k_gb_pairs<0>, grid, kRows, s, w.GP, n_pairs, n_layers, pt, z0_max, w.tbase, w.rbase,
                   w.bcnt, w.boff, w.lr, w.lphi, w.lz, w.rcnt, w.total, nullptr, nullptr, nullptr, nullptr, nullptr,
                   nullptr, nullptr);
    }
    if (int rc = scan_counts(w.rcnt, 0, 1, w.roff, nullptr, rb, w.sums, s)) return rc;
    GNN_LAUNCH("k_gb_final", k_gb_final, grid_for(w.G + 1), kBlock, s, w.G, n_pairs, n_layers, w.boff, w.rbase, w.tbase,
               w.roff, w.status, w.total, sizes_out, hit_ptr, seg_ptr);
    return 0;
}

int gnn_graph_build_fill(const int64_t *particle_id, int64_t n_hits, int64_t n_events, const int32_t *layer_pairs,
                         int32_t n_pairs, int32_t n_layers, int32_t n_phi_sectors, float phi_slope_max,
                         float phi_slope_outer_max, float z0_max, double scale_r, double scale_phi, double scale_z,
                         const gnn_graph_build_sizes_t *sizes, void *workspace, size_t workspace_bytes, float *X,
                         int32_t *src, int32_t *dst, float *y, int64_t *hit_index, void *stream)
{
    ProfChain chain_;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int64_t rb = 0;
    if (int rc = check_common("gnn_graph_build_fill", n_hits, n_events, layer_pairs, n_pairs, n_layers, n_phi_sectors,
                              &rb))
        return rc;
    if (!sizes || sizes->status != 0 || sizes->n_hits < 0 || sizes->n_hits > n_hits || sizes->n_segments < 0 ||
        sizes->n_segments >= kInt32End || sizes->n_graphs != n_events * n_phi_sectors)
        return fail(GNN_ERR_BADARG, "gnn_graph_build_fill: sizes missing, flagged or not from this input");
    if ((sizes->n_hits > 0 && (!X || !hit_index)) || (sizes->n_segments > 0 && (!src || !dst)))
        return fail(GNN_ERR_BADARG, "gnn_graph_build_fill: output pointer missing");
    if (int rc = check_scales("gnn_graph_build_fill", scale_r, scale_phi, scale_z)) return rc;
    if (int rc = check_workspace(workspace, workspace_bytes,
                                 carve_gb(nullptr, n_hits, n_events, n_layers, n_pairs, n_phi_sectors, rb).bytes))
        return rc;
    GbWs w = carve_gb(align_ws(workspace), n_hits, n_events, n_layers, n_pairs, n_phi_sectors, rb);
    const PairTab pt = pair_tab(layer_pairs, n_pairs, phi_slope_max, phi_slope_outer_max);
    if (sizes->n_hits > 0)
        GNN_LAUNCH("k_gb_features", k_gb_features, grid_for(sizes->n_hits), kBlock, s, sizes->n_hits, n_layers, w.hkey,
                   w.boff, w.bcnt, w.lrow, w.lr, w.lphi, w.lz, scale_r, scale_phi, scale_z, w.lout, X, hit_index);
    if (sizes->n_segments > 0 && sizes->n_tasks > 0) {
        const unsigned grid = (unsigned)min(sizes->n_tasks, (int64_t)device_cus() * kTaskWgPerCu);
        GNN_LAUNCH("k_gb_fill", k_gb_pairs<1>, grid, kRows, s, w.GP, n_pairs, n_layers, pt, z0_max, w.tbase, w.rbase,
                   w.bcnt, w.boff, w.lr, w.lphi, w.lz, nullptr, nullptr, w.roff, w.lout, w.lrow,
                   y ? particle_id : nullptr, src, dst, particle_id ? y : nullptr);
    }
    return 0;
}

size_t gnn_cut_study_workspace_bytes(int64_t n_hits, int64_t n_events, const int32_t *layer_pairs, int32_t n_pairs,
                                     int32_t n_layers, int32_t n_phi_sectors, int32_t n_slope_edges, int32_t n_z0_edges)
{
    int64_t rb = 0;
    if (check_common("gnn_cut_study_workspace_bytes", n_hits, n_events, layer_pairs, n_pairs, n_layers, n_phi_sectors,
                     &rb) ||
        check_study("gnn_cut_study_workspace_bytes", n_hits, n_slope_edges, n_z0_edges))
        return 0;
    return carve_gb(nullptr, n_hits, n_events, n_layers, n_pairs, n_phi_sectors, 0).bytes;   // no per-row counts
}

int gnn_cut_study(const float *r, const float *phi, const float *z, const int32_t *layer, const int64_t *particle_id,
                  int64_t n_hits, const int64_t *event_ptr, int64_t n_events, const int32_t *layer_pairs, int32_t n_pairs,
                  int32_t n_layers, int32_t n_phi_sectors, const float *phi_slope_edges, int32_t n_slope_edges,
                  const float *z0_edges, int32_t n_z0_edges, void *workspace, size_t workspace_bytes, int64_t *counts,
                  int64_t *status, void *stream)
{
    ProfChain chain_;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int64_t rb = 0;
    if (int rc = check_common("gnn_cut_study", n_hits, n_events, layer_pairs, n_pairs, n_layers, n_phi_sectors, &rb))
        return rc;
    if (int rc = check_study("gnn_cut_study", n_hits, n_slope_edges, n_z0_edges)) return rc;
    if ((n_hits > 0 && (!r || !phi || !z || !layer || !particle_id)) || !event_ptr || !phi_slope_edges || !z0_edges ||
        (n_pairs > 0 && !counts) || !status)
        return fail(GNN_ERR_BADARG, "gnn_cut_study: pointer missing");
    if (int rc = check_workspace(workspace, workspace_bytes,
                                 carve_gb(nullptr, n_hits, n_events, n_layers, n_pairs, n_phi_sectors, 0).bytes))
        return rc;
    GbWs w = carve_gb(align_ws(workspace), n_hits, n_events, n_layers, n_pairs, n_phi_sectors, 0);
    const PairTab pt = pair_tab(layer_pairs, n_pairs, 0.f, 0.f);
    const int64_t cells = ((int64_t)n_slope_edges + 1) * (n_z0_edges + 1);
    if (n_pairs > 0) {
        const hipError_t err = hipMemsetAsync(counts, 0, (size_t)n_pairs * 2 * cells * sizeof(int64_t), s);
        if (err != hipSuccess) return fail(-(int)err, "gnn_cut_study: memset failed: %s", hipGetErrorString(err));
    }
    if (int rc = stage_gb("gnn_cut_study", w, pt, r, phi, z, layer, n_hits, event_ptr, n_events, n_pairs, n_layers,
                          n_phi_sectors, s))
        return rc;
    const int64_t task_bound = rb / kRows + w.GP;
    if (n_hits > 0 && task_bound > 0) {
        const unsigned grid = (unsigned)min(task_bound, (int64_t)device_cus() * kTaskWgPerCu);
        const size_t lds = (size_t)(2 * cells + n_slope_edges + n_z0_edges) * 4;   // at most 40 KB beside the tiles
        GNN_LAUNCH_SH("k_cs_pairs", k_cs_pairs, grid, kRows, lds, s, w.GP, n_pairs, n_layers, pt, w.tbase, w.bcnt, w.boff, w.lr,
                   w.lphi, w.lz, w.lrow, particle_id, phi_slope_edges, n_slope_edges, z0_edges, n_z0_edges,
                   reinterpret_cast<unsigned long long *>(counts));
    }
    GNN_LAUNCH("k_cs_final", k_cs_final, 1, 1, s, w.status, status);
    return 0;
}

}  // extern "C"
