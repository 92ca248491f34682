// toy_graphs.hip - the toy notebooks' graphs for gfx950, from sorted hits straight into the compressed adjacency of
// gcn.hip (row_cnt / row_idx / row_val [, col_*]): no dense [E, N, N] tensor, no read-back, one launch per builder.
//
//   k_toy_segments   gnn/GCN_Seg_Toy2D.ipynb cells 10-17 and 24: all T^2 (L - 1) layer-to-next-layer segments of an
//                    event, X = (x0, x1, r0, r1, slope), y, and the kernel-weighted segment adjacency (cell 12's triple
//                    loop is an index relation: segment (l, a, b) touches (l - 1, *, a) and (l + 1, b, *))
//   k_toy_hits       gnn/GCN_Toy2D.ipynb cells 8 and 17 with cell 4's calc_adjacency / norm_adjacency /
//                    kwnorm_adjacency: X = (x, r / r_max, seed), y0, and the hit adjacency, rows and columns
//
// A workgroup owns `epw` consecutive events (as many as fill its 256 threads, one thread per node) and so one
// contiguous stretch of every output.  A thread builds the list of its node in an LDS tile, compacting the "!= 0"
// entries as it goes; the workgroup then copies the tile out in linear order, so a wave's store covers 256 contiguous
// bytes of row_idx / row_val whatever the list width is.  X is written in linear order too.
//
// Arithmetic.  Segments: the slope is one fp32 subtract and one fp32 divide, the kernel argument -(ds ds) / c with
// c = float32(2 sigma^2) in the notebook's order, and expf is the one value that cannot equal numpy's bit for bit.
// (s_j - s_i)^2 = (s_i - s_j)^2 bit for bit: the column lists ARE the row lists.  Hits: fp64 as the cell writes it,
// entry by entry - a[i, j] and a[j, i] round differently and neither is mirrored; x0 and xn are a rounded product and
// a rounded sum, never an FMA: contraction is off for this file, by the pragma below and by the Makefile's flag for
// this unit.  (HIP's __dmul_rn / __dadd_rn do not help: they are plain * and + in a header compiled with contraction
// on, and fuse once inlined - the edge fixture of tests/golden/toy_graphs is what shows it.)  A column's entries are
// kept as a bit mask per hit, so the lists and the counts the normalisers need come from one evaluation of every
// entry.  The normalisers are table look-ups by an integer count (1 / c, 1 / sqrt(c), made by numpy on the host): no
// device division or square root enters a value.
#include "common.h"

#pragma clang fp contract(off)

namespace gnn {
namespace {

constexpr int kToyMaxTracks = 16;            // a hit's 2 T candidates are the bits of one 32-bit word
constexpr int kToyMaxNodes = 4096;           // gcn.hip's limit on the nodes of a graph
constexpr int kToyLdsMax = 160 * 1024;

inline int toy_epw(int nodes) { return nodes >= kBlock ? 1 : kBlock / nodes; }

// LDS bytes: per staged hit `hit_bytes` (position + label [+ mask]), per node `node_bytes`, and the list tile
inline size_t toy_lds(int epw, int hits, int hit_bytes, int nodes, int node_bytes, int W)
{
    return (size_t)epw * hits * hit_bytes + (size_t)epw * nodes * node_bytes + (size_t)kBlock * W * 8;
}

// the workgroup's tile of `rows` lists -> the lists' place in global memory, in linear order
__device__ __forceinline__ void tile_out(const int32_t *ti, const float *tv, int words, int32_t *__restrict__ idx,
                                         float *__restrict__ val, int64_t at)
{
    __syncthreads();
    for (int q = threadIdx.x; q < words; q += kBlock) {
        idx[at + q] = ti[q];
        val[at + q] = tv[q];
    }
    __syncthreads();
}

__global__ __launch_bounds__(kBlock) void k_toy_segments(const float *__restrict__ hx, const int32_t *__restrict__ hy,
                                                         const float *__restrict__ det_r, int64_t E, int L, int T,
                                                         int epw, int W, float c, float *__restrict__ X,
                                                         float *__restrict__ y, int32_t *__restrict__ cnt,
                                                         int32_t *__restrict__ idx, float *__restrict__ val)
{
    extern __shared__ __align__(16) unsigned char toy_smem[];
    const int LT = L * T, TT = T * T, S = TT * (L - 1);
    const int64_t e0 = (int64_t)blockIdx.x * epw;
    const int nev = (int)min((int64_t)epw, E - e0);
    const int rows = nev * S;
    float *sx = reinterpret_cast<float *>(toy_smem);             // [epw][LT] positions
    int32_t *sy = reinterpret_cast<int32_t *>(sx + epw * LT);    // [epw][LT] track labels
    float *ss = reinterpret_cast<float *>(sy + epw * LT);        // [epw][S] slopes
    int32_t *ti = reinterpret_cast<int32_t *>(ss + epw * S);     // [kBlock][W] list tile
    float *tv = reinterpret_cast<float *>(ti + kBlock * W);
    const int tid = threadIdx.x;

    for (int q = tid; q < nev * LT; q += kBlock) {
        sx[q] = hx[e0 * LT + q];
        sy[q] = hy[e0 * LT + q];
    }
    __syncthreads();
    for (int rr = tid; rr < rows; rr += kBlock) {
        const int ev = rr / S, s = rr - ev * S;
        const int l = s / TT, ab = s - l * TT, a = ab / T, b = ab - a * T;
        const int h0 = ev * LT + l * T + a, h1 = ev * LT + (l + 1) * T + b;
        ss[rr] = (sx[h1] - sx[h0]) / (det_r[l + 1] - det_r[l]);
        y[e0 * S + rr] = sy[h0] == sy[h1] ? 1.0f : 0.0f;
    }
    __syncthreads();
    for (int q = tid; q < rows * 5; q += kBlock) {
        const int rr = q / 5, k = q - rr * 5;
        const int ev = rr / S, s = rr - ev * S;
        const int l = s / TT, ab = s - l * TT, a = ab / T, b = ab - a * T;
        float v;
        if (k == 0) v = sx[ev * LT + l * T + a];
        else if (k == 1) v = sx[ev * LT + (l + 1) * T + b];
        else if (k == 2) v = det_r[l];
        else if (k == 3) v = det_r[l + 1];
        else v = ss[rr];
        X[e0 * S * 5 + q] = v;
    }
    for (int r0 = 0; r0 < rows; r0 += kBlock) {
        const int rr = r0 + tid;
        if (rr < rows) {
            const int ev = rr / S, s = rr - ev * S;
            const int l = s / TT, ab = s - l * TT, a = ab / T, b = ab - a * T;
            const float *se = ss + ev * S;
            const float si = se[s];
            int32_t *li = ti + tid * W;
            float *lv = tv + tid * W;
            int k = 0;
            auto entry = [&](int j) {
                const float d = se[j] - si;
                const float v = expf(-(d * d) / c);
                if (v != 0.0f && k < W) {
                    li[k] = j;
                    lv[k] = v;
                    ++k;
                }
            };
            if (l > 0)                                           // the segments that end where this one starts
                for (int t = 0; t < T; ++t) entry(((l - 1) * T + t) * T + a);
            if (l < L - 2)                                       // the segments that start where this one ends
                for (int t = 0; t < T; ++t) entry(((l + 1) * T + b) * T + t);
            cnt[e0 * S + rr] = k;
            for (; k < W; ++k) {
                li[k] = 0;
                lv[k] = 0.0f;
            }
        }
        tile_out(ti, tv, min(kBlock, rows - r0) * W, idx, val, (e0 * S + r0) * W);
    }
}

// norm: 0 binary, 1 norm_adjacency (tab[c] = 1 / c, tab[0] = 0), 2 kwnorm_adjacency (tab[c] = 1 / sqrt(c))
__global__ __launch_bounds__(kBlock) void k_toy_hits(const double *__restrict__ hx, const int32_t *__restrict__ hy,
                                                     const double *__restrict__ det_r, const float *__restrict__ r_norm,
                                                     const double *__restrict__ tab, int64_t E, int L, int T, int epw,
                                                     int W, int seed_size, int norm, int target, float *__restrict__ X,
                                                     float *__restrict__ y0, int32_t *__restrict__ row_cnt,
                                                     int32_t *__restrict__ row_idx, float *__restrict__ row_val,
                                                     int32_t *__restrict__ col_cnt, int32_t *__restrict__ col_idx,
                                                     float *__restrict__ col_val, unsigned long long *__restrict__ n_iso)
{
    extern __shared__ __align__(16) unsigned char toy_smem[];
    const int N = L * T;
    const int64_t e0 = (int64_t)blockIdx.x * epw;
    const int nev = (int)min((int64_t)epw, E - e0);
    const int rows = nev * N;
    double *sx = reinterpret_cast<double *>(toy_smem);           // [epw][N] positions
    int32_t *sy = reinterpret_cast<int32_t *>(sx + epw * N);     // [epw][N] track labels
    uint32_t *sm = reinterpret_cast<uint32_t *>(sy + epw * N);   // [epw][N] column masks: bit t = a[(l - 1, t), i],
    int32_t *ti = reinterpret_cast<int32_t *>(sm + epw * N);     //   bit T + t = a[(l + 1, t), i]
    float *tv = reinterpret_cast<float *>(ti + kBlock * W);
    const int tid = threadIdx.x;
    const double rn = det_r[L - 1];

    for (int q = tid; q < rows; q += kBlock) {
        sx[q] = hx[e0 * N + q];
        const int32_t t = hy[e0 * N + q];
        sy[q] = t;
        y0[e0 * N + q] = t == target ? 1.0f : 0.0f;
    }
    __syncthreads();
    for (int q = tid; q < rows * 3; q += kBlock) {
        const int rr = q / 3, k = q - rr * 3;
        const int l = (rr % N) / T;
        float v;
        if (k == 0) v = (float)sx[rr];
        else if (k == 1) v = r_norm[l];
        else v = l < seed_size && sy[rr] == target ? 1.0f : 0.0f;
        X[e0 * N * 3 + q] = v;
    }
    // column i of the event's adjacency, entry by entry as calc_adjacency writes a[k, i]
    for (int r0 = 0; r0 < rows; r0 += kBlock) {
        const int rr = r0 + tid;
        bool isolated = false;
        if (rr < rows) {
            const int ev = rr / N, i = rr - ev * N, l = i / T;
            const double xi = sx[rr], ri = det_r[l];
            const double *xe = sx + ev * N;
            uint32_t mask = 0;
            for (int side = 0; side < 2; ++side) {
                const int lk = side ? l + 1 : l - 1;
                if (lk < 0 || lk >= L) continue;
                double dr = ri - det_r[lk];
                if (dr == 0.0) dr = 1e-7;
                for (int t = 0; t < T; ++t) {
                    const double slope = (xi - xe[lk * T + t]) / dr;
                    const double x0 = xi - slope * ri;           // (a rounded product, then a rounded sum)
                    const double xn = xi + slope * (rn - ri);
                    if (x0 < 1.0 && x0 > 0.0 && xn < 1.0 && xn > 0.0) mask |= 1u << (side * T + t);
                }
            }
            sm[rr] = mask;
            isolated = mask == 0;
        }
        const unsigned long long iso = __ballot(isolated);
        if ((tid & 63) == 0 && iso) atomicAdd(n_iso, (unsigned long long)__popcll(iso));
    }
    __syncthreads();
    for (int which = 0; which < 2; ++which) {                    // 0: the rows' lists, 1: the columns'
        int32_t *cnt = which ? col_cnt : row_cnt, *idx = which ? col_idx : row_idx;
        float *val = which ? col_val : row_val;
        for (int r0 = 0; r0 < rows; r0 += kBlock) {
            const int rr = r0 + tid;
            if (rr < rows) {
                const int ev = rr / N, h = rr - ev * N, l = h / T, p = h - l * T;
                const uint32_t *me = sm + ev * N;
                const uint32_t mh = me[h];
                int32_t *li = ti + tid * W;
                float *lv = tv + tid * W;
                int k = 0;
                // the entry between this hit and hit o: a[h, o] for a row list, a[o, h] for a column list
                auto entry = [&](int o, bool set) {
                    if (!set) return;
                    float v = 1.0f;
                    if (norm == 1) v = (float)tab[__popc(which ? me[o] : mh)];
                    else if (norm == 2) {
                        const double dh = tab[__popc(mh) + 1], d_o = tab[__popc(me[o]) + 1];
                        v = (float)(which ? d_o * dh : dh * d_o);
                    }
                    if (v != 0.0f && k < W) {
                        li[k] = o;
                        lv[k] = v;
                        ++k;
                    }
                };
                if (l > 0)
                    for (int t = 0; t < T; ++t) {
                        const int o = (l - 1) * T + t;
                        entry(o, which ? (mh >> t) & 1u : (me[o] >> (T + p)) & 1u);
                    }
                if (norm == 2) entry(h, true);                   // kwnorm_adjacency's identity
                if (l < L - 1)
                    for (int t = 0; t < T; ++t) {
                        const int o = (l + 1) * T + t;
                        entry(o, which ? (mh >> (T + t)) & 1u : (me[o] >> p) & 1u);
                    }
                cnt[e0 * N + rr] = k;
                for (; k < W; ++k) {
                    li[k] = 0;
                    lv[k] = 0.0f;
                }
            }
            tile_out(ti, tv, min(kBlock, rows - r0) * W, idx, val, (e0 * N + r0) * W);
        }
    }
}

int toy_shape_check(const char *who, int kind, int L, int T, int norm)
{
    if (kind != GNN_TOY_SEGMENTS && kind != GNN_TOY_HITS) return fail(GNN_ERR_BADARG, "%s: kind %d is unknown", who, kind);
    if (norm < GNN_TOY_NORM_NONE || norm > GNN_TOY_NORM_KW || (kind == GNN_TOY_SEGMENTS && norm != GNN_TOY_NORM_NONE))
        return fail(GNN_ERR_BADARG, "%s: norm %d is unknown", who, norm);
    if (L < 2) return fail(GNN_ERR_UNSUPPORTED, "%s: n_layers %d, the toy graphs need at least 2 detector layers", who, L);
    if (T < 1 || T > kToyMaxTracks)
        return fail(GNN_ERR_UNSUPPORTED, "%s: n_tracks %d, the kernels take 1 to %d tracks per event", who, T, kToyMaxTracks);
    const int64_t nodes = kind == GNN_TOY_SEGMENTS ? (int64_t)T * T * (L - 1) : (int64_t)L * T;
    if (nodes > kToyMaxNodes)
        return fail(GNN_ERR_UNSUPPORTED, "%s: %lld %s per event, the kernels take at most %d", who, (long long)nodes,
                    kind == GNN_TOY_SEGMENTS ? "segments" : "hits", kToyMaxNodes);
    return 0;
}

int toy_width(int kind, int L, int T, int norm)
{
    const int nodes = kind == GNN_TOY_SEGMENTS ? T * T * (L - 1) : L * T;
    return min(2 * T + (norm == GNN_TOY_NORM_KW ? 1 : 0), nodes);
}

}  // namespace
}  // namespace gnn

using namespace gnn;

extern "C" {

int32_t gnn_toy_graphs_list_width(int32_t kind, int32_t n_layers, int32_t n_tracks, int32_t norm)
{
    if (toy_shape_check("gnn_toy_graphs_list_width", kind, n_layers, n_tracks, norm)) return 0;
    return toy_width(kind, n_layers, n_tracks, norm);
}

int gnn_toy_segment_graphs(const float *hit_x, const int32_t *hit_y, const float *det_r, int64_t n_events,
                           int32_t n_layers, int32_t n_tracks, float two_sigma2, float *X, float *y, int32_t *row_cnt,
                           int32_t *row_idx, float *row_val, void *stream)
{
    static const char *who = "gnn_toy_segment_graphs";
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int L = n_layers, T = n_tracks;
    if (int rc = toy_shape_check(who, GNN_TOY_SEGMENTS, L, T, GNN_TOY_NORM_NONE)) return rc;
    if (n_events < 0 || n_events >= 0x7fffffffLL) return fail(GNN_ERR_BADARG, "%s: n_events negative or 2^31 and more", who);
    if (!(two_sigma2 > 0.0f) || two_sigma2 - two_sigma2 != 0.0f)
        return fail(GNN_ERR_BADARG, "%s: two_sigma2 must be positive and finite", who);
    if (!det_r) return fail(GNN_ERR_BADARG, "%s: pointer det_r missing", who);
    if (n_events == 0) return 0;
    if (!hit_x || !hit_y) return fail(GNN_ERR_BADARG, "%s: pointer hit_x or hit_y missing", who);
    if (!X || !y) return fail(GNN_ERR_BADARG, "%s: pointer X or y missing", who);
    if (!row_cnt || !row_idx || !row_val) return fail(GNN_ERR_BADARG, "%s: pointer row_cnt, row_idx or row_val missing", who);
    const int S = T * T * (L - 1), W = toy_width(GNN_TOY_SEGMENTS, L, T, 0), epw = toy_epw(S);
    const size_t lds = toy_lds(epw, L * T, 8, S, 4, W);
    static DevOnce attr_done;     // dynamic LDS above 64 KB must be opted into, once per device
    if (attr_done.need())
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_toy_segments),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, kToyLdsMax);
    GNN_LAUNCH_SH("k_toy_segments", k_toy_segments, (unsigned)((n_events + epw - 1) / epw), kBlock, lds, s, hit_x, hit_y,
                  det_r, n_events, L, T, epw, W, two_sigma2, X, y, row_cnt, row_idx, row_val);
    return 0;
}

int gnn_toy_hit_graphs(const double *hit_x, const int32_t *hit_y, const double *det_r, const float *r_norm,
                       const double *norm_table, int64_t n_events, int32_t n_layers, int32_t n_tracks,
                       int32_t seed_size, int32_t norm, int32_t target, float *X, float *y0, int32_t *row_cnt,
                       int32_t *row_idx, float *row_val, int32_t *col_cnt, int32_t *col_idx, float *col_val,
                       int64_t *n_isolated, void *stream)
{
    static const char *who = "gnn_toy_hit_graphs";
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int L = n_layers, T = n_tracks;
    if (int rc = toy_shape_check(who, GNN_TOY_HITS, L, T, norm)) return rc;
    if (n_events < 0 || n_events >= 0x7fffffffLL) return fail(GNN_ERR_BADARG, "%s: n_events negative or 2^31 and more", who);
    if (!n_isolated) return fail(GNN_ERR_BADARG, "%s: pointer n_isolated missing", who);
    if (!det_r || !r_norm) return fail(GNN_ERR_BADARG, "%s: pointer det_r or r_norm missing", who);
    if (norm != GNN_TOY_NORM_NONE && !norm_table) return fail(GNN_ERR_BADARG, "%s: pointer norm_table missing", who);
    const hipError_t err = hipMemsetAsync(n_isolated, 0, sizeof(int64_t), s);
    if (err != hipSuccess) return fail(-(int)err, "%s: memset failed: %s", who, hipGetErrorString(err));
    if (n_events == 0) return 0;
    if (!hit_x || !hit_y) return fail(GNN_ERR_BADARG, "%s: pointer hit_x or hit_y missing", who);
    if (!X || !y0) return fail(GNN_ERR_BADARG, "%s: pointer X or y0 missing", who);
    if (!row_cnt || !row_idx || !row_val) return fail(GNN_ERR_BADARG, "%s: pointer row_cnt, row_idx or row_val missing", who);
    if (!col_cnt || !col_idx || !col_val) return fail(GNN_ERR_BADARG, "%s: pointer col_cnt, col_idx or col_val missing", who);
    const int N = L * T, W = toy_width(GNN_TOY_HITS, L, T, norm), epw = toy_epw(N);
    const size_t lds = toy_lds(epw, N, 16, 0, 0, W);
    static DevOnce attr_done;
    if (attr_done.need())
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_toy_hits),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, kToyLdsMax);
    GNN_LAUNCH_SH("k_toy_hits", k_toy_hits, (unsigned)((n_events + epw - 1) / epw), kBlock, lds, s, hit_x, hit_y, det_r,
                  r_norm, norm_table, n_events, L, T, epw, W, seed_size, norm, target, X, y0, row_cnt, row_idx, row_val,
                  col_cnt, col_idx, col_val, reinterpret_cast<unsigned long long *>(n_isolated));
    return 0;
}

}  // extern "C"
