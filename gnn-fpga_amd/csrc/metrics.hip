// metrics.hip - scoring a segment classifier on the GPU: confusion counts, score histograms, per-graph counts.
//
// The reference's notebooks (gnn/MPNN_Seg_ACTS*.ipynb: makeROC and the per-sample cells) read every score back and
// call sklearn.metrics accuracy_score / precision_score / recall_score on `pred > thresh` and roc_curve on the flat
// scores.  Here one pass over a batch adds into int64 counters the caller keeps on the device; gnn-fpga_amd/metrics.py
// turns them into those numbers and is, in segment_metrics_numpy, the specification of every counter.
//
//   k_metrics  persistent workgroups over tiles of kTile contiguous segments (16-B loads of e, y, src)
//     - totals and `e > t_k` counts per class: registers, then the wave, then LDS; one 64-bit add per counter and
//       workgroup at the end;
//     - histogram per class, key = float32 bits >> key_shift: the keys go into an LDS hash table (one slot per
//       distinct (key, class), a 32-bit count), which is emptied into the global histogram - one 64-bit add per
//       slot - when it is a quarter full and at the end.  Keys that many lanes of a wave share are merged in the
//       wave first (kPeel rounds of ballot), so LDS adds on one slot do not serialize either;
//     - per-graph counts (seg_ptr given): for every graph the tile touches, a block reduction of the tile's
//       segments in it and one 64-bit add per counter;
//     - the status word: any NaN / inf / score outside [0, 1], label other than 0 / 1, threshold not finite.
// Only integer atomics: the counters are the same bits in every run, whatever order the adds arrive in.
#include "common.h"

namespace gnn {
namespace {

constexpr int kMaxThr = 16;
constexpr int kCounters = 2 * (kMaxThr + 1);          // [T + 1][2]: totals, then `e > t_k`, per class
constexpr int kPer = 8;                               // segments per lane and tile (two 16-B loads per array)
constexpr int kTile = kBlock * kPer;                  // 2048
constexpr int kSlots = 4096;                          // LDS hash table: 32 KB (keys + counts)
constexpr unsigned kFlushAt = kSlots / 4;             // after a tile adds <= kTile slots: at most 75 % full
constexpr int64_t kMaxTilesPerFlush = 1 << 16;        // a slot's 32-bit count stays below 2^27
constexpr int kPeel = 2;
constexpr int kWgPerCu = 4;
constexpr unsigned kEmpty = 0xFFFFFFFFu;
constexpr int kStatusScore = 1, kStatusLabel = 2, kStatusThreshold = 4;

struct Thr {
    float t[kMaxThr];
};

__device__ __forceinline__ unsigned slot_of(unsigned k) { return (k * 2654435761u) >> (32 - 12); }
static_assert(kSlots == 1 << 12, "slot_of gives 12 bits");

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v)
{
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

__device__ __forceinline__ unsigned wave_sum32(unsigned v)
{
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// c[0..nc) of every lane summed over the workgroup, then out[i] += sum (64-bit, one add per counter, zero skipped)
template <typename V>
__device__ __forceinline__ void block_add(const V (&c)[kCounters], int nc, unsigned long long (*red)[kCounters],
                                          unsigned long long *out)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < kCounters; ++i) {
        if (i < nc) {
            const unsigned long long s = sizeof(V) == 4 ? (unsigned long long)wave_sum32((unsigned)c[i])
                                                        : wave_sum64((unsigned long long)c[i]);
            if (lane == 0) red[w][i] = s;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < nc) {
        unsigned long long s = 0;
#pragma unroll
        for (int k = 0; k < kBlock / 64; ++k) s += red[k][threadIdx.x];
        if (s) atomicAdd(out + threadIdx.x, s);
    }
    __syncthreads();
}

// count += c in the slot of key k (linear probing; the table never fills: see kFlushAt)
__device__ __forceinline__ void slot_add(unsigned *skey, unsigned *scnt, unsigned *occ, unsigned k, unsigned c)
{
    unsigned h = slot_of(k);
    for (;;) {
        const unsigned prev = atomicCAS(&skey[h], kEmpty, k);
        if (prev == kEmpty) atomicAdd(occ, 1u);
        if (prev == kEmpty || prev == k) {
            atomicAdd(&scnt[h], c);
            return;
        }
        h = (h + 1) & (kSlots - 1);
    }
}

template <bool VEC>
__device__ __forceinline__ void load_tile(const float *__restrict__ e, const float *__restrict__ y,
                                          const int32_t *__restrict__ src, int64_t tb, int64_t n, float (&ev)[kPer],
                                          float (&yv)[kPer], int (&sv)[kPer])
{
    // lane t holds tb + 4 t + c and tb + 1024 + 4 t + c (c = 0..3): each load instruction covers 1 KB of a wave
    if (VEC && tb + kTile <= n) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int64_t i = tb + j * (kTile / 2) + 4 * threadIdx.x;
            const float4 a = *reinterpret_cast<const float4 *>(e + i);
            const float4 b = *reinterpret_cast<const float4 *>(y + i);
            ev[4 * j] = a.x; ev[4 * j + 1] = a.y; ev[4 * j + 2] = a.z; ev[4 * j + 3] = a.w;
            yv[4 * j] = b.x; yv[4 * j + 1] = b.y; yv[4 * j + 2] = b.z; yv[4 * j + 3] = b.w;
            if (src) {
                const int4 s = *reinterpret_cast<const int4 *>(src + i);
                sv[4 * j] = s.x; sv[4 * j + 1] = s.y; sv[4 * j + 2] = s.z; sv[4 * j + 3] = s.w;
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) sv[4 * j + c] = 0;
            }
        }
    } else {
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const int64_t i = tb + (q >> 2) * (kTile / 2) + 4 * threadIdx.x + (q & 3);
            const bool in = i < n;
            ev[q] = in ? e[i] : 0.0f;
            yv[q] = in ? y[i] : 0.0f;
            sv[q] = !in ? -1 : src ? src[i] : 0;        // past the end: skipped like a padded segment
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_metrics(const float *__restrict__ e, const float *__restrict__ y,
                                                    const int32_t *__restrict__ src, int64_t n, Thr th, int T,
                                                    int key_shift, int64_t n_bins,
                                                    unsigned long long *__restrict__ counts,
                                                    unsigned long long *__restrict__ hist,
                                                    const int64_t *__restrict__ seg_ptr, int64_t G,
                                                    unsigned long long *__restrict__ per_graph,
                                                    int32_t *__restrict__ status)
{
    __shared__ unsigned skey[kSlots], scnt[kSlots];
    __shared__ unsigned long long red[kBlock / 64][kCounters];
    __shared__ unsigned occ;
    __shared__ int64_t g_first;
    const int nc = 2 * (T + 1);
    for (int s = threadIdx.x; s < kSlots; s += kBlock) {
        skey[s] = kEmpty;
        scnt[s] = 0;
    }
    if (threadIdx.x == 0) occ = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        bool ok = true;
#pragma unroll
        for (int k = 0; k < kMaxThr; ++k) ok = ok && (k >= T || __builtin_isfinite(th.t[k]));
        if (!ok) atomicOr(status, kStatusThreshold);
    }
    __syncthreads();

    unsigned c0[kMaxThr + 1] = {}, c1[kMaxThr + 1] = {};   // [0] totals, [1 + k] e > t_k; class 0 / 1
    int bad = 0;
    const int64_t n_tiles = (n + kTile - 1) / kTile;
    int64_t since_flush = 0;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t tb = t * kTile;
        float ev[kPer], yv[kPer];
        int sv[kPer];
        load_tile<VEC>(e, y, src, tb, n, ev, yv, sv);
        unsigned pos = 0, neg = 0;                          // bit q: segment q of the lane counts, in class 1 / 0
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            if (sv[q] < 0) continue;
            const bool ok_e = ev[q] >= 0.0f && ev[q] <= 1.0f;             // false for NaN
            const bool is1 = yv[q] == 1.0f, is0 = yv[q] == 0.0f;
            bad |= (ok_e ? 0 : kStatusScore) | (is1 || is0 ? 0 : kStatusLabel);
            if (ok_e && is1) pos |= 1u << q;
            if (ok_e && is0) neg |= 1u << q;
        }
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const bool p = (pos >> q) & 1, m = (neg >> q) & 1;
            c1[0] += p;
            c0[0] += m;
#pragma unroll
            for (int k = 0; k < kMaxThr; ++k) {
                if (k < T) {
                    const bool gt = ev[q] > th.t[k];
                    c1[1 + k] += gt && p;
                    c0[1 + k] += gt && m;
                }
            }
        }

        // histogram: (key << 1 | class) into the LDS table
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const bool p = (pos >> q) & 1;
            bool have = p || ((neg >> q) & 1);
            const unsigned k = have ? (((__float_as_uint(ev[q]) & 0x7FFFFFFFu) >> key_shift) << 1 | (unsigned)p)
                                    : kEmpty;
#pragma unroll
            for (int r = 0; r < kPeel; ++r) {               // the first open lane's key, merged over the wave
                const unsigned long long open = __ballot(have);
                if (!open) break;
                const int leader = __ffsll((long long)open) - 1;
                const bool match = have && k == (unsigned)__shfl((int)k, leader, 64);
                const unsigned long long same = __ballot(match);
                if (match) {
                    if ((int)(threadIdx.x & 63) == leader) slot_add(skey, scnt, &occ, k, (unsigned)__popcll(same));
                    have = false;
                }
            }
            if (have) slot_add(skey, scnt, &occ, k, 1u);
        }

        if (per_graph) {                                    // graphs that meet [tb, tb + kTile)
            const int64_t te = min(tb + kTile, n);
            if (threadIdx.x == 0) {
                int64_t lo = 0, hi = G;                     // the largest g < G with seg_ptr[g] <= tb (0 if none)
                while (hi - lo > 1) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (seg_ptr[mid] <= tb) lo = mid; else hi = mid;
                }
                g_first = lo;
            }
            __syncthreads();
            for (int64_t g = g_first; g < G && seg_ptr[g] < te; ++g) {
                const int64_t a = max(seg_ptr[g], tb), b = min(seg_ptr[g + 1], te);
                if (a >= b) continue;                       // (uniform: every lane reads the same two words)
                unsigned pc[kCounters];
#pragma unroll
                for (int i = 0; i < kCounters; ++i) pc[i] = 0;
#pragma unroll
                for (int q = 0; q < kPer; ++q) {
                    const int64_t i = tb + (q >> 2) * (kTile / 2) + 4 * threadIdx.x + (q & 3);
                    const bool in = i >= a && i < b;
                    const bool p = in && ((pos >> q) & 1), m = in && ((neg >> q) & 1);
                    pc[0] += m;
                    pc[1] += p;
#pragma unroll
                    for (int k = 0; k < kMaxThr; ++k) {
                        if (k < T) {
                            const bool gt = ev[q] > th.t[k];
                            pc[2 + 2 * k] += gt && m;
                            pc[3 + 2 * k] += gt && p;
                        }
                    }
                }
                block_add(pc, nc, red, per_graph + g * nc);
            }
        }

        __syncthreads();                                    // the tile's inserts are in
        const unsigned o = occ;
        __syncthreads();                                    // every lane has read occ before the next tile adds to it
        const bool flush = o > kFlushAt || ++since_flush == kMaxTilesPerFlush;   // (the same in every lane)
        if (flush) {
            for (int s = threadIdx.x; s < kSlots; s += kBlock) {
                const unsigned k = skey[s];
                if (k != kEmpty) {
                    atomicAdd(hist + (int64_t)(k & 1) * n_bins + (k >> 1), (unsigned long long)scnt[s]);
                    skey[s] = kEmpty;
                    scnt[s] = 0;
                }
            }
            since_flush = 0;
            if (threadIdx.x == 0) occ = 0;
            __syncthreads();                                // the table is empty before the next tile's inserts
        }
    }
    for (int s = threadIdx.x; s < kSlots; s += kBlock) {
        const unsigned k = skey[s];
        if (k != kEmpty) atomicAdd(hist + (int64_t)(k & 1) * n_bins + (k >> 1), (unsigned long long)scnt[s]);
    }

    const unsigned long long bad_lanes = __ballot(bad != 0);
    if (bad_lanes) {
        int b = bad;
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) b |= __shfl_xor(b, s, 64);
        if ((threadIdx.x & 63) == 0) atomicOr(status, b);
    }
    unsigned long long fc[kCounters];
#pragma unroll
    for (int k = 0; k <= kMaxThr; ++k) {
        fc[2 * k] = c0[k];
        fc[2 * k + 1] = c1[k];
    }
    block_add(fc, nc, red, counts);
}

}  // namespace
}  // namespace gnn

using namespace gnn;

extern "C" {

int64_t gnn_metrics_bins(int32_t key_shift)
{
    if (key_shift < 10 || key_shift > 23) return 0;
    return (int64_t)(0x3F800000u >> key_shift) + 1;
}

size_t gnn_metrics_workspace_bytes(int64_t n, int32_t n_thresholds, int32_t key_shift, int64_t n_graphs)
{
    return 0;
}

int gnn_segment_metrics_update(const float *e, const float *y, const int32_t *src, int64_t n, const float *thresholds,
                               int32_t n_thresholds, int32_t key_shift, int64_t *counts, int64_t *hist,
                               const int64_t *seg_ptr, int64_t n_graphs, int64_t *per_graph, int32_t *status,
                               void *workspace, size_t workspace_bytes, void *stream)
{
    ProfChain chain_;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t n_bins = gnn_metrics_bins(key_shift);
    if (n < 0 || n_thresholds < 0 || n_thresholds > kMaxThr || n_bins == 0 || n_graphs < 0)
        return fail(GNN_ERR_BADARG, "gnn_segment_metrics_update: bad argument (n %lld, n_thresholds %d, key_shift %d, "
                    "n_graphs %lld)", (long long)n, n_thresholds, key_shift, (long long)n_graphs);
    if ((n > 0 && (!e || !y)) || (n_thresholds > 0 && !thresholds) || !counts || !hist || !status ||
        ((seg_ptr != nullptr) != (per_graph != nullptr)))
        return fail(GNN_ERR_BADARG, "gnn_segment_metrics_update: pointer missing");
    const size_t need = gnn_metrics_workspace_bytes(n, n_thresholds, key_shift, n_graphs);
    if (workspace_bytes < need || (need > 0 && !workspace))
        return fail(GNN_ERR_WORKSPACE, "workspace too small: need %zu bytes", need);
    Thr th = {};
    for (int k = 0; k < n_thresholds; ++k) th.t[k] = thresholds[k];
    if (per_graph && n_graphs > 0) {
        const hipError_t err = hipMemsetAsync(per_graph, 0, (size_t)n_graphs * 2 * (n_thresholds + 1) * 8, s);
        if (err != hipSuccess)
            return fail(-(int)err, "gnn_segment_metrics_update: memset failed: %s", hipGetErrorString(err));
    }
    const int64_t n_tiles = (n + kTile - 1) / kTile;
    const unsigned grid = (unsigned)max((int64_t)1, min(n_tiles, (int64_t)device_cus() * kWgPerCu));
    auto *c = reinterpret_cast<unsigned long long *>(counts);
    auto *h = reinterpret_cast<unsigned long long *>(hist);
    auto *pg = reinterpret_cast<unsigned long long *>(per_graph);
    const int64_t G = per_graph ? n_graphs : 0;
    const bool vec = ((reinterpret_cast<uintptr_t>(e) | reinterpret_cast<uintptr_t>(y) |
                       reinterpret_cast<uintptr_t>(src)) & 15) == 0;
    if (vec)
        GNN_LAUNCH("k_metrics", k_metrics<true>, grid, kBlock, s, e, y, src, n, th, n_thresholds, key_shift, n_bins, c,
                   h, seg_ptr, G, pg, status);
    else
        GNN_LAUNCH("k_metrics", k_metrics<false>, grid, kBlock, s, e, y, src, n, th, n_thresholds, key_shift, n_bins,
                   c, h, seg_ptr, G, pg, status);
    return 0;
}

}  // extern "C"
