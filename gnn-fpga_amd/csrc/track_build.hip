// track_build.hip - track candidates from scored segments on the GPU: connected components of the kept segments,
// track numbering, the tracks' hit lists, and track-to-particle matching.
//
// The reference has no counterpart: it stops at one score per segment (Estimator.predict, gnn/estimator.py:137-146)
// and its notebooks only draw the scored segments (the draw_sample cells).  gnn-fpga_amd/tracks.py is the
// specification (build_tracks_numpy, match_tracks_numpy) of every array written here.
//
// Labels (gnn_track_build_labels), a device-wide union-find, one item per thread, nothing read back:
//   k_tb_init     parent[i] = i, sizes and best words cleared
//   k_tb_best     ("best" mode) per candidate segment a 64-bit atomicMax per end of (score key << 32 | ~segment id):
//                 a hit's best outgoing / incoming candidate, largest score, ties to the smallest id
//   k_tb_hook     per kept segment: find both roots, link the LARGER root to the SMALLER with an integer
//                 compare-and-swap; status bits (NaN score, endpoint out of range, kept segment across two graphs)
//   k_tb_flatten  per hit: chase to the root, store it, count the root's hits
//   k_tb_flag + the shared scan + k_tb_number   roots with >= min_hits hits numbered in ascending order of root
//   k_tb_sizes    the per-workgroup counts of kept segments and of hits in tracks added up
// Invariant of `parent`: parent[x] <= x at all times, and a word only ever changes from x (a root) to a smaller hit.
// So every chase strictly decreases and ends, a root is its tree's minimum, and the final root of a component is its
// smallest hit: the labels are defined by minima and maxima, not by which thread came first.  No thread waits for
// another one; only integer atomics touch global memory.
//
// Lists (gnn_track_build_lists) and matching (gnn_track_match) are stable radix sorts (builder_sort.h), run lengths
// and integer atomicMax votes: the same arrays in every run.
#include <cstring>

#pragma clang fp contract(off)
#include "builder_sort.h"

namespace gnn {
namespace {

constexpr int kTbNaN = 1, kTbCross = 2, kTbRange = 4;         // status bits (TB_STATUS_* in tracks.py)
constexpr int kSzTracks = 0, kSzTrackHits = 1, kSzKept = 2, kSzStatus = 3;   // words of sizes_out
constexpr unsigned kLow = 0xFFFFFFFFu;

__device__ __forceinline__ int64_t item() { return (int64_t)blockIdx.x * kBlock + threadIdx.x; }

// adds the number of lanes with `pred` to *ctr: one 64-bit add per wave (call it from every lane of the wave)
__device__ __forceinline__ void wave_count(bool pred, u64 *ctr)
{
    const u64 m = __ballot(pred);
    if (m && (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(ctr, (u64)__popcll(m));
}

// adds the workgroup's number of threads with `pred` to one of kSlots counters, a 64-byte line each, picked by the
// workgroup's index (every thread of the workgroup must call it): one word for a whole grid takes the adds of a
// 25.6 M-segment batch one after the other, 4.5 of k_tb_hook's 5.9 ms; k_tb_sizes adds the slots up
constexpr int kSlots = 256, kSlotStride = 8;
__device__ __forceinline__ void block_count(bool pred, u64 *slots)
{
    const int c = __syncthreads_count(pred);
    if (threadIdx.x == 0 && c) atomicAdd(slots + (size_t)(blockIdx.x & (kSlots - 1)) * kSlotStride, (u64)c);
}

__device__ __forceinline__ void wave_or(int bad, u64 *status)
{
    if (__ballot(bad != 0)) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) bad |= __shfl_xor(bad, s, 64);
        if ((threadIdx.x & 63) == 0) atomicOr(status, (u64)bad);
    }
}

// the graph of hit h (hit_ptr non-decreasing from 0; G >= 1)
__device__ __forceinline__ int64_t graph_of(const int64_t *hit_ptr, int64_t G, int64_t h)
{
    return G > 1 ? last_le(hit_ptr, G, h) : 0;
}

// Is segment j a candidate?  a, b: its hits.  src < 0 is a padded segment: skipped whatever its score.
__device__ __forceinline__ bool candidate(const int32_t *__restrict__ src, const int32_t *__restrict__ dst,
                                          const float *__restrict__ scores, int64_t j, int64_t n_hits, float thr, int &a,
                                          int &b, int &bad)
{
    a = src[j];
    b = dst[j];
    if (a < 0) return false;
    const float e = scores[j];
    if (e != e) bad |= kTbNaN;
    if (a >= n_hits || b < 0 || b >= n_hits) {
        bad |= kTbRange;
        return false;
    }
    return a != b && e > thr;                          // strict; false for NaN
}

// order-preserving key of a score: e1 < e2 <=> key(e1) < key(e2), -0 and +0 the same key
__device__ __forceinline__ unsigned score_key(float e)
{
    const unsigned u = e == 0.0f ? 0u : __float_as_uint(e);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(kBlock) void k_tb_init(int32_t *__restrict__ parent, int32_t *__restrict__ size,
                                                    u64 *__restrict__ best_out, u64 *__restrict__ best_in, int64_t n_hits)
{
    const int64_t i = item();
    if (i >= n_hits) return;
    parent[i] = (int32_t)i;
    size[i] = 0;
    best_out[i] = 0;
    best_in[i] = 0;
}

__global__ __launch_bounds__(kBlock) void k_tb_best(const int32_t *__restrict__ src, const int32_t *__restrict__ dst,
                                                    const float *__restrict__ scores, int64_t n_segments, int64_t n_hits,
                                                    float thr, u64 *__restrict__ best_out, u64 *__restrict__ best_in)
{
    const int64_t j = item();
    if (j >= n_segments) return;
    int a, b, bad = 0;
    if (!candidate(src, dst, scores, j, n_hits, thr, a, b, bad)) return;
    const u64 pack = ((u64)score_key(scores[j]) << 32) | (u64)(kLow - (unsigned)j);   // never 0: j < 2^31
    atomicMax(best_out + a, pack);
    atomicMax(best_in + b, pack);
}

__device__ __forceinline__ int tb_parent(const int32_t *parent, int x)
{
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int tb_find(const int32_t *parent, int x)
{
    // bounded: parent[x] <= x always, so every step that does not return lowers x: at most x steps
    for (;;) {
        const int p = tb_parent(parent, x);
        if (p == x) return x;
        x = p;
    }
}

template <bool BEST>
__global__ __launch_bounds__(kBlock) void k_tb_hook(const int32_t *__restrict__ src, const int32_t *__restrict__ dst,
                                                    const float *__restrict__ scores, int64_t n_segments, int64_t n_hits,
                                                    float thr, const u64 *__restrict__ best_out,
                                                    const u64 *__restrict__ best_in, const int64_t *__restrict__ hit_ptr,
                                                    int64_t G, int32_t *parent, u64 *__restrict__ sizes,
                                                    u64 *__restrict__ kept_slots)
{
    const int64_t j = item();
    int a = 0, b = 0, bad = 0;
    bool kept = j < n_segments && candidate(src, dst, scores, j, n_hits, thr, a, b, bad);
    if (BEST && kept) {
        const unsigned inv = kLow - (unsigned)j;
        kept = (unsigned)best_out[a] == inv && (unsigned)best_in[b] == inv;
    }
    if (kept && G > 1) {
        const int64_t g = last_le(hit_ptr, G, (int64_t)a);
        if (!(hit_ptr[g] <= b && b < hit_ptr[g + 1])) bad |= kTbCross;
    }
    if (kept) {
        int ra = tb_find(parent, a), rb = tb_find(parent, b);
        // bounded: a retry follows only a compare-and-swap that lost to a write which lowered parent[hi]; the new
        // pair of roots is (<= old parent[hi] < hi, <= lo), so ra + rb falls with every retry
        while (ra != rb) {
            const int hi = max(ra, rb), lo = min(ra, rb);
            const int old = atomicCAS(parent + hi, hi, lo);
            if (old == hi) break;
            ra = tb_find(parent, old);
            rb = tb_find(parent, lo);
        }
    }
    block_count(kept, kept_slots);
    wave_or(bad, sizes + kSzStatus);
}

__global__ __launch_bounds__(kBlock) void k_tb_flatten(const int32_t *__restrict__ parent, int64_t n_hits,
                                                       int32_t *__restrict__ root, int32_t *__restrict__ size)
{
    const int64_t i = item();
    if (i >= n_hits) return;
    const int r = tb_find(parent, (int)i);
    root[i] = r;
    atomicAdd(size + r, 1);
}

__global__ __launch_bounds__(kBlock) void k_tb_flag(const int32_t *__restrict__ root, const int32_t *__restrict__ size,
                                                    int64_t n_hits, int32_t min_hits, int32_t *__restrict__ flag)
{
    const int64_t i = item();
    if (i >= n_hits) return;
    flag[i] = root[i] == i && size[i] >= min_hits;
}

__global__ __launch_bounds__(kBlock) void k_tb_number(const int32_t *__restrict__ root, const int32_t *__restrict__ flag,
                                                      const int32_t *__restrict__ tptr, int64_t n_hits,
                                                      int32_t *__restrict__ track_of_hit, u64 *__restrict__ sizes,
                                                      u64 *__restrict__ hit_slots)
{
    const int64_t i = item();
    bool in = false;
    if (i < n_hits) {
        const int r = root[i];
        in = flag[r] != 0;
        track_of_hit[i] = in ? tptr[r] : -1;
    }
    if (i == 0) sizes[kSzTracks] = (u64)tptr[n_hits];
    block_count(in, hit_slots);
}

// one workgroup of kSlots threads: the slots of block_count into the sizes
__global__ __launch_bounds__(kSlots) void k_tb_sizes(const u64 *__restrict__ kept_slots, const u64 *__restrict__ hit_slots,
                                                     u64 *__restrict__ sizes)
{
    const u64 k = kept_slots[threadIdx.x * kSlotStride], h = hit_slots[threadIdx.x * kSlotStride];
    if (k) atomicAdd(sizes + kSzKept, k);
    if (h) atomicAdd(sizes + kSzTrackHits, h);
}

// ---- lists ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_tb_list_count(const int32_t *__restrict__ flag, const int32_t *__restrict__ tptr,
                                                          const int32_t *__restrict__ size,
                                                          const int64_t *__restrict__ hit_ptr, int64_t G, int64_t n_hits,
                                                          int64_t n_tracks, int32_t *__restrict__ cnt,
                                                          int32_t *__restrict__ track_graph)
{
    const int64_t i = item();
    if (i >= n_hits || !flag[i]) return;
    const int64_t t = tptr[i];
    if (t >= n_tracks) return;                         // (sizes that are not this workspace's)
    cnt[t] = size[i];
    track_graph[t] = (int32_t)graph_of(hit_ptr, G, i);
}

__global__ __launch_bounds__(kBlock) void k_tb_list_graphs(const int64_t *__restrict__ hit_ptr, int64_t G, int64_t n_hits,
                                                           const int32_t *__restrict__ tptr,
                                                           int32_t *__restrict__ graph_track_ptr)
{
    const int64_t g = item();
    if (g > G) return;
    const int64_t h = min(max(hit_ptr[g], (int64_t)0), n_hits);
    graph_track_ptr[g] = tptr[h];                      // roots below the graph's first hit
}

__global__ __launch_bounds__(kBlock) void k_tb_list_keys(const int32_t *__restrict__ track_of_hit, int64_t n_hits,
                                                         int64_t n_tracks, u64 *__restrict__ key, int32_t *__restrict__ val)
{
    const int64_t i = item();
    if (i >= n_hits) return;
    const int64_t t = track_of_hit[i];
    key[i] = (u64)(t >= 0 && t < n_tracks ? t : n_tracks);      // hits of no track sort last
    val[i] = (int32_t)i;
}

__global__ __launch_bounds__(kBlock) void k_tb_list_copy(const int32_t *__restrict__ sorted, int64_t n,
                                                         int32_t *__restrict__ track_hits)
{
    const int64_t p = item();
    if (p < n) track_hits[p] = sorted[p];
}

// ---- matching -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 pid_key(int64_t pid) { return pid > 0 ? (u64)pid : 0; }        // 0: no particle

__global__ __launch_bounds__(kBlock) void k_tb_match_keys(const int64_t *__restrict__ pid, int64_t n_hits,
                                                          u64 *__restrict__ key, int32_t *__restrict__ val)
{
    const int64_t i = item();
    if (i >= n_hits) return;
    key[i] = pid_key(pid[i]);
    val[i] = (int32_t)i;
}

__global__ __launch_bounds__(kBlock) void k_tb_match_graph_keys(const int32_t *__restrict__ hit, int64_t n_hits,
                                                                const int64_t *__restrict__ hit_ptr, int64_t G,
                                                                u64 *__restrict__ key)
{
    const int64_t p = item();
    if (p < n_hits) key[p] = (u64)graph_of(hit_ptr, G, hit[p]);
}

// order: the hits sorted by (graph, particle key), ascending hit id within a run; flag = 1 where a run starts
__global__ __launch_bounds__(kBlock) void k_tb_match_run_flag(const int32_t *__restrict__ order,
                                                              const int64_t *__restrict__ pid, int64_t n_hits,
                                                              const int64_t *__restrict__ hit_ptr, int64_t G,
                                                              int32_t *__restrict__ flag)
{
    const int64_t p = item();
    if (p >= n_hits) return;
    if (p == 0) {
        flag[0] = 1;
        return;
    }
    const int h = order[p], h0 = order[p - 1];
    flag[p] = pid_key(pid[h]) != pid_key(pid[h0]) || graph_of(hit_ptr, G, h) != graph_of(hit_ptr, G, h0);
}

// ridx: exclusive scan of flag ([n_hits] = the number of runs); run r starts at position run_start[r]
__global__ __launch_bounds__(kBlock) void k_tb_match_runs(const int32_t *__restrict__ order, const int32_t *__restrict__ flag,
                                                          const int32_t *__restrict__ ridx, int64_t n_hits,
                                                          int32_t *__restrict__ pidx, int32_t *__restrict__ run_start)
{
    const int64_t p = item();
    if (p >= n_hits) return;
    const int r = ridx[p] + flag[p] - 1;
    pidx[order[p]] = r;
    if (flag[p]) run_start[r] = (int32_t)p;
    if (p == n_hits - 1) run_start[ridx[n_hits]] = (int32_t)n_hits;
}

// counts[2]: particles (runs with an id > 0) with at least min_hits hits in their graph
__global__ __launch_bounds__(kBlock) void k_tb_match_particles(const int32_t *__restrict__ order,
                                                               const int64_t *__restrict__ pid,
                                                               const int32_t *__restrict__ ridx,
                                                               const int32_t *__restrict__ run_start, int64_t n_hits,
                                                               int32_t min_hits, u64 *__restrict__ counts)
{
    const int64_t r = item();
    bool ok = false;
    if (r < n_hits && r < ridx[n_hits]) {
        const int p0 = run_start[r];
        ok = pid[order[p0]] > 0 && run_start[r + 1] - p0 >= min_hits;
    }
    wave_count(ok, counts + 2);
}

__global__ __launch_bounds__(kBlock) void k_tb_match_keys2(const int32_t *__restrict__ track_of_hit,
                                                           const int32_t *__restrict__ pidx, int64_t n_hits,
                                                           int64_t n_tracks, u64 *__restrict__ key, int32_t *__restrict__ val)
{
    const int64_t i = item();
    if (i >= n_hits) return;
    const int64_t t = track_of_hit[i];
    key[i] = ((u64)(t >= 0 && t < n_tracks ? t : n_tracks) << 32) | (u64)(unsigned)pidx[i];
    val[i] = (int32_t)i;
}

// key: (track << 32 | particle index), sorted.  The first entry of every (track, particle) run votes its length:
// best[track] = max of (length << 32 | ~particle index) - the most hits, ties to the smaller index = the smaller id
__global__ __launch_bounds__(kBlock) void k_tb_match_vote(const u64 *__restrict__ key, int64_t n_hits, int64_t n_tracks,
                                                          const int32_t *__restrict__ order,
                                                          const int32_t *__restrict__ run_start,
                                                          const int64_t *__restrict__ pid, u64 *__restrict__ best)
{
    const int64_t p = item();
    if (p >= n_hits) return;
    const u64 k = key[p];
    const int64_t t = (int64_t)(k >> 32);
    if (t >= n_tracks || (p > 0 && key[p - 1] == k)) return;
    const unsigned r = (unsigned)k;
    if (pid[order[run_start[r]]] <= 0) return;         // the track's noise hits are no particle
    const int64_t len = lower_bound(key, n_hits, k + 1) - p;
    atomicMax(best + t, ((u64)len << 32) | (u64)(kLow - r));
}

__global__ __launch_bounds__(kBlock) void k_tb_match_final(const u64 *__restrict__ best, const int32_t *__restrict__ track_ptr,
                                                           int64_t n_tracks, const int32_t *__restrict__ order,
                                                           const int32_t *__restrict__ run_start,
                                                           const int64_t *__restrict__ pid, int32_t min_hits,
                                                           int64_t *__restrict__ majority_particle,
                                                           int32_t *__restrict__ majority_hits,
                                                           int32_t *__restrict__ particle_hits, int32_t *__restrict__ matched,
                                                           u64 *__restrict__ counts)
{
    const int64_t t = item();
    bool m = false, found = false;
    if (t < n_tracks) {
        const u64 b = best[t];
        int64_t id = 0, c = 0, ph = 0;
        if (b) {
            c = (int64_t)(b >> 32);
            const unsigned r = kLow - (unsigned)b;
            const int p0 = run_start[r];
            ph = run_start[r + 1] - p0;
            id = pid[order[p0]];
            const int64_t size = (int64_t)track_ptr[t + 1] - track_ptr[t];
            m = 2 * c > size && 2 * c > ph;
            found = m && ph >= min_hits;
        }
        majority_particle[t] = id;
        majority_hits[t] = (int32_t)c;
        particle_hits[t] = (int32_t)ph;
        matched[t] = m;
    }
    if (t == 0) counts[0] = (u64)n_tracks;
    wave_count(m, counts + 1);
    wave_count(found, counts + 3);
}

struct BuildWs {
    int32_t *parent, *size, *flag, *tptr, *cnt, *sums, *va, *vb;
    u64 *ka, *kb;                                      // best_out / best_in of the labels, the sort keys of the lists
    u64 *slots;                                        // block_count's counters: kept segments, then hits in tracks
    void *temp;
    size_t temp_bytes, bytes;
};

BuildWs carve_build(void *ws, int64_t n_hits)
{
    Carver c{ws ? align_ws(ws) : nullptr};
    const size_t n = (size_t)n_hits;
    BuildWs w;
    w.parent = c.take<int32_t>(n);
    w.size = c.take<int32_t>(n);
    w.flag = c.take<int32_t>(n);
    w.tptr = c.take<int32_t>(n + 1);
    w.cnt = c.take<int32_t>(n);
    w.sums = c.take<int32_t>((size_t)scan_sums_words(n_hits + 1));
    w.va = c.take<int32_t>(n);
    w.vb = c.take<int32_t>(n);
    w.ka = c.take<u64>(n);
    w.kb = c.take<u64>(n);
    w.slots = c.take<u64>((size_t)2 * kSlots * kSlotStride);
    w.temp_bytes = sort_temp_bytes(n_hits > 0 ? n_hits : 1);
    w.temp = c.take<char>(w.temp_bytes);
    w.bytes = c.bytes();
    return w;
}

struct MatchWs {
    int32_t *va, *vb, *order, *flag, *ridx, *run_start, *pidx, *sums;
    u64 *ka, *kb, *best;
    void *temp;
    size_t temp_bytes, bytes;
};

MatchWs carve_match(void *ws, int64_t n_hits, int64_t n_tracks)
{
    Carver c{ws ? align_ws(ws) : nullptr};
    const size_t n = (size_t)n_hits;
    MatchWs w;
    w.va = c.take<int32_t>(n);
    w.vb = c.take<int32_t>(n);
    w.order = c.take<int32_t>(n);
    w.flag = c.take<int32_t>(n);
    w.ridx = c.take<int32_t>(n + 1);
    w.run_start = c.take<int32_t>(n + 1);
    w.pidx = c.take<int32_t>(n);
    w.sums = c.take<int32_t>((size_t)scan_sums_words(n_hits + 1));
    w.ka = c.take<u64>(n);
    w.kb = c.take<u64>(n);
    w.best = c.take<u64>((size_t)n_tracks);
    w.temp_bytes = sort_temp_bytes(n_hits > 0 ? n_hits : 1);
    w.temp = c.take<char>(w.temp_bytes);
    w.bytes = c.bytes();
    return w;
}

bool int32_sizes(int64_t a, int64_t b) { return a >= 0 && b >= 0 && a < kInt32End && b < kInt32End; }

int memset_async(const char *who, void *p, size_t bytes, hipStream_t s)
{
    const hipError_t e = hipMemsetAsync(p, 0, bytes, s);
    if (e != hipSuccess) return fail(-(int)e, "%s: memset failed: %s", who, hipGetErrorString(e));
    return 0;
}

}  // namespace
}  // namespace gnn

using namespace gnn;

extern "C" {

size_t gnn_track_build_workspace_bytes(int64_t n_hits, int64_t n_segments)
{
    if (!int32_sizes(n_hits, n_segments)) {
        fail(GNN_ERR_BADARG, "gnn_track_build_workspace_bytes: n_hits / n_segments negative or 2^31 and more");
        return 0;
    }
    return carve_build(nullptr, n_hits).bytes;
}

int gnn_track_build_labels(const int32_t *src, const int32_t *dst, const float *scores, int64_t n_segments,
                           int64_t n_hits, const int64_t *hit_ptr, int64_t n_graphs, float threshold, int32_t mode,
                           int32_t min_hits, void *workspace, size_t workspace_bytes, int32_t *root,
                           int32_t *track_of_hit, int64_t *sizes_out, void *stream)
{
    static const char *who = "gnn_track_build_labels";
    ProfChain chain_;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!int32_sizes(n_hits, n_segments)) return fail(GNN_ERR_BADARG, "%s: n_hits / n_segments negative or 2^31 and more", who);
    if (n_graphs < 0 || n_graphs >= kInt32End) return fail(GNN_ERR_BADARG, "%s: n_graphs negative or 2^31 and more", who);
    if (!(threshold == threshold) || threshold - threshold != 0.0f) return fail(GNN_ERR_BADARG, "%s: threshold is not finite", who);
    if (mode != GNN_TRACKS_COMPONENTS && mode != GNN_TRACKS_BEST) return fail(GNN_ERR_BADARG, "%s: mode %d is unknown", who, mode);
    if (min_hits < 1) return fail(GNN_ERR_BADARG, "%s: min_hits %d < 1", who, min_hits);
    if (!sizes_out) return fail(GNN_ERR_BADARG, "%s: pointer sizes_out missing", who);
    if (n_segments > 0 && (!src || !dst || !scores)) return fail(GNN_ERR_BADARG, "%s: pointer src, dst or scores missing", who);
    if (n_hits > 0 && (!root || !track_of_hit)) return fail(GNN_ERR_BADARG, "%s: pointer root or track_of_hit missing", who);
    if (n_hits > 0 && (!hit_ptr || n_graphs < 1)) return fail(GNN_ERR_BADARG, "%s: hit_ptr missing or n_graphs < 1", who);
    const BuildWs need = carve_build(nullptr, n_hits);
    if (int rc = check_workspace(workspace, workspace_bytes, need.bytes)) return rc;
    const BuildWs w = carve_build(workspace, n_hits);
    if (int rc = memset_async(who, sizes_out, 4 * sizeof(int64_t), s)) return rc;
    if (int rc = memset_async(who, w.slots, (size_t)2 * kSlots * kSlotStride * sizeof(u64), s)) return rc;
    u64 *sizes = reinterpret_cast<u64 *>(sizes_out);
    u64 *kept_slots = w.slots, *hit_slots = w.slots + kSlots * kSlotStride;
    if (n_hits > 0) GNN_LAUNCH("k_tb_init", k_tb_init, grid_for(n_hits), kBlock, s, w.parent, w.size, w.ka, w.kb, n_hits);
    if (n_segments > 0) {
        const unsigned g = grid_for(n_segments);
        if (mode == GNN_TRACKS_BEST) {
            GNN_LAUNCH("k_tb_best", k_tb_best, g, kBlock, s, src, dst, scores, n_segments, n_hits, threshold, w.ka, w.kb);
            GNN_LAUNCH("k_tb_hook", k_tb_hook<true>, g, kBlock, s, src, dst, scores, n_segments, n_hits, threshold,
                       (const u64 *)w.ka, (const u64 *)w.kb, hit_ptr, n_graphs, w.parent, sizes, kept_slots);
        } else {
            GNN_LAUNCH("k_tb_hook", k_tb_hook<false>, g, kBlock, s, src, dst, scores, n_segments, n_hits, threshold,
                       (const u64 *)w.ka, (const u64 *)w.kb, hit_ptr, n_graphs, w.parent, sizes, kept_slots);
        }
    }
    if (n_hits > 0) {
        const unsigned g = grid_for(n_hits);
        GNN_LAUNCH("k_tb_flatten", k_tb_flatten, g, kBlock, s, (const int32_t *)w.parent, n_hits, root, w.size);
        GNN_LAUNCH("k_tb_flag", k_tb_flag, g, kBlock, s, (const int32_t *)root, (const int32_t *)w.size, n_hits, min_hits, w.flag);
        if (int rc = scan_counts(w.flag, 0, 1, w.tptr, nullptr, n_hits, w.sums, s)) return rc;
        GNN_LAUNCH("k_tb_number", k_tb_number, g, kBlock, s, (const int32_t *)root, (const int32_t *)w.flag,
                   (const int32_t *)w.tptr, n_hits, track_of_hit, sizes, hit_slots);
    }
    GNN_LAUNCH("k_tb_sizes", k_tb_sizes, 1, kSlots, s, (const u64 *)kept_slots, (const u64 *)hit_slots, sizes);
    return 0;
}

int gnn_track_build_lists(const int32_t *track_of_hit, int64_t n_hits, const int64_t *hit_ptr, int64_t n_graphs,
                          int64_t n_tracks, int64_t n_track_hits, void *workspace, size_t workspace_bytes,
                          int32_t *track_ptr, int32_t *track_hits, int32_t *track_graph, int32_t *graph_track_ptr,
                          void *stream)
{
    static const char *who = "gnn_track_build_lists";
    ProfChain chain_;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n_hits < 0 || n_hits >= kInt32End) return fail(GNN_ERR_BADARG, "%s: n_hits negative or 2^31 and more", who);
    if (n_graphs < 0 || n_graphs >= kInt32End) return fail(GNN_ERR_BADARG, "%s: n_graphs negative or 2^31 and more", who);
    if (n_tracks < 0 || n_tracks > n_hits) return fail(GNN_ERR_BADARG, "%s: n_tracks outside 0 .. n_hits", who);
    if (n_track_hits < n_tracks || n_track_hits > n_hits)
        return fail(GNN_ERR_BADARG, "%s: n_track_hits outside n_tracks .. n_hits", who);
    if (!track_ptr || !graph_track_ptr) return fail(GNN_ERR_BADARG, "%s: pointer track_ptr or graph_track_ptr missing", who);
    if (n_tracks > 0 && (!track_hits || !track_graph)) return fail(GNN_ERR_BADARG, "%s: pointer track_hits or track_graph missing", who);
    if (n_hits > 0 && (!track_of_hit || !hit_ptr || n_graphs < 1))
        return fail(GNN_ERR_BADARG, "%s: pointer track_of_hit or hit_ptr missing, or n_graphs < 1", who);
    const BuildWs need = carve_build(nullptr, n_hits);
    if (int rc = check_workspace(workspace, workspace_bytes, need.bytes)) return rc;
    const BuildWs w = carve_build(workspace, n_hits);
    if (n_hits == 0) {
        if (int rc = memset_async(who, track_ptr, sizeof(int32_t), s)) return rc;
        return memset_async(who, graph_track_ptr, (size_t)(n_graphs + 1) * sizeof(int32_t), s);
    }
    const unsigned g = grid_for(n_hits);
    GNN_LAUNCH("k_tb_list_graphs", k_tb_list_graphs, grid_for(n_graphs + 1), kBlock, s, hit_ptr, n_graphs, n_hits,
               (const int32_t *)w.tptr, graph_track_ptr);
    if (n_tracks > 0)
        GNN_LAUNCH("k_tb_list_count", k_tb_list_count, g, kBlock, s, (const int32_t *)w.flag, (const int32_t *)w.tptr,
                   (const int32_t *)w.size, hit_ptr, n_graphs, n_hits, n_tracks, w.cnt, track_graph);
    if (int rc = scan_counts(w.cnt, 0, 1, track_ptr, nullptr, n_tracks, w.sums, s)) return rc;
    if (n_tracks == 0) return 0;
    GNN_LAUNCH("k_tb_list_keys", k_tb_list_keys, g, kBlock, s, track_of_hit, n_hits, n_tracks, w.ka, w.va);
    if (int rc = sort_pairs(who, "of the hits by track", w.temp, w.temp_bytes, w.ka, w.kb, w.va, w.vb, n_hits,
                            bits_for((u64)n_tracks), s))
        return rc;
    GNN_LAUNCH("k_tb_list_copy", k_tb_list_copy, grid_for(n_track_hits), kBlock, s, (const int32_t *)w.vb, n_track_hits,
               track_hits);
    return 0;
}

size_t gnn_track_match_workspace_bytes(int64_t n_hits, int64_t n_tracks)
{
    if (n_hits < 0 || n_hits >= kInt32End || n_tracks < 0 || n_tracks > n_hits) {
        fail(GNN_ERR_BADARG, "gnn_track_match_workspace_bytes: n_hits negative or 2^31 and more, or n_tracks outside "
             "0 .. n_hits");
        return 0;
    }
    return carve_match(nullptr, n_hits, n_tracks).bytes;
}

int gnn_track_match(const int32_t *track_of_hit, const int64_t *particle_id, int64_t n_hits, const int64_t *hit_ptr,
                    int64_t n_graphs, const int32_t *track_ptr, int64_t n_tracks, int32_t min_hits, void *workspace,
                    size_t workspace_bytes, int64_t *majority_particle, int32_t *majority_hits, int32_t *particle_hits,
                    int32_t *matched, int64_t *counts, void *stream)
{
    static const char *who = "gnn_track_match";
    ProfChain chain_;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n_hits < 0 || n_hits >= kInt32End) return fail(GNN_ERR_BADARG, "%s: n_hits negative or 2^31 and more", who);
    if (n_graphs < 0 || n_graphs >= kInt32End) return fail(GNN_ERR_BADARG, "%s: n_graphs negative or 2^31 and more", who);
    if (n_tracks < 0 || n_tracks > n_hits) return fail(GNN_ERR_BADARG, "%s: n_tracks outside 0 .. n_hits", who);
    if (min_hits < 1) return fail(GNN_ERR_BADARG, "%s: min_hits %d < 1", who, min_hits);
    if (!counts) return fail(GNN_ERR_BADARG, "%s: pointer counts missing", who);
    if (n_hits > 0 && (!track_of_hit || !particle_id || !hit_ptr || n_graphs < 1))
        return fail(GNN_ERR_BADARG, "%s: pointer track_of_hit, particle_id or hit_ptr missing, or n_graphs < 1", who);
    if (n_tracks > 0 && (!track_ptr || !majority_particle || !majority_hits || !particle_hits || !matched))
        return fail(GNN_ERR_BADARG, "%s: pointer track_ptr or an output pointer missing", who);
    const MatchWs need = carve_match(nullptr, n_hits, n_tracks);
    if (int rc = check_workspace(workspace, workspace_bytes, need.bytes)) return rc;
    const MatchWs w = carve_match(workspace, n_hits, n_tracks);
    if (int rc = memset_async(who, counts, 4 * sizeof(int64_t), s)) return rc;
    if (n_hits == 0) return 0;
    u64 *cnt = reinterpret_cast<u64 *>(counts);
    const unsigned g = grid_for(n_hits);
    // (graph, particle id) -> dense particle index: a stable sort by id, then - several graphs - by graph
    GNN_LAUNCH("k_tb_match_keys", k_tb_match_keys, g, kBlock, s, particle_id, n_hits, w.ka, w.va);
    if (int rc = sort_pairs(who, "of the hits by particle id", w.temp, w.temp_bytes, w.ka, w.kb, w.va,
                            n_graphs > 1 ? w.vb : w.order, n_hits, 63, s))
        return rc;
    if (n_graphs > 1) {
        GNN_LAUNCH("k_tb_match_graph_keys", k_tb_match_graph_keys, g, kBlock, s, (const int32_t *)w.vb, n_hits, hit_ptr,
                   n_graphs, w.ka);
        if (int rc = sort_pairs(who, "of the hits by graph", w.temp, w.temp_bytes, w.ka, w.kb, w.vb, w.order, n_hits,
                                bits_for((u64)(n_graphs - 1)), s))
            return rc;
    }
    GNN_LAUNCH("k_tb_match_run_flag", k_tb_match_run_flag, g, kBlock, s, (const int32_t *)w.order, particle_id, n_hits,
               hit_ptr, n_graphs, w.flag);
    if (int rc = scan_counts(w.flag, 0, 1, w.ridx, nullptr, n_hits, w.sums, s)) return rc;
    GNN_LAUNCH("k_tb_match_runs", k_tb_match_runs, g, kBlock, s, (const int32_t *)w.order, (const int32_t *)w.flag,
               (const int32_t *)w.ridx, n_hits, w.pidx, w.run_start);
    GNN_LAUNCH("k_tb_match_particles", k_tb_match_particles, g, kBlock, s, (const int32_t *)w.order, particle_id,
               (const int32_t *)w.ridx, (const int32_t *)w.run_start, n_hits, min_hits, cnt);
    if (n_tracks == 0) return 0;
    // per track, the particle with the most hits: sort (track, particle index), vote the run lengths
    GNN_LAUNCH("k_tb_match_keys2", k_tb_match_keys2, g, kBlock, s, track_of_hit, (const int32_t *)w.pidx, n_hits, n_tracks,
               w.ka, w.va);
    if (int rc = sort_pairs(who, "of the hits by track and particle", w.temp, w.temp_bytes, w.ka, w.kb, w.va, w.vb,
                            n_hits, 32 + bits_for((u64)n_tracks), s))
        return rc;
    if (int rc = memset_async(who, w.best, (size_t)n_tracks * sizeof(u64), s)) return rc;
    GNN_LAUNCH("k_tb_match_vote", k_tb_match_vote, g, kBlock, s, (const u64 *)w.kb, n_hits, n_tracks,
               (const int32_t *)w.order, (const int32_t *)w.run_start, particle_id, w.best);
    GNN_LAUNCH("k_tb_match_final", k_tb_match_final, grid_for(n_tracks), kBlock, s, (const u64 *)w.best, track_ptr,
               n_tracks, (const int32_t *)w.order, (const int32_t *)w.run_start, particle_id, min_hits, majority_particle,
               majority_hits, particle_hits, matched, cnt);
    return 0;
}

}  // extern "C"
