// layer_census.hip - which layers follow which along the particles' paths, counted on the GPU.
//
// The reference groups the hits by (evtid, barcode), sorts each group by r and pairs up the adjacent layers
// (gnn/GraphConstructionDev.ipynb cells 16-17), then counts every ordered pair (cells 37-41); the counts decide
// `layer_pairs`.  gnn-fpga_amd/cut_study.py (count_layer_transitions_numpy) is the specification.
//
//   gnn_layer_census
//     k_lc_rows    one lane per row: its event (binary search of event_ptr), checks (layer range, NaN r, event_ptr)
//                  into the status word, the order-preserving 32-bit key of r, value = the row
//     sort         by r key (32 bits), then by particle_id (64 bits), then by event: three stable passes, least
//                  significant key first, so equal r within a particle stays in input-row order
//     k_lc_count   one lane per sorted position: it and its successor are one (event, particle)'s neighbours in r ->
//                  table[layer][next layer] += 1; the table is private to the workgroup in LDS (32-bit counters) for
//                  n_layers <= 64 and added to the int64 table once per workgroup; above that, global atomics
// Integer sums only: every run gives the same bits.
#include <cstring>

#include "common.h"

#include "builder_sort.h"

namespace gnn {
namespace {

constexpr int kLdsLayers = 64;                         // 64 x 64 32-bit counters: 16 KB
constexpr int kMaxLayers = 4096;
constexpr int kCountWgPerCu = 4;

struct LcWs {
    int32_t *status;
    u64 *ka, *kb;                                      // [n] each
    int32_t *va, *vb, *evt;                            // [n] each
    char *temp;
    size_t temp_bytes, bytes;
};

LcWs carve_lc(char *base, int64_t n)
{
    LcWs w;
    Carver c{base};
    w.status = c.take<int32_t>(64);
    w.ka = c.take<u64>(n);
    w.kb = c.take<u64>(n);
    w.va = c.take<int32_t>(n);
    w.vb = c.take<int32_t>(n);
    w.evt = c.take<int32_t>(n);
    w.temp_bytes = n > 0 ? sort_temp_bytes(n) : 0;
    w.temp = c.take<char>(w.temp_bytes);
    w.bytes = c.bytes();
    return w;
}

// float32 -> uint32 with the same order (-0 and +0 are one value, as they are to a sort by r)
__device__ __forceinline__ uint32_t order_key(float v)
{
    const uint32_t u = __float_as_uint(v == 0.f ? 0.f : v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(kBlock) void k_lc_rows(const float *__restrict__ r, const int32_t *__restrict__ layer,
                                                    int64_t n, const int64_t *__restrict__ ep, int64_t E, int L,
                                                    u64 *__restrict__ key, int32_t *__restrict__ val,
                                                    int32_t *__restrict__ evt, int32_t *__restrict__ status)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    check_event_ptr(ep, E, n, i, status);
    if (i >= n) return;
    const int64_t e = last_le(ep, E, i);
    const int l = layer[i];
    const float ri = r[i];
    if (l < 0 || l >= L) atomicOr(status, kStatusLayer);
    if (ri != ri) atomicOr(status, kStatusFinite);
    evt[i] = event_owns(ep, e, i) ? (int)e : -1;       // -1: a malformed event_ptr (flagged), the row is left out
    key[i] = order_key(ri);
    val[i] = (int)i;
}

// the next pass's key of every sorted position: particle_id (any one-to-one image groups the same) or event
template <int BY_EVENT>
__global__ __launch_bounds__(kBlock) void k_lc_key(int64_t n, const int32_t *__restrict__ val,
                                                   const int64_t *__restrict__ pid, const int32_t *__restrict__ evt,
                                                   u64 *__restrict__ key)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const int row = val[j];
    key[j] = BY_EVENT ? (u64)(evt[row] + 1) : (u64)pid[row];
}

template <int LDS>
__global__ __launch_bounds__(kBlock) void k_lc_count(int64_t n, int L, const int32_t *__restrict__ val,
                                                     const int32_t *__restrict__ layer,
                                                     const int64_t *__restrict__ pid, const int32_t *__restrict__ evt,
                                                     int has_skip, int64_t skip, unsigned long long *__restrict__ table)
{
    __shared__ unsigned int tab[LDS ? kLdsLayers * kLdsLayers : 1];
    if (LDS) {
        for (int k = threadIdx.x; k < L * L; k += kBlock) tab[k] = 0;
        __syncthreads();
    }
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j + 1 < n; j += stride) {
        const int a = val[j], b = val[j + 1];
        const int64_t id = pid[a];
        const int la = layer[a], lb = layer[b];
        if (evt[a] < 0 || evt[a] != evt[b] || id != pid[b] || (has_skip && id == skip)) continue;
        if (la < 0 || la >= L || lb < 0 || lb >= L) continue;      // flagged by k_lc_rows
        if (LDS) atomicAdd(&tab[la * L + lb], 1u);                 // fewer than 2^31 rows: 32 bits hold them
        else atomicAdd(table + (int64_t)la * L + lb, 1ull);
    }
    if (LDS) {
        __syncthreads();
        for (int k = threadIdx.x; k < L * L; k += kBlock)
            if (tab[k]) atomicAdd(table + k, (unsigned long long)tab[k]);
    }
}

__global__ void k_lc_final(const int32_t *__restrict__ status, int64_t *__restrict__ status_out)
{
    *status_out = *status;
}

int check_lc(const char *who, int64_t n_hits, int64_t n_events, int32_t n_layers)
{
    if (n_hits < 0 || n_events < 1 || n_layers < 1)
        return fail(GNN_ERR_BADARG, "%s: bad argument (n_hits %lld, n_events %lld, n_layers %d)", who,
                    (long long)n_hits, (long long)n_events, n_layers);
    if (n_hits >= kInt32End || n_events >= kInt32End - 1)
        return fail(GNN_ERR_UNSUPPORTED, "%s: sizes outside the int32 index range", who);
    if (n_layers > kMaxLayers) return fail(GNN_ERR_UNSUPPORTED, "%s: more than %d layers", who, kMaxLayers);
    return 0;
}

}  // namespace
}  // namespace gnn

using namespace gnn;

extern "C" {

size_t gnn_layer_census_workspace_bytes(int64_t n_hits, int64_t n_events, int32_t n_layers)
{
    if (check_lc("gnn_layer_census_workspace_bytes", n_hits, n_events, n_layers)) return 0;
    return carve_lc(nullptr, n_hits).bytes;
}

int gnn_layer_census(const float *r, const int32_t *layer, const int64_t *particle_id, int64_t n_hits,
                     const int64_t *event_ptr, int64_t n_events, int32_t n_layers, int32_t has_skip,
                     int64_t skip_particle_id, void *workspace, size_t workspace_bytes, int64_t *table, int64_t *status,
                     void *stream)
{
    ProfChain chain_;
    const char *who = "gnn_layer_census";
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = check_lc(who, n_hits, n_events, n_layers)) return rc;
    if ((n_hits > 0 && (!r || !layer || !particle_id)) || !event_ptr || !table || !status)
        return fail(GNN_ERR_BADARG, "%s: pointer missing", who);
    if (int rc = check_workspace(workspace, workspace_bytes, carve_lc(nullptr, n_hits).bytes)) return rc;
    LcWs w = carve_lc(align_ws(workspace), n_hits);
    const int64_t n = n_hits;
    const int L = n_layers;
    hipError_t err = hipMemsetAsync(w.status, 0, 256, s);
    if (err == hipSuccess) err = hipMemsetAsync(table, 0, (size_t)L * L * sizeof(int64_t), s);
    if (err != hipSuccess) return fail(-(int)err, "%s: memset failed: %s", who, hipGetErrorString(err));
    GNN_LAUNCH("k_lc_rows", k_lc_rows, max(grid_for(max(n, n_events)), 1u), kBlock, s, r, layer, n, event_ptr, n_events,
               L, w.ka, w.va, w.evt, w.status);
    if (n > 1) {
        // (event, particle_id, r, row) order: the least significant key first, every pass stable
        if (int rc = sort_pairs(who, "rows by r", w.temp, w.temp_bytes, w.ka, w.kb, w.va, w.vb, n, 32, s)) return rc;
        GNN_LAUNCH("k_lc_pidkey", k_lc_key<0>, grid_for(n), kBlock, s, n, w.vb, particle_id, w.evt, w.ka);
        if (int rc = sort_pairs(who, "rows by particle_id", w.temp, w.temp_bytes, w.ka, w.kb, w.vb, w.va, n, 64, s))
            return rc;
        if (n_events > 1) {
            GNN_LAUNCH("k_lc_evkey", k_lc_key<1>, grid_for(n), kBlock, s, n, w.va, particle_id, w.evt, w.ka);
            if (int rc = sort_pairs(who, "rows by event", w.temp, w.temp_bytes, w.ka, w.kb, w.va, w.vb, n,
                                    bits_for((u64)n_events), s))
                return rc;
        }
        const int32_t *order = n_events > 1 ? w.vb : w.va;
        const unsigned grid = min(grid_for(n - 1), (unsigned)(device_cus() * kCountWgPerCu));
        if (L <= kLdsLayers)
            GNN_LAUNCH("k_lc_count", k_lc_count<1>, grid, kBlock, s, n, L, order, layer, particle_id, w.evt, has_skip,
                       skip_particle_id, reinterpret_cast<unsigned long long *>(table));
        else
            GNN_LAUNCH("k_lc_count_global", k_lc_count<0>, grid, kBlock, s, n, L, order, layer, particle_id, w.evt,
                       has_skip, skip_particle_id, reinterpret_cast<unsigned long long *>(table));
    }
    GNN_LAUNCH("k_lc_final", k_lc_final, 1, 1, s, w.status, status);
    return 0;
}

}  // extern "C"
