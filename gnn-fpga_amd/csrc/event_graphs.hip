// event_graphs.hip - the ACTS full-event graphs from cluster hits on the GPU.
//
// The reference builds them on the host (gnn/MPNN_Seg_ACTS_fullEvents.ipynb): select_hits (cell 5) picks the barrel
// hits, renumbers the layers and deduplicates per (event, barcode, layer) in pandas; construct_graph (cell 8) tests
// every pair of hits of one event through three dense N x N masks, builds two dense N x E matrices and finds the
// labels with an int64 matmul against them; cells 16-18 loop over the events and drop those outside an occupancy
// window.  gnn-fpga_amd/event_graphs.py is the numpy specification of what is computed here; the window test is the
// reference's float32 arithmetic in its order of operations, with contraction to FMA off (the pragma).
//
//   gnn_event_graphs_sizes
//     k_eg_key       one lane per row: its event (binary search of event_ptr), barrel volume, layer, checks
//     radix sorts    by layer (8 bits), then barcode (64, biased), then event: all stable, so the rows stand in
//                    (event, barcode, layer, row) order; rows that are not barrel hits sort behind every event
//     k_eg_dedup     one lane per position: the first of a (event, barcode, layer) group walks it and keeps the hit
//                    of smallest r (the first row on ties); a scan of the flags numbers the kept hits: that number
//                    is the hit's position, event by event in (barcode, layer) order
//     k_eg_evstart   one lane per event: its first position (binary search of the sorted events)
//     k_eg_compact   row, event and layer of every kept hit by position; the bucket key (event, layer)
//     radix sort     by bucket key, stable: every (event, layer) bucket in position order
//     k_eg_stage     phi, z and barcode of every kept hit, SoA in bucket order; 1 where a task starts (a bucket's
//                    hits in blocks of 64); a scan numbers the tasks, k_eg_tstart lists them
//     k_eg_pairs     (count) one workgroup per task, one lane per start hit: the hits of the bucket one layer up
//                    through LDS tiles (every lane reads the same word: a broadcast), the window test, a count
//                    per start hit; events that fail a hit-count bound are not tested; a scan of the counts
//     k_eg_events    one lane per event: hits, segments, the occupancy test; scans -> graph number, hit and
//                    segment offsets of the kept events
//     k_eg_final     hit_ptr, seg_ptr, event_index of the kept events, the sizes and the status word
//   gnn_event_graphs_fill
//     k_eg_hits      X, hit_index, layer of every kept event's hits
//     k_eg_pairs     (fill) the same walk: every start hit writes src, dst, y from its scanned offset, end hits in
//                    position order: np.where order of the dense adjacency, start-hit-major
// Nothing is ordered by atomics (one integer total is summed by them): two builds of one input give the same bits.
#include <cstring>

#include "common.h"

#include <cmath>

#pragma clang fp contract(off)

#include "builder_sort.h"

namespace gnn {
namespace {

constexpr int kFB = 64;                                // start hits per task, one lane each (one wave)
constexpr int kTile = 512;                             // end hits per LDS tile
constexpr int kPairWgPerCu = 16;

struct EgWs {
    int32_t *status;                                   // head: [status | pad | total (u64) at byte 8]
    u64 *total;
    int32_t *evt, *lay, *gf, *gx, *best, *krow, *kevt, *klay, *ehit, *tf, *tx, *tstart, *cnt, *soff;
    int32_t *ev3, *ogr, *ohit, *oseg;                  // ev3: keep / hits / segments of the kept events, 3 x stride
    u64 *ka, *kb;
    int32_t *va, *vb;
    float *sphi, *sz;
    int64_t *sbc;
    int32_t *sums;
    void *temp;
    size_t temp_bytes;
    int64_t stride;
    size_t bytes;
};

EgWs carve_eg(char *base, int64_t n, int64_t E)
{
    EgWs w;
    Carver c{base};
    char *head = c.take<char>(256);
    w.status = reinterpret_cast<int32_t *>(head);
    w.total = head ? reinterpret_cast<u64 *>(head + 8) : nullptr;
    w.stride = (E + 64) & ~(int64_t)63;
    w.evt = c.take<int32_t>(n);
    w.lay = c.take<int32_t>(n);
    w.gf = c.take<int32_t>(n);
    w.gx = c.take<int32_t>(n + 1);
    w.best = c.take<int32_t>(n);
    w.krow = c.take<int32_t>(n);
    w.kevt = c.take<int32_t>(n);
    w.klay = c.take<int32_t>(n);
    w.ehit = c.take<int32_t>(E + 1);
    w.tf = c.take<int32_t>(n);
    w.tx = c.take<int32_t>(n + 1);
    w.tstart = c.take<int32_t>(n);
    w.cnt = c.take<int32_t>(n);
    w.soff = c.take<int32_t>(n + 1);
    w.ev3 = c.take<int32_t>(3 * w.stride);
    w.ogr = c.take<int32_t>(E + 1);
    w.ohit = c.take<int32_t>(E + 1);
    w.oseg = c.take<int32_t>(E + 1);
    w.ka = c.take<u64>(n);
    w.kb = c.take<u64>(n);
    w.va = c.take<int32_t>(n);
    w.vb = c.take<int32_t>(n);
    w.sphi = c.take<float>(n);
    w.sz = c.take<float>(n);
    w.sbc = c.take<int64_t>(n);
    w.sums = c.take<int32_t>(scan_sums_words(max(n, E)));
    w.temp_bytes = n > 0 ? sort_temp_bytes(n) : 0;
    w.temp = c.take<char>(w.temp_bytes);
    w.bytes = c.bytes();
    return w;
}

// cell 5: the barrel selection and the layer, int8(layid / 2 - 1 + 4 * volume) in float64, truncated toward zero
__global__ __launch_bounds__(kBlock) void k_eg_key(const float *__restrict__ r, const float *__restrict__ phi,
                                                   const float *__restrict__ z, const int32_t *__restrict__ volid,
                                                   const int32_t *__restrict__ layid, int64_t n,
                                                   const int64_t *__restrict__ ep, int64_t E,
                                                   int32_t *__restrict__ evt, int32_t *__restrict__ lay,
                                                   u64 *__restrict__ ka, int32_t *__restrict__ va,
                                                   int32_t *__restrict__ status)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    check_event_ptr(ep, E, n, i, status);
    if (i >= n) return;
    const int64_t lo = last_le(ep, E, i);              // the event
    int e = (int)lo, l = 0;
    const int v = volid[i];
    const int vol = v == 8 ? 0 : v == 13 ? 1 : v == 17 ? 2 : -1;
    if (!(isfinite(r[i]) && isfinite(phi[i]) && isfinite(z[i]))) {
        atomicOr(status, kStatusFinite);
        e = (int)E;                                    // in no event: never kept
    } else if (vol < 0) {
        e = (int)E;                                    // not a barrel hit
    } else {
        const double lf = trunc((double)layid[i] / 2.0 - 1.0 + (double)(4 * vol));
        if (lf < -128.0 || lf > 127.0) {
            atomicOr(status, kStatusLayer);
            e = (int)E;
        } else {
            l = (int)lf;
        }
    }
    if (e < E && !event_owns(ep, lo, i)) e = (int)E;   // (flagged above: event_ptr is malformed)
    evt[i] = e;
    lay[i] = l;
    ka[i] = (u64)(l + 128);                            // signed order
    va[i] = (int)i;
}

__global__ __launch_bounds__(kBlock) void k_eg_bckey(int64_t n, const int64_t *__restrict__ barcode,
                                                     const int32_t *__restrict__ rows, u64 *__restrict__ key)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) key[i] = (u64)barcode[rows[i]] ^ 0x8000000000000000ull;   // signed order
}

__global__ __launch_bounds__(kBlock) void k_eg_evkey(int64_t n, const int32_t *__restrict__ evt,
                                                     const int32_t *__restrict__ rows, u64 *__restrict__ key)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) key[i] = (u64)evt[rows[i]];
}

// rows: (event, barcode, layer, row) order.  The first position of a group keeps its hit of smallest r
__global__ __launch_bounds__(kBlock) void k_eg_dedup(int64_t n, int64_t E, const int32_t *__restrict__ rows,
                                                     const int32_t *__restrict__ evt, const int32_t *__restrict__ lay,
                                                     const int64_t *__restrict__ barcode, const float *__restrict__ r,
                                                     int32_t *__restrict__ gf, int32_t *__restrict__ best)
{
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const int a = rows[p];
    const int e = evt[a], l = lay[a];
    const int64_t b = barcode[a];
    int f = e < E;
    if (f && p > 0) {
        const int q = rows[p - 1];
        f = evt[q] != e || barcode[q] != b || lay[q] != l;
    }
    int row = a;
    if (f) {
        float rb = r[a];
        for (int64_t k = p + 1; k < n; ++k) {          // idxmin: the first in frame order on ties (rows ascend)
            const int q = rows[k];
            if (evt[q] != e || barcode[q] != b || lay[q] != l) break;
            if (r[q] < rb) {
                rb = r[q];
                row = q;
            }
        }
    }
    gf[p] = f;
    best[p] = row;
}

__global__ __launch_bounds__(kBlock) void k_eg_evstart(int64_t n, int64_t E, const u64 *__restrict__ sorted_evt,
                                                       const int32_t *__restrict__ gx, int32_t *__restrict__ ehit)
{
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e <= E) ehit[e] = gx[lower_bound(sorted_evt, n, (u64)e)];
}

// kept hits by position q; the slots behind them take the key of no bucket
__global__ __launch_bounds__(kBlock) void k_eg_compact(int64_t n, int64_t E, const int32_t *__restrict__ gf,
                                                       const int32_t *__restrict__ gx, const int32_t *__restrict__ best,
                                                       const int32_t *__restrict__ evt, const int32_t *__restrict__ lay,
                                                       int32_t *__restrict__ krow, int32_t *__restrict__ kevt,
                                                       int32_t *__restrict__ klay, u64 *__restrict__ key,
                                                       int32_t *__restrict__ val, int32_t *__restrict__ cnt)
{
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    cnt[p] = 0;
    if (gf[p]) {
        const int q = gx[p], row = best[p];
        krow[q] = row;
        kevt[q] = evt[row];
        klay[q] = lay[row];
        key[q] = ((u64)evt[row] << 8) | (u64)(lay[row] + 128);
        val[q] = q;
    } else {
        const int64_t q = (int64_t)gx[n] + (p - gx[p]);   // the p - gx[p]-th position that keeps nothing
        key[q] = (u64)E << 8;
        val[q] = (int)q;
    }
}

__global__ __launch_bounds__(kBlock) void k_eg_stage(int64_t n, const int32_t *__restrict__ gx,
                                                     const u64 *__restrict__ bkey, const int32_t *__restrict__ bq,
                                                     const int32_t *__restrict__ krow, const float *__restrict__ phi,
                                                     const float *__restrict__ z, const int64_t *__restrict__ barcode,
                                                     float *__restrict__ sphi, float *__restrict__ sz,
                                                     int64_t *__restrict__ sbc, int32_t *__restrict__ tf)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n) return;
    int f = 0;
    if (t < gx[n]) {
        const int row = krow[bq[t]];
        sphi[t] = phi[row];
        sz[t] = z[row];
        sbc[t] = barcode[row];
        f = (t - lower_bound(bkey, n, bkey[t])) % kFB == 0;
    }
    tf[t] = f;
}

__global__ __launch_bounds__(kBlock) void k_eg_tstart(int64_t n, const int32_t *__restrict__ tf,
                                                      const int32_t *__restrict__ tx, int32_t *__restrict__ tstart)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t < n && tf[t]) tstart[tx[t]] = (int)t;
}

// cell 8 for one (event, layer) bucket's block of start hits per task: each against every hit of the bucket one layer
// up, in position order.  FILL = false counts per start hit; FILL = true writes from the scanned offsets.
template <bool FILL>
__global__ __launch_bounds__(kFB) void k_eg_pairs(int64_t n, const int32_t *__restrict__ tx,
                                                  const int32_t *__restrict__ tstart, const u64 *__restrict__ bkey,
                                                  const int32_t *__restrict__ bq, const float *__restrict__ sphi,
                                                  const float *__restrict__ sz, const int64_t *__restrict__ sbc,
                                                  const int32_t *__restrict__ ehit, float dphi_max, float dz_max,
                                                  int64_t nodes_min, int64_t nodes_max, int32_t *__restrict__ cnt,
                                                  u64 *__restrict__ total, const int32_t *__restrict__ soff,
                                                  const int32_t *__restrict__ keep, const int32_t *__restrict__ ohit,
                                                  const int32_t *__restrict__ oseg, int32_t *__restrict__ src,
                                                  int32_t *__restrict__ dst, float *__restrict__ y)
{
    __shared__ float s_phi[kTile], s_z[kTile];
    __shared__ int32_t s_q[FILL ? kTile : 1];
    __shared__ int64_t s_bc[FILL ? kTile : 1];
    const int64_t n_tasks = tx[n];
    for (int64_t task = blockIdx.x; task < n_tasks; task += gridDim.x) {
        const int64_t t0 = tstart[task];
        const u64 key = bkey[t0];
        const int64_t e = (int64_t)(key >> 8);
        const int h0 = ehit[e], nh = ehit[e + 1] - h0;
        if (FILL ? !keep[e] : !(nh > nodes_min && nh < nodes_max)) continue;   // (their counts stay 0)
        const int64_t t = t0 + threadIdx.x;
        const bool valid = t < n && bkey[t] == key;
        int64_t p0 = 0, p1 = 0;
        if ((key & 255) != 255) {                      // layer 127 has no layer above it
            p0 = lower_bound(bkey, n, key + 1);
            p1 = lower_bound(bkey, n, key + 2);
        }
        float my_phi = 0.f, my_z = 0.f;
        int64_t my_bc = 0, o = 0;
        int q = 0, c = 0, my_pos = 0;
        if (valid) {
            my_phi = sphi[t];
            my_z = sz[t];
            q = bq[t];
            if (FILL) {
                my_bc = sbc[t];
                my_pos = ohit[e] + (q - h0);
                o = (int64_t)oseg[e] + (soff[q] - soff[h0]);
            }
        }
        const int64_t m = p1 - p0;
        for (int64_t m0 = 0; m0 < m; m0 += kTile) {
            const int mt = (int)min((int64_t)kTile, m - m0);
            __syncthreads();                           // the previous tile has been read
            for (int k = threadIdx.x; k < mt; k += kFB) {
                s_phi[k] = sphi[p0 + m0 + k];
                s_z[k] = sz[p0 + m0 + k];
                if (FILL) {
                    s_q[k] = bq[p0 + m0 + k];
                    s_bc[k] = sbc[p0 + m0 + k];
                }
            }
            __syncthreads();
            if (valid) {
                for (int k = 0; k < mt; ++k) {
                    const float dphi = wrap_dphi(my_phi - s_phi[k]);   // cell 7: calc_dphi(phi[None, :], phi[:, None])
                    const float dz = s_z[k] - my_z;
                    if (fabsf(dphi) < dphi_max && fabsf(dz) < dz_max) {
                        if (FILL) {
                            src[o + c] = my_pos;
                            dst[o + c] = ohit[e] + (s_q[k] - h0);
                            y[o + c] = s_bc[k] == my_bc ? 1.0f : 0.0f;
                        }
                        ++c;
                    }
                }
            }
        }
        if (!FILL) {
            if (valid) cnt[q] = c;
            u64 sum = (u64)c;                          // one wave per workgroup: its total in one atomic
            for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d, 64);
            if (threadIdx.x == 0 && sum) atomicAdd(total, sum);
        }
    }
}

// cells 16-18: an event without a kept hit is no graph; the occupancy test, all three strict
__global__ __launch_bounds__(kBlock) void k_eg_events(int64_t E, int64_t stride, const int32_t *__restrict__ ehit,
                                                      const int32_t *__restrict__ soff, int64_t nodes_min,
                                                      int64_t nodes_max, int64_t edges_max, int32_t *__restrict__ ev3)
{
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= E) return;
    const int64_t nh = ehit[e + 1] - ehit[e];
    const int64_t ns = (int64_t)soff[ehit[e + 1]] - soff[ehit[e]];
    const int k = nh > 0 && nh > nodes_min && nh < nodes_max && ns < edges_max;
    ev3[e] = k;
    ev3[stride + e] = k ? (int)nh : 0;
    ev3[2 * stride + e] = k ? (int)ns : 0;
}

__global__ __launch_bounds__(kBlock) void k_eg_final(int64_t n, int64_t E, const int32_t *__restrict__ ev3,
                                                     const int32_t *__restrict__ ogr, const int32_t *__restrict__ ohit,
                                                     const int32_t *__restrict__ oseg, const int32_t *__restrict__ gx,
                                                     const int32_t *__restrict__ tx, const int32_t *__restrict__ status,
                                                     const u64 *__restrict__ total, gnn_event_graphs_sizes_t *sizes,
                                                     int64_t *__restrict__ hit_ptr, int64_t *__restrict__ seg_ptr,
                                                     int64_t *__restrict__ event_index)
{
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e > E) return;
    if (e < E) {
        if (!ev3[e]) return;
        const int g = ogr[e];
        hit_ptr[g] = ohit[e];
        seg_ptr[g] = oseg[e];
        event_index[g] = e;
        return;
    }
    const int G = ogr[E];
    hit_ptr[G] = ohit[E];
    seg_ptr[G] = oseg[E];
    const bool ovf = *total >= (u64)kInt32End;
    sizes->n_graphs = G;
    sizes->n_hits = ovf ? 0 : ohit[E];
    sizes->n_segments = ovf ? 0 : oseg[E];
    sizes->n_kept = gx[n];
    sizes->n_tasks = tx[n];
    sizes->n_tested = (int64_t)*total;
    sizes->status = *status | (ovf ? kStatusInt32 : 0);
}

__global__ __launch_bounds__(kBlock) void k_eg_hits(int64_t n, const int32_t *__restrict__ gx,
                                                    const int32_t *__restrict__ krow, const int32_t *__restrict__ kevt,
                                                    const int32_t *__restrict__ klay, const int32_t *__restrict__ ehit,
                                                    const int32_t *__restrict__ keep, const int32_t *__restrict__ ohit,
                                                    const float *__restrict__ r, const float *__restrict__ phi,
                                                    const float *__restrict__ z, double sc_r, double sc_phi, double sc_z,
                                                    float *__restrict__ X, int64_t *__restrict__ hit_index,
                                                    int32_t *__restrict__ layer)
{
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= gx[n]) return;
    const int e = kevt[q];
    if (!keep[e]) return;
    const int64_t o = (int64_t)ohit[e] + (q - ehit[e]);
    const int row = krow[q];
    X[3 * o] = feature(r[row], sc_r);                  // cell 8: float32 columns / a float64 array, then float32
    X[3 * o + 1] = feature(phi[row], sc_phi);
    X[3 * o + 2] = feature(z[row], sc_z);
    hit_index[o] = row;
    layer[o] = klay[q];
}

int check_args(const char *who, int64_t n_rows, int64_t n_events)
{
    if (n_rows < 0 || n_events < 1)
        return fail(GNN_ERR_BADARG, "%s: bad argument (n_rows %lld, n_events %lld)", who, (long long)n_rows,
                    (long long)n_events);
    if (n_rows >= kInt32End - 1 || n_events >= kInt32End - 1)
        return fail(GNN_ERR_UNSUPPORTED, "%s: sizes outside the int32 index range", who);
    return 0;
}

int check_cuts(const char *who, float dphi_max, float dz_max)
{
    if (dphi_max != dphi_max || dz_max != dz_max) return fail(GNN_ERR_BADARG, "%s: dphi_max or dz_max is NaN", who);
    return 0;
}

}  // namespace
}  // namespace gnn

using namespace gnn;

extern "C" {

size_t gnn_event_graphs_workspace_bytes(int64_t n_rows, int64_t n_events)
{
    if (check_args("gnn_event_graphs_workspace_bytes", n_rows, n_events)) return 0;
    return carve_eg(nullptr, n_rows, n_events).bytes;
}

int gnn_event_graphs_sizes(const float *r, const float *phi, const float *z, const int32_t *volid, const int32_t *layid,
                           const int64_t *barcode, int64_t n_rows, const int64_t *event_ptr, int64_t n_events,
                           float dphi_max, float dz_max, int64_t n_nodes_min, int64_t n_nodes_max, int64_t n_edges_max,
                           void *workspace, size_t workspace_bytes, gnn_event_graphs_sizes_t *sizes_out,
                           int64_t *hit_ptr, int64_t *seg_ptr, int64_t *event_index, void *stream)
{
    ProfChain chain_;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = check_args("gnn_event_graphs_sizes", n_rows, n_events)) return rc;
    if (int rc = check_cuts("gnn_event_graphs_sizes", dphi_max, dz_max)) return rc;
    if ((n_rows > 0 && (!r || !phi || !z || !volid || !layid || !barcode)) || !event_ptr || !sizes_out || !hit_ptr ||
        !seg_ptr || !event_index)
        return fail(GNN_ERR_BADARG, "gnn_event_graphs_sizes: pointer missing");
    const int64_t n = n_rows, E = n_events;
    if (int rc = check_workspace(workspace, workspace_bytes, carve_eg(nullptr, n, E).bytes)) return rc;
    EgWs w = carve_eg(align_ws(workspace), n, E);
    hipError_t err = hipMemsetAsync(w.status, 0, 256, s);
    if (err == hipSuccess) err = hipMemsetAsync(sizes_out, 0, sizeof(gnn_event_graphs_sizes_t), s);
    if (err == hipSuccess) err = hipMemsetAsync(w.gx, 0, sizeof(int32_t), s);       // (n = 0: no scan writes them)
    if (err == hipSuccess) err = hipMemsetAsync(w.tx, 0, sizeof(int32_t), s);
    if (err == hipSuccess) err = hipMemsetAsync(w.soff, 0, sizeof(int32_t), s);
    if (err != hipSuccess) return fail(-(int)err, "gnn_event_graphs_sizes: memset failed: %s", hipGetErrorString(err));
    GNN_LAUNCH("k_eg_key", k_eg_key, max(grid_for(max(n, E)), 1u), kBlock, s, r, phi, z, volid, layid, n, event_ptr, E,
               w.evt, w.lay, w.ka, w.va, w.status);
    auto sort = [&](const char *what, const u64 *kin, u64 *kout, const int32_t *vin, int32_t *vout, int bits) {
        return sort_pairs("gnn_event_graphs_sizes", what, w.temp, w.temp_bytes, kin, kout, vin, vout, n, bits, s);
    };
    if (n > 0) {
        // (event, barcode, layer, row) order: the least significant key first, every sort stable
        if (int rc = sort("by layer", w.ka, w.kb, w.va, w.vb, 8)) return rc;
        GNN_LAUNCH("k_eg_bckey", k_eg_bckey, grid_for(n), kBlock, s, n, barcode, w.vb, w.ka);
        if (int rc = sort("by barcode", w.ka, w.kb, w.vb, w.va, 64)) return rc;
        GNN_LAUNCH("k_eg_evkey", k_eg_evkey, grid_for(n), kBlock, s, n, w.evt, w.va, w.ka);
        if (int rc = sort("by event", w.ka, w.kb, w.va, w.vb, bits_for((u64)E))) return rc;
        GNN_LAUNCH("k_eg_dedup", k_eg_dedup, grid_for(n), kBlock, s, n, E, w.vb, w.evt, w.lay, barcode, r, w.gf, w.best);
        if (int rc = scan_counts(w.gf, 0, 1, w.gx, nullptr, n, w.sums, s)) return rc;
    }
    GNN_LAUNCH("k_eg_evstart", k_eg_evstart, grid_for(E + 1), kBlock, s, n, E, w.kb, w.gx, w.ehit);
    if (n > 0) {
        GNN_LAUNCH("k_eg_compact", k_eg_compact, grid_for(n), kBlock, s, n, E, w.gf, w.gx, w.best, w.evt, w.lay, w.krow,
                   w.kevt, w.klay, w.ka, w.va, w.cnt);
        // every (event, layer) bucket in position order
        if (int rc = sort("by event and layer", w.ka, w.kb, w.va, w.vb, bits_for(((u64)E << 8) | 255))) return rc;
        GNN_LAUNCH("k_eg_stage", k_eg_stage, grid_for(n), kBlock, s, n, w.gx, w.kb, w.vb, w.krow, phi, z, barcode,
                   w.sphi, w.sz, w.sbc, w.tf);
        if (int rc = scan_counts(w.tf, 0, 1, w.tx, nullptr, n, w.sums, s)) return rc;
        GNN_LAUNCH("k_eg_tstart", k_eg_tstart, grid_for(n), kBlock, s, n, w.tf, w.tx, w.tstart);
        const unsigned grid = (unsigned)min(n, (int64_t)device_cus() * kPairWgPerCu);
        GNN_LAUNCH("k_eg_pairs", k_eg_pairs<false>, grid, kFB, s, n, w.tx, w.tstart, w.kb, w.vb, w.sphi, w.sz, w.sbc,
                   w.ehit, dphi_max, dz_max, n_nodes_min, n_nodes_max, w.cnt, w.total, nullptr, nullptr, nullptr,
                   nullptr, nullptr, nullptr, nullptr);
        if (int rc = scan_counts(w.cnt, 0, 1, w.soff, nullptr, n, w.sums, s)) return rc;
    }
    GNN_LAUNCH("k_eg_events", k_eg_events, grid_for(E), kBlock, s, E, w.stride, w.ehit, w.soff, n_nodes_min, n_nodes_max,
               n_edges_max, w.ev3);
    if (int rc = scan_counts(w.ev3, w.stride, 2, w.ogr, w.ohit, E, w.sums, s)) return rc;
    if (int rc = scan_counts(w.ev3 + 2 * w.stride, 0, 1, w.oseg, nullptr, E, w.sums, s)) return rc;
    GNN_LAUNCH("k_eg_final", k_eg_final, grid_for(E + 1), kBlock, s, n, E, w.ev3, w.ogr, w.ohit, w.oseg, w.gx, w.tx,
               w.status, w.total, sizes_out, hit_ptr, seg_ptr, event_index);
    return 0;
}

int gnn_event_graphs_fill(const float *r, const float *phi, const float *z, const int64_t *barcode, int64_t n_rows,
                          int64_t n_events, float dphi_max, float dz_max, double scale_r, double scale_phi,
                          double scale_z, const gnn_event_graphs_sizes_t *sizes, void *workspace,
                          size_t workspace_bytes, float *X, int32_t *src, int32_t *dst, float *y, int64_t *hit_index,
                          int32_t *layer, void *stream)
{
    ProfChain chain_;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = check_args("gnn_event_graphs_fill", n_rows, n_events)) return rc;
    if (int rc = check_cuts("gnn_event_graphs_fill", dphi_max, dz_max)) return rc;
    const int64_t n = n_rows, E = n_events;
    if (!sizes || sizes->status != 0 || sizes->n_graphs < 0 || sizes->n_graphs > E || sizes->n_hits < 0 ||
        sizes->n_hits > sizes->n_kept || sizes->n_kept > n || sizes->n_segments < 0 ||
        sizes->n_segments > sizes->n_tested || sizes->n_tested >= kInt32End || sizes->n_tasks < 0 ||
        sizes->n_tasks > n || (sizes->n_graphs == 0) != (sizes->n_hits == 0))
        return fail(GNN_ERR_BADARG, "gnn_event_graphs_fill: sizes missing, flagged or not from this input");
    if (sizes->n_hits == 0) return 0;
    if (!r || !phi || !z || !barcode || !X || !hit_index || !layer || (sizes->n_segments > 0 && (!src || !dst || !y)))
        return fail(GNN_ERR_BADARG, "gnn_event_graphs_fill: pointer missing");
    if (int rc = check_scales("gnn_event_graphs_fill", scale_r, scale_phi, scale_z)) return rc;
    if (int rc = check_workspace(workspace, workspace_bytes, carve_eg(nullptr, n, E).bytes)) return rc;
    EgWs w = carve_eg(align_ws(workspace), n, E);
    GNN_LAUNCH("k_eg_hits", k_eg_hits, grid_for(sizes->n_kept), kBlock, s, n, w.gx, w.krow, w.kevt, w.klay, w.ehit,
               w.ev3, w.ohit, r, phi, z, scale_r, scale_phi, scale_z, X, hit_index, layer);
    if (sizes->n_segments > 0) {
        const unsigned grid = (unsigned)min(sizes->n_tasks, (int64_t)device_cus() * kPairWgPerCu);
        GNN_LAUNCH("k_eg_pairs", k_eg_pairs<true>, grid, kFB, s, n, w.tx, w.tstart, w.kb, w.vb, w.sphi, w.sz, w.sbc,
                   w.ehit, dphi_max, dz_max, (int64_t)0, (int64_t)0, nullptr, nullptr, w.soff, w.ev3, w.ohit, w.oseg,
                   src, dst, y);
    }
    return 0;
}

}  // extern "C"
