// select_hits.hip - the TrackML barrel hit selection from raw event tables on the GPU.
//
// The reference does it on the host in pandas (gnn/prepareGraphs.py:53-85, select_hits): ten get_group calls and a
// concat for the barrel layers, pt and its cut, two merges (truth with particles, hits with truth), an optional
// "hits every layer" filter and groupby(['particle_id', 'layer']).r.idxmin() for the deduplication.
// gnn-fpga_amd/select_hits.py is the numpy specification of what is computed here; pt and r are the reference's
// float32 arithmetic in its order of operations, with contraction to FMA off (the pragma) and a correctly rounded sqrt.
//
//   gnn_select_hits_sizes
//     k_sh_pkey      one lane per particle row: its event (binary search of its event_ptr), pt, the cut
//     radix sorts    by particle_id (64 bits, biased), then event: stable, so the table stands in (event, id) order
//     k_sh_pstage    event, id and the cut's verdict in that order; adjacent equal keys are a duplicated id
//     k_sh_tkey      one lane per truth row: its event;  radix sorts by hit_id, then event
//     k_sh_tstage    event, hit_id and particle_id in that order, duplicates; each row searches its own event's
//                    particles: is its particle a kept one?
//     k_sh_hkey      one lane per hit row: its event, the layer (table lookup), r, the finite check; a barrel row
//                    searches its own event's truth rows: its particle_id, or no particle
//     radix sorts    by hit_id, then event;  k_sh_hdup: adjacent equal keys are a duplicated hit_id
//     radix sorts    by layer, then particle_id, then event (rows that did not survive sort behind every event): all
//                    stable, so the surviving rows stand in (event, particle, layer, row) order
//     k_sh_group     one lane per position: the first of an (event, particle, layer) group walks it and keeps the hit
//                    of smallest r (the first row on ties)
//     k_sh_layers    no_missing_hits: a group's first position walks its particle and counts the groups
//     scan           numbers the kept hits: that number is the hit's place in the output
//     k_sh_final     event_ptr of the output, the sizes and the status word
//   gnn_select_hits_fill
//     k_sh_fill      gathers r, phi (as given, or atan2f(y, x)), z, layer, particle_id, hit_id and the input row
// Nothing is ordered by atomics (the status word is or-ed by them): two builds of one input give the same bits.
// Known cliff: one particle id shared by very many hits of an event is one lane's long serial walk, in k_sh_group and
// again in k_sh_layers (as a many-hit particle is in hit_samples.hip).
#include <cstring>

#include "common.h"

#include <cmath>

#pragma clang fp contract(off)

#include "builder_sort.h"

namespace gnn {
namespace {

constexpr u64 kSignBit = 0x8000000000000000ull;       // biases an int64 into a u64 of the same (signed) order

inline int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }   // (the host's max() takes ints)

struct ShLayers {                                      // barrel_layers, by value in the kernel arguments
    int32_t n;
    int32_t vol[GNN_SELECT_HITS_MAX_LAYERS], lay[GNN_SELECT_HITS_MAX_LAYERS];
};

struct ShWs {
    int32_t *status;
    int32_t *pevt, *pkeep, *sp_evt, *sp_keep;          // particles: by row; in (event, id) order
    int64_t *sp_pid;
    int32_t *tevt, *st_evt, *st_ok;                    // truth: by row; in (event, hit_id) order
    int64_t *st_hid, *st_pid;
    int32_t *hevt, *sevt, *hlay;                       // hits by row: event, event if it survives the joins (else E)
    int64_t *hpid;
    float *r;
    int32_t *gf, *best, *kf, *kx;
    u64 *ka, *kb;
    int32_t *va, *vb;
    int32_t *sums;
    void *temp;
    size_t temp_bytes;
    size_t bytes;
};

ShWs carve_sh(char *base, int64_t n, int64_t nt, int64_t np, int64_t E)
{
    ShWs w;
    Carver c{base};
    w.status = reinterpret_cast<int32_t *>(c.take<char>(256));
    const int64_t m = max64(n, max64(nt, np));
    w.pevt = c.take<int32_t>(np);
    w.pkeep = c.take<int32_t>(np);
    w.sp_evt = c.take<int32_t>(np);
    w.sp_keep = c.take<int32_t>(np);
    w.sp_pid = c.take<int64_t>(np);
    w.tevt = c.take<int32_t>(nt);
    w.st_evt = c.take<int32_t>(nt);
    w.st_ok = c.take<int32_t>(nt);
    w.st_hid = c.take<int64_t>(nt);
    w.st_pid = c.take<int64_t>(nt);
    w.hevt = c.take<int32_t>(n);
    w.sevt = c.take<int32_t>(n);
    w.hlay = c.take<int32_t>(n);
    w.hpid = c.take<int64_t>(n);
    w.r = c.take<float>(n);
    w.gf = c.take<int32_t>(n);
    w.best = c.take<int32_t>(n);
    w.kf = c.take<int32_t>(n);
    w.kx = c.take<int32_t>(n + 1);
    w.ka = c.take<u64>(m);
    w.kb = c.take<u64>(m);
    w.va = c.take<int32_t>(m);
    w.vb = c.take<int32_t>(m);
    w.sums = c.take<int32_t>(scan_sums_words(max64(n, E)));
    w.temp_bytes = m > 0 ? sort_temp_bytes(m) : 0;
    w.temp = c.take<char>(w.temp_bytes);
    w.bytes = c.bytes();
    return w;
}

// the event of row i of a table, E where event_ptr gives it to none (check_event_ptr flags that)
__device__ __forceinline__ int event_of(const int64_t *ep, int64_t E, int64_t i)
{
    const int64_t e = last_le(ep, E, i);
    return event_owns(ep, e, i) ? (int)e : (int)E;
}

// the first position of a table in (event, id) order, ids signed, whose (event, id) is not below (e, v); n if none
__device__ __forceinline__ int64_t find_pair(const int32_t *evt, const int64_t *id, int64_t n, int e, int64_t v)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (evt[mid] < e || (evt[mid] == e && id[mid] < v)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// :64-67: pt = sqrt(px**2 + py**2) in float32, kept when pt > pt_min (NaN compares false)
__global__ __launch_bounds__(kBlock) void k_sh_pkey(const int64_t *__restrict__ pid, const float *__restrict__ px,
                                                    const float *__restrict__ py, int64_t np,
                                                    const int64_t *__restrict__ ep, int64_t E, float pt_min,
                                                    int32_t *__restrict__ pevt, int32_t *__restrict__ pkeep,
                                                    u64 *__restrict__ key, int32_t *__restrict__ val,
                                                    int32_t *__restrict__ status)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    check_event_ptr(ep, E, np, i, status);
    if (i >= np) return;
    const float a = px[i] * px[i], b = py[i] * py[i];
    const float pt = sqrtf(a + b);
    pevt[i] = event_of(ep, E, i);
    pkeep[i] = pt > pt_min;
    key[i] = (u64)pid[i] ^ kSignBit;
    val[i] = (int)i;
}

// a table's hit_id (or any int64 id) as the sort key, its event by row
__global__ __launch_bounds__(kBlock) void k_sh_tkey(const int64_t *__restrict__ id, int64_t nt,
                                                    const int64_t *__restrict__ ep, int64_t E,
                                                    int32_t *__restrict__ tevt, u64 *__restrict__ key,
                                                    int32_t *__restrict__ val, int32_t *__restrict__ status)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    check_event_ptr(ep, E, nt, i, status);
    if (i >= nt) return;
    tevt[i] = event_of(ep, E, i);
    key[i] = (u64)id[i] ^ kSignBit;
    val[i] = (int)i;
}

__global__ __launch_bounds__(kBlock) void k_sh_evkey(int64_t n, const int32_t *__restrict__ evt,
                                                     const int32_t *__restrict__ rows, u64 *__restrict__ key)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j < n) key[j] = (u64)evt[rows[j]];
}

__global__ __launch_bounds__(kBlock) void k_sh_pstage(int64_t np, int64_t E, const int32_t *__restrict__ rows,
                                                      const int32_t *__restrict__ pevt,
                                                      const int32_t *__restrict__ pkeep,
                                                      const int64_t *__restrict__ pid, int32_t *__restrict__ sp_evt,
                                                      int64_t *__restrict__ sp_pid, int32_t *__restrict__ sp_keep,
                                                      int32_t *__restrict__ status)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= np) return;
    const int a = rows[j];
    const int e = pevt[a];
    const int64_t id = pid[a];
    sp_evt[j] = e;
    sp_pid[j] = id;
    sp_keep[j] = pkeep[a];
    if (j > 0 && e < E) {
        const int q = rows[j - 1];
        if (pevt[q] == e && pid[q] == id) atomicOr(status, kStatusDup);
    }
}

// :68-69: truth.merge(particles[['particle_id']], on='particle_id'), per event: noise (id 0) has no particle row
__global__ __launch_bounds__(kBlock) void k_sh_tstage(int64_t nt, int64_t E, const int32_t *__restrict__ rows,
                                                      const int32_t *__restrict__ tevt,
                                                      const int64_t *__restrict__ thid,
                                                      const int64_t *__restrict__ tpid, int64_t np,
                                                      const int32_t *__restrict__ sp_evt,
                                                      const int64_t *__restrict__ sp_pid,
                                                      const int32_t *__restrict__ sp_keep,
                                                      int32_t *__restrict__ st_evt, int64_t *__restrict__ st_hid,
                                                      int64_t *__restrict__ st_pid, int32_t *__restrict__ st_ok,
                                                      int32_t *__restrict__ status)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= nt) return;
    const int a = rows[j];
    const int e = tevt[a];
    const int64_t hid = thid[a], id = tpid[a];
    st_evt[j] = e;
    st_hid[j] = hid;
    st_pid[j] = id;
    int ok = 0;
    if (e < E) {
        const int64_t p = find_pair(sp_evt, sp_pid, np, e, id);
        ok = p < np && sp_evt[p] == e && sp_pid[p] == id && sp_keep[p];
        if (j > 0) {
            const int q = rows[j - 1];
            if (tevt[q] == e && thid[q] == hid) atomicOr(status, kStatusDup);
        }
    }
    st_ok[j] = ok;
}

// :60-62 the layer, :71 r = sqrt(x**2 + y**2) in float32, :74-76 the merge with truth, per event
__global__ __launch_bounds__(kBlock) void k_sh_hkey(const int64_t *__restrict__ hid, const float *__restrict__ x,
                                                    const float *__restrict__ y,
                                                    const int32_t *__restrict__ volid,
                                                    const int32_t *__restrict__ layid, int64_t n,
                                                    const int64_t *__restrict__ ep, int64_t E, ShLayers tab,
                                                    int64_t nt, const int32_t *__restrict__ st_evt,
                                                    const int64_t *__restrict__ st_hid,
                                                    const int64_t *__restrict__ st_pid,
                                                    const int32_t *__restrict__ st_ok, int32_t *__restrict__ hevt,
                                                    int32_t *__restrict__ sevt, int32_t *__restrict__ hlay,
                                                    int64_t *__restrict__ hpid, float *__restrict__ r,
                                                    u64 *__restrict__ key, int32_t *__restrict__ val,
                                                    int32_t *__restrict__ status)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    check_event_ptr(ep, E, n, i, status);
    if (i >= n) return;
    const int e = event_of(ep, E, i);
    const float xx = x[i], yy = y[i];
    const float a = xx * xx, b = yy * yy;
    r[i] = sqrtf(a + b);
    const int v = volid[i], li = layid[i];
    int l = -1;
    for (int k = tab.n - 1; k >= 0; --k)
        if (tab.vol[k] == v && tab.lay[k] == li) l = k;  // the first entry that matches
    int s = (int)E;
    int64_t id = 0;
    const int64_t h = hid[i];
    if (!(isfinite(xx) && isfinite(yy))) {
        atomicOr(status, kStatusFinite);
    } else if (l >= 0 && e < E) {
        const int64_t p = find_pair(st_evt, st_hid, nt, e, h);
        if (p < nt && st_evt[p] == e && st_hid[p] == h && st_ok[p]) {
            s = e;
            id = st_pid[p];
        }
    }
    hevt[i] = e;
    sevt[i] = s;
    hlay[i] = l < 0 ? 0 : l;
    hpid[i] = id;
    key[i] = (u64)h ^ kSignBit;
    val[i] = (int)i;
}

__global__ __launch_bounds__(kBlock) void k_sh_hdup(int64_t n, int64_t E, const int32_t *__restrict__ rows,
                                                    const int32_t *__restrict__ hevt, const int64_t *__restrict__ hid,
                                                    int32_t *__restrict__ status)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j < 1 || j >= n) return;
    const int a = rows[j], q = rows[j - 1];
    if (hevt[a] < E && hevt[a] == hevt[q] && hid[a] == hid[q]) atomicOr(status, kStatusDup);
}

__global__ __launch_bounds__(kBlock) void k_sh_laykey(int64_t n, const int32_t *__restrict__ hlay,
                                                      u64 *__restrict__ key, int32_t *__restrict__ val)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    key[i] = (u64)hlay[i];
    val[i] = (int)i;
}

__global__ __launch_bounds__(kBlock) void k_sh_pidkey(int64_t n, const int64_t *__restrict__ hpid,
                                                      const int32_t *__restrict__ rows, u64 *__restrict__ key)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j < n) key[j] = (u64)hpid[rows[j]] ^ kSignBit;
}

// rows: (event, particle, layer, row) order.  :82-84: the first position of a group keeps its hit of smallest r
__global__ __launch_bounds__(kBlock) void k_sh_group(int64_t n, int64_t E, const int32_t *__restrict__ rows,
                                                     const int32_t *__restrict__ sevt,
                                                     const int32_t *__restrict__ hlay,
                                                     const int64_t *__restrict__ hpid, const float *__restrict__ r,
                                                     int32_t *__restrict__ gf, int32_t *__restrict__ best)
{
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const int a = rows[p];
    const int e = sevt[a], l = hlay[a];
    const int64_t id = hpid[a];
    int f = e < E;
    if (f && p > 0) {
        const int q = rows[p - 1];
        f = sevt[q] != e || hpid[q] != id || hlay[q] != l;
    }
    int row = a;
    if (f) {
        float rb = r[a];
        for (int64_t k = p + 1; k < n; ++k) {          // idxmin: the first in frame order on ties (rows ascend)
            const int q = rows[k];
            if (sevt[q] != e || hpid[q] != id || hlay[q] != l) break;
            if (r[q] < rb) {
                rb = r[q];
                row = q;
            }
        }
    }
    gf[p] = f;
    best[p] = row;
}

// :77-80: with no_missing_hits a particle is kept when its hits cover n_layers distinct layers: its groups, counted
// by each group's first position over the particle's positions on both sides
__global__ __launch_bounds__(kBlock) void k_sh_layers(int64_t n, int32_t n_layers, const int32_t *__restrict__ rows,
                                                      const int32_t *__restrict__ sevt,
                                                      const int64_t *__restrict__ hpid,
                                                      const int32_t *__restrict__ gf, int32_t *__restrict__ kf)
{
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    int f = gf[p];
    if (f) {
        const int a = rows[p];
        const int e = sevt[a];
        const int64_t id = hpid[a];
        int c = 1;
        for (int64_t k = p - 1; k >= 0; --k) {
            const int q = rows[k];
            if (sevt[q] != e || hpid[q] != id) break;
            c += gf[k];
        }
        for (int64_t k = p + 1; k < n; ++k) {
            const int q = rows[k];
            if (sevt[q] != e || hpid[q] != id) break;
            c += gf[k];
        }
        f = c == n_layers;
    }
    kf[p] = f;
}

__global__ __launch_bounds__(kBlock) void k_sh_final(int64_t n, int64_t E, const u64 *__restrict__ sorted_evt,
                                                     const int32_t *__restrict__ kx,
                                                     const int32_t *__restrict__ status,
                                                     gnn_select_hits_sizes_t *sizes, int64_t *__restrict__ out_ptr)
{
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e > E) return;
    out_ptr[e] = kx[lower_bound(sorted_evt, n, (u64)e)];
    if (e == E) {
        sizes->n_kept = kx[n];
        sizes->status = *status;
    }
}

__global__ __launch_bounds__(kBlock) void k_sh_fill(int64_t n, const int32_t *__restrict__ kf,
                                                    const int32_t *__restrict__ kx, const int32_t *__restrict__ best,
                                                    const int32_t *__restrict__ hlay, const int64_t *__restrict__ hpid,
                                                    const float *__restrict__ rr, const int64_t *__restrict__ hid,
                                                    const float *__restrict__ x, const float *__restrict__ y,
                                                    const float *__restrict__ z, const float *__restrict__ phi,
                                                    float *__restrict__ o_r, float *__restrict__ o_phi,
                                                    float *__restrict__ o_z, int32_t *__restrict__ o_layer,
                                                    int64_t *__restrict__ o_pid, int64_t *__restrict__ o_hid,
                                                    int64_t *__restrict__ o_row)
{
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n || !kf[p]) return;
    const int q = kx[p], row = best[p];
    o_r[q] = rr[row];
    o_phi[q] = phi ? phi[row] : atan2f(y[row], x[row]);    // :72
    o_z[q] = z[row];
    o_layer[q] = hlay[row];
    o_pid[q] = hpid[row];
    o_hid[q] = hid[row];
    o_row[q] = row;
}

int check_args(const char *who, int64_t n, int64_t nt, int64_t np, int64_t E)
{
    if (n < 0 || nt < 0 || np < 0 || E < 1)
        return fail(GNN_ERR_BADARG, "%s: bad argument (n_hits %lld, n_truth %lld, n_particles %lld, n_events %lld)", who,
                    (long long)n, (long long)nt, (long long)np, (long long)E);
    if (max64(max64(n, nt), max64(np, E)) >= kInt32End - 1)
        return fail(GNN_ERR_UNSUPPORTED, "%s: sizes outside the int32 index range", who);
    return 0;
}

}  // namespace
}  // namespace gnn

using namespace gnn;

extern "C" {

size_t gnn_select_hits_workspace_bytes(int64_t n_hits, int64_t n_truth, int64_t n_particles, int64_t n_events)
{
    if (check_args("gnn_select_hits_workspace_bytes", n_hits, n_truth, n_particles, n_events)) return 0;
    return carve_sh(nullptr, n_hits, n_truth, n_particles, n_events).bytes;
}

int gnn_select_hits_sizes(const int64_t *hit_id, const float *x, const float *y, const int32_t *volume_id,
                          const int32_t *layer_id, int64_t n_hits, const int64_t *hit_event_ptr,
                          const int64_t *truth_hit_id, const int64_t *truth_particle_id, int64_t n_truth,
                          const int64_t *truth_event_ptr, const int64_t *particle_id, const float *px, const float *py,
                          int64_t n_particles, const int64_t *particle_event_ptr, int64_t n_events,
                          const int32_t *barrel_layers, int32_t n_layers, float pt_min, int32_t no_missing_hits,
                          void *workspace, size_t workspace_bytes, gnn_select_hits_sizes_t *sizes_out,
                          int64_t *event_ptr_out, void *stream)
{
    const char *who = "gnn_select_hits_sizes";
    ProfChain chain_;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t n = n_hits, nt = n_truth, np = n_particles, E = n_events;
    if (int rc = check_args(who, n, nt, np, E)) return rc;
    if (n_layers < 1 || n_layers > GNN_SELECT_HITS_MAX_LAYERS || !barrel_layers)
        return fail(GNN_ERR_BADARG, "%s: barrel_layers needs 1 .. %d (volume, layer) pairs", who,
                    GNN_SELECT_HITS_MAX_LAYERS);
    if (pt_min != pt_min) return fail(GNN_ERR_BADARG, "%s: pt_min is NaN", who);
    if ((n > 0 && (!hit_id || !x || !y || !volume_id || !layer_id)) || (nt > 0 && (!truth_hit_id || !truth_particle_id)) ||
        (np > 0 && (!particle_id || !px || !py)) || !hit_event_ptr || !truth_event_ptr || !particle_event_ptr ||
        !sizes_out || !event_ptr_out)
        return fail(GNN_ERR_BADARG, "%s: pointer missing", who);
    if (int rc = check_workspace(workspace, workspace_bytes, carve_sh(nullptr, n, nt, np, E).bytes)) return rc;
    ShWs w = carve_sh(align_ws(workspace), n, nt, np, E);
    ShLayers tab;
    memset(&tab, 0, sizeof tab);
    tab.n = n_layers;
    for (int k = 0; k < n_layers; ++k) {
        tab.vol[k] = barrel_layers[2 * k];
        tab.lay[k] = barrel_layers[2 * k + 1];
    }
    hipError_t err = hipMemsetAsync(w.status, 0, 256, s);
    if (err == hipSuccess) err = hipMemsetAsync(sizes_out, 0, sizeof(gnn_select_hits_sizes_t), s);
    if (err == hipSuccess) err = hipMemsetAsync(w.kx, 0, sizeof(int32_t), s);        // (n = 0: no scan writes it)
    if (err != hipSuccess) return fail(-(int)err, "%s: memset failed: %s", who, hipGetErrorString(err));
    auto sort = [&](const char *what, int64_t m, const u64 *kin, u64 *kout, const int32_t *vin, int32_t *vout, int bits) {
        return sort_pairs(who, what, w.temp, w.temp_bytes, kin, kout, vin, vout, m, bits, s);
    };
    const int ebits = bits_for((u64)E);
    // a table in (event, id) order: the least significant key first, both sorts stable; the rows end in va
    auto by_event_and_id = [&](const char *what, int64_t m, const int32_t *evt) {
        if (int rc = sort(what, m, w.ka, w.kb, w.va, w.vb, 64)) return rc;
        GNN_LAUNCH("k_sh_evkey", k_sh_evkey, grid_for(m), kBlock, s, m, evt, w.vb, w.ka);
        return sort("by event", m, w.ka, w.kb, w.vb, w.va, ebits);
    };
    GNN_LAUNCH("k_sh_pkey", k_sh_pkey, max(grid_for(max64(np, E)), 1u), kBlock, s, particle_id, px, py, np,
               particle_event_ptr, E, pt_min, w.pevt, w.pkeep, w.ka, w.va, w.status);
    if (np > 0) {
        if (int rc = by_event_and_id("particles by particle_id", np, w.pevt)) return rc;
        GNN_LAUNCH("k_sh_pstage", k_sh_pstage, grid_for(np), kBlock, s, np, E, w.va, w.pevt, w.pkeep, particle_id,
                   w.sp_evt, w.sp_pid, w.sp_keep, w.status);
    }
    GNN_LAUNCH("k_sh_tkey", k_sh_tkey, max(grid_for(max64(nt, E)), 1u), kBlock, s, truth_hit_id, nt, truth_event_ptr, E,
               w.tevt, w.ka, w.va, w.status);
    if (nt > 0) {
        if (int rc = by_event_and_id("truth by hit_id", nt, w.tevt)) return rc;
        GNN_LAUNCH("k_sh_tstage", k_sh_tstage, grid_for(nt), kBlock, s, nt, E, w.va, w.tevt, truth_hit_id,
                   truth_particle_id, np, w.sp_evt, w.sp_pid, w.sp_keep, w.st_evt, w.st_hid, w.st_pid, w.st_ok,
                   w.status);
    }
    GNN_LAUNCH("k_sh_hkey", k_sh_hkey, max(grid_for(max64(n, E)), 1u), kBlock, s, hit_id, x, y, volume_id, layer_id, n,
               hit_event_ptr, E, tab, nt, w.st_evt, w.st_hid, w.st_pid, w.st_ok, w.hevt, w.sevt, w.hlay, w.hpid, w.r,
               w.ka, w.va, w.status);
    if (n > 0) {
        if (int rc = by_event_and_id("hits by hit_id", n, w.hevt)) return rc;
        GNN_LAUNCH("k_sh_hdup", k_sh_hdup, grid_for(n), kBlock, s, n, E, w.va, w.hevt, hit_id, w.status);
        // (event, particle, layer, row) order; the rows end in va, their events (E: not a survivor) in kb
        GNN_LAUNCH("k_sh_laykey", k_sh_laykey, grid_for(n), kBlock, s, n, w.hlay, w.ka, w.vb);
        if (int rc = sort("hits by layer", n, w.ka, w.kb, w.vb, w.va, bits_for((u64)(n_layers - 1)))) return rc;
        GNN_LAUNCH("k_sh_pidkey", k_sh_pidkey, grid_for(n), kBlock, s, n, w.hpid, w.va, w.ka);
        if (int rc = sort("hits by particle_id", n, w.ka, w.kb, w.va, w.vb, 64)) return rc;
        GNN_LAUNCH("k_sh_evkey", k_sh_evkey, grid_for(n), kBlock, s, n, w.sevt, w.vb, w.ka);
        if (int rc = sort("hits by event", n, w.ka, w.kb, w.vb, w.va, ebits)) return rc;
        GNN_LAUNCH("k_sh_group", k_sh_group, grid_for(n), kBlock, s, n, E, w.va, w.sevt, w.hlay, w.hpid, w.r, w.gf,
                   w.best);
        const int32_t *flags = w.gf;
        if (no_missing_hits) {
            GNN_LAUNCH("k_sh_layers", k_sh_layers, grid_for(n), kBlock, s, n, n_layers, w.va, w.sevt, w.hpid, w.gf,
                       w.kf);
            flags = w.kf;
        }
        if (int rc = scan_counts(flags, 0, 1, w.kx, nullptr, n, w.sums, s)) return rc;
    }
    GNN_LAUNCH("k_sh_final", k_sh_final, grid_for(E + 1), kBlock, s, n, E, w.kb, w.kx, w.status, sizes_out,
               event_ptr_out);
    return 0;
}

int gnn_select_hits_fill(const int64_t *hit_id, const float *x, const float *y, const float *z, const float *phi,
                         int64_t n_hits, int64_t n_truth, int64_t n_particles, int64_t n_events,
                         int32_t no_missing_hits, const gnn_select_hits_sizes_t *sizes, void *workspace,
                         size_t workspace_bytes, float *r_out, float *phi_out, float *z_out, int32_t *layer_out,
                         int64_t *particle_id_out, int64_t *hit_id_out, int64_t *row_out, void *stream)
{
    const char *who = "gnn_select_hits_fill";
    ProfChain chain_;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t n = n_hits;
    if (int rc = check_args(who, n, n_truth, n_particles, n_events)) return rc;
    if (!sizes || sizes->status != 0 || sizes->n_kept < 0 || sizes->n_kept > n)
        return fail(GNN_ERR_BADARG, "%s: sizes missing, flagged or not from this input", who);
    if (sizes->n_kept == 0) return 0;
    if (!hit_id || !z || (!phi && (!x || !y)) || !r_out || !phi_out || !z_out || !layer_out || !particle_id_out ||
        !hit_id_out || !row_out)
        return fail(GNN_ERR_BADARG, "%s: pointer missing", who);
    if (int rc = check_workspace(workspace, workspace_bytes, carve_sh(nullptr, n, n_truth, n_particles, n_events).bytes))
        return rc;
    ShWs w = carve_sh(align_ws(workspace), n, n_truth, n_particles, n_events);
    GNN_LAUNCH("k_sh_fill", k_sh_fill, grid_for(n), kBlock, s, n, no_missing_hits ? w.kf : w.gf, w.kx, w.best, w.hlay,
               w.hpid, w.r, hit_id, x, y, z, phi, r_out, phi_out, z_out, layer_out, particle_id_out, hit_id_out,
               row_out);
    return 0;
}

}  // extern "C"
