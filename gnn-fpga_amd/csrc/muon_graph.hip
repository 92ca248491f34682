// muon_graph.hip - muon trigger graphs from EMTF hits on the GPU.
//
// The reference builds them on the host in pandas: gnn/prepareMuonGraphs.py main (:171-263) looks up every hit's layer
// in a row-wise DataFrame.apply, filters, deduplicates and mixes the muon and PU frames entry by entry, takes the
// layer pairs from Python set order, and calls gnn/Muon_graph.py construct_graph per entry, which merges every hit of
// layer l1 with every hit of layer l2.  gnn-fpga_amd/muon_graph.py is the numpy specification of what is computed
// here; the output is bit-identical to it: the pair test (keep_pair, builder_common.h) is the reference's float32
// operations in the same order, with contraction to FMA off (the pragma) and IEEE division, and the layer order is an
// exact emulation of CPython's set insertion.
//
//   gnn_muon_graph_sizes
//     k_mg_check      one lane per row of either source and per entry: LUT index range, finite z, event_ptr -> status
//     k_mg_entry      one wavefront per entry: both sources' rows in chunks of 64 lanes; the cross-frame filter, the
//                     truth filter and the first row of every chamber (a ballot per chamber: the lowest lane not seen
//                     before) -> <= 21 kept subentries per source, in row order; "has rows" flags
//     scan            the two flag arrays -> muon and PU ordinals (the reference's mixing is by ordinal)
//     k_mg_graph      one lane per entry: which sources the graph of the entry holds, in which order, its hit count
//     scan            hit counts and "graph exists" -> hit offsets, graph numbers
//     k_mg_pairs<0>   one wavefront per entry: the hits in LDS, the set order and the layer pairs (lane 0), then every
//                     (pair, l1 hit, l2 hit) candidate on its own lane, tested; counts the kept segments
//     scan            segment counts -> segment offsets
//     k_mg_final      one lane per entry: hit_ptr, seg_ptr by graph number, the sizes and the status word
//   gnn_muon_graph_fill
//     k_mg_pairs<1>   the same again; writes X, hit_source, hit_row, src, dst, y (a ballot orders the kept
//                     candidates) and entry, pt, eta, flags, counts per graph
//   gnn_muon_graph_padded (no read-back)
//     k_mg_check, k_mg_entry, scan, k_mg_graph, then k_mg_pairs<2>: graph slot e = entry e, 42 hits and 441 segments,
//     the unused ones written as padding (X = 0 rows, src = dst = -1)
// Nothing is ordered by atomics: two builds of one input give the same bits.
#include "common.h"

#include <cmath>

#pragma clang fp contract(off)

#include "builder_common.h"

namespace gnn {
namespace {

constexpr int kChambers = 21;                          // (type, station, ring) with a layer in the reference's LUT
constexpr int kGraphHits = 2 * kChambers;              // 42: deduplicated muon + PU rows of one entry
constexpr int kGraphSegs = kChambers * kChambers;      // 441: the pairs form a bipartite graph over <= 42 hits
constexpr int kWave = 64;
constexpr int kLayerHits = 8;                          // hits of one signed layer value != 0: <= 3 chambers x 2 sources
constexpr int kMaxEntries = 0x7FFFFFFF / kGraphSegs;
constexpr float kCutF = 10e30f;                        // gnn/Muon_graph.py:60: 10e30, compared in float32
constexpr int kMgStatusIndex = 1, kMgStatusFinite = 2, kMgStatusEvents = 4;   // (not the hit builders' bits)
constexpr int kFlagPresent = 1, kFlagWritten = 2, kFlagVpMissing = 4;
constexpr unsigned kAllChambers = (1u << kChambers) - 1;
constexpr int8_t kEmpty = -128;

// gnn/prepareMuonGraphs.py:71-92: chamber id 0..20 of LUT index t * 25 + s * 5 + r, -1 where the LUT holds -99
__constant__ int8_t c_chamber[125] = {
    -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,   // type 0
    -1, -1, -1, -1, -1, -1, 0, 1, 2, 3, -1, 4, 5, -1, -1, -1, 6, 7, -1, -1, -1, 8, 9, -1, -1,             // type 1
    -1, -1, -1, -1, -1, -1, -1, 10, -1, -1, -1, -1, 11, -1, -1, -1, 12, 13, 14, -1, -1, 15, 16, 17, -1,   // type 2
    -1, -1, -1, -1, -1, -1, 18, -1, -1, -1, -1, 19, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,  // type 3
    -1, -1, -1, -1, -1, -1, 20, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}; // type 4
// the layer of each chamber: ME1/1b, ME1/2, ME1/3, ME1/1a, ME2/1, ME2/2, ME3/1, ME3/2, ME4/1, ME4/2, RE1/2, RE2/2,
// RE3/1-3, RE4/1-3, GE1/1, GE2/1, ME0
__constant__ int8_t c_layer[kChambers] = {3, 4, 4, 3, 8, 8, 9, 9, 11, 11, 5, 6, 10, 10, 10, 12, 12, 12, 2, 7, 1};

__device__ __forceinline__ int chamber_of(int t, int s, int r)
{
    if ((unsigned)t >= 5u || (unsigned)s >= 5u || (unsigned)r >= 5u) return -1;
    return c_chamber[t * 25 + s * 5 + r];
}

// rows of entry e of one source, clamped into [0, n_rows] (a malformed event_ptr is flagged by k_mg_check)
__device__ __forceinline__ void entry_rows(const gnn_emtf_hits_t &h, int64_t e, int64_t *lo, int64_t *len)
{
    const int64_t a = min(max(h.event_ptr[e], (int64_t)0), h.n_rows);
    const int64_t b = min(max(h.event_ptr[e + 1], a), h.n_rows);
    *lo = a;
    *len = min(b - a, (int64_t)0x7FFFFFFF);
}

struct MgWs {
    int32_t *status;
    int32_t *fl, *kmu, *kpu, *cnt, *rows, *hc, *hoff, *goff, *meta, *scnt, *soff, *sums;
    int64_t E, stride;
    size_t bytes;
};

MgWs carve_mg(char *base, int64_t E)
{
    MgWs w;
    w.E = E;
    w.stride = (E + 64) & ~(int64_t)63;
    Carver c{base};
    w.status = c.take<int32_t>(64);
    w.fl = c.take<int32_t>(2 * w.stride);
    w.kmu = c.take<int32_t>(E + 1);
    w.kpu = c.take<int32_t>(E + 1);
    w.cnt = c.take<int32_t>(2 * E);
    w.rows = c.take<int32_t>(2 * E * kChambers);
    w.hc = c.take<int32_t>(2 * w.stride);
    w.hoff = c.take<int32_t>(E + 1);
    w.goff = c.take<int32_t>(E + 1);
    w.meta = c.take<int32_t>(E);
    w.scnt = c.take<int32_t>(E);
    w.soff = c.take<int32_t>(E + 1);
    w.sums = c.take<int32_t>(scan_sums_words(E));
    w.bytes = c.bytes();
    return w;
}

__device__ __forceinline__ void check_source(const gnn_emtf_hits_t &h, int64_t i, int64_t E, int32_t *status)
{
    if (i < h.n_rows) {
        const int t = h.type[i], s = h.station[i], r = h.ring[i];
        if ((unsigned)t >= 5u || (unsigned)s >= 5u || (unsigned)r >= 5u) atomicOr(status, kMgStatusIndex);
        if (!isfinite(h.z[i])) atomicOr(status, kMgStatusFinite);
    }
    if (i < E) {
        const int64_t a = h.event_ptr[i], b = h.event_ptr[i + 1];
        if (a > b || b - a > 0x7FFFFFFF || (i == 0 && (a != 0 || h.event_ptr[E] != h.n_rows)))
            atomicOr(status, kMgStatusEvents);
    }
}

__global__ __launch_bounds__(kBlock) void k_mg_check(gnn_emtf_hits_t mu, gnn_emtf_hits_t pu, int64_t E,
                                                     int32_t *__restrict__ status)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    check_source(mu, i, E, status);
    check_source(pu, i, E, status);
}

// the lane that holds the first row of a chamber not seen before keeps it (chamber -1: nothing to keep)
__device__ __forceinline__ bool first_of_chamber(int ch, unsigned &seen)
{
    const int lane = threadIdx.x;
    bool keep = false;
    for (int k = 0; k < kChambers; ++k) {
        const unsigned long long m = __ballot(ch == k);
        if (m && !((seen >> k) & 1u)) {
            keep |= lane == __ffsll((long long)m) - 1;
            seen |= 1u << k;
        }
    }
    return keep;
}

__device__ __forceinline__ int compact(bool keep, int32_t *out, int cnt, int value)
{
    const int lane = threadIdx.x;
    const unsigned long long m = __ballot(keep);
    if (keep) out[cnt + __popcll(m & ((1ull << lane) - 1))] = value;
    return cnt + __popcll(m);
}

// one wavefront per entry: gnn/prepareMuonGraphs.py:178-179 (cross-frame filter), :192 (truth filter), :202 and :209
// (first row of every (type, station, ring) per source and entry) -> kept subentries in row order
__global__ __launch_bounds__(kWave) void k_mg_entry(gnn_emtf_hits_t mu, gnn_emtf_hits_t pu, int64_t E, int64_t stride,
                                                    int32_t *__restrict__ cnt, int32_t *__restrict__ rows,
                                                    int32_t *__restrict__ fl)
{
    const int64_t e = blockIdx.x;
    const int lane = threadIdx.x;
    int64_t bm, nm, bp, np_;
    entry_rows(mu, e, &bm, &nm);
    entry_rows(pu, e, &bp, &np_);
    const int n = (int)min(nm, np_);
    int32_t *rm = rows + e * kChambers, *rp = rows + (E + e) * kChambers;
    unsigned seen_m = 0, seen_p = 0;
    int cm = 0, cp = 0;
    for (int s0 = 0; s0 < n; s0 += kWave) {
        const int s = s0 + lane;
        int chm = -1, chp = -1;
        if (s < n) {
            const int64_t im = bm + s, ip = bp + s;
            const int a = chamber_of(mu.type[im], mu.station[im], mu.ring[im]);
            const int b = chamber_of(pu.type[ip], pu.station[ip], pu.ring[ip]);
            if (a >= 0 && b >= 0) {
                chp = b;
                if (mu.tp1[im] == 0 && mu.tp2[im] == 0) chm = a;
            }
        }
        cm = compact(first_of_chamber(chm, seen_m), rm, cm, s);
        cp = compact(first_of_chamber(chp, seen_p), rp, cp, s);
        if (seen_m == kAllChambers && seen_p == kAllChambers) break;
    }
    if (lane == 0) {
        cnt[e] = cm;
        cnt[E + e] = cp;
        fl[e] = cm > 0;
        fl[stride + e] = cp > 0;
    }
}

// gnn/prepareMuonGraphs.py:193-232: PU entry of ordinal k mixed with the muon entry of ordinal k, then regrouped by
// entry; meta = muon hits | PU hits << 8 | (muon rows first) << 16
__global__ __launch_bounds__(kBlock) void k_mg_graph(int64_t E, int64_t stride, int muon_only,
                                                     const int32_t *__restrict__ fl, const int32_t *__restrict__ kmu,
                                                     const int32_t *__restrict__ kpu, const int32_t *__restrict__ cnt,
                                                     int32_t *__restrict__ meta, int32_t *__restrict__ hc)
{
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= E) return;
    const bool use_mu = fl[e] != 0;
    const bool use_pu = !muon_only && fl[stride + e] != 0 && kpu[e] < kmu[E];
    const int cm = use_mu ? cnt[e] : 0, cp = use_pu ? cnt[E + e] : 0;
    const bool mu_first = use_mu && use_pu && kmu[e] < kpu[e];
    meta[e] = cm | (cp << 8) | ((int)mu_first << 16);
    hc[e] = cm + cp;
    hc[stride + e] = cm + cp > 0;
}

struct MgOut {                                         // gnn_muon_graph_out_t, by value
    float *X;
    int32_t *src, *dst;
    float *y;
    int32_t *hit_source;
    int64_t *hit_row, *entry;
    float *pt, *eta;
    int32_t *flags, *graph_hits, *graph_segments;
};

// CPython's set_add_entry probe sequence (Objects/setobject.c): the slot v is in (true) or would go to (false)
__device__ bool set_probe(const int8_t *tab, unsigned mask, int v, unsigned *slot)
{
    const long long h = v == -1 ? -2 : v;              // hash(-1.0) == -2
    unsigned long long perturb = (unsigned long long)h;
    unsigned long long i = (unsigned long long)h & mask;
    while (true) {
        if (tab[i] == kEmpty) { *slot = (unsigned)i; return false; }
        if (tab[i] == v) { *slot = (unsigned)i; return true; }
        if (i + 9 <= mask) {                           // LINEAR_PROBES
            for (unsigned j = 1; j <= 9; ++j) {
                if (tab[i + j] == kEmpty) { *slot = (unsigned)(i + j); return false; }
                if (tab[i + j] == v) { *slot = (unsigned)(i + j); return true; }
            }
        }
        perturb >>= 5;                                 // PERTURB_SHIFT
        i = (i * 5 + 1 + perturb) & mask;
    }
}

// MODE 0: count the kept segments of entry e -> scnt[e]; 1: write the flat graph; 2: write slot e of the padded layout
template <int MODE>
__global__ __launch_bounds__(kWave) void k_mg_pairs(gnn_emtf_hits_t mu, gnn_emtf_hits_t pu, int64_t E,
                                                    const int32_t *__restrict__ meta, const int32_t *__restrict__ rows,
                                                    const int32_t *__restrict__ hoff, const int32_t *__restrict__ goff,
                                                    const int32_t *__restrict__ soff, int32_t *__restrict__ scnt,
                                                    const float *__restrict__ vp_pt, const float *__restrict__ vp_eta,
                                                    int64_t n_vp, int64_t entry_start, MgOut out)
{
    __shared__ float sr[kGraphHits], sp[kGraphHits], sz[kGraphHits];
    __shared__ int8_t sv[kGraphHits], smu[kGraphHits];
    __shared__ int8_t tab[128], tmp[32];
    __shared__ int8_t lcnt[25], lst[25 * kLayerHits];
    __shared__ int8_t pd1[24], pd2[24];
    __shared__ int16_t pre[25];
    __shared__ int npairs;
    const int64_t e = blockIdx.x;
    const int lane = threadIdx.x;
    const int m = meta[e];
    const int cm = m & 0xFF, cp = (m >> 8) & 0xFF, nh = cm + cp;
    const bool mu_first = (m >> 16) & 1;
    int64_t hb, sb, g;
    if (MODE == 2) {
        hb = e * kGraphHits;
        sb = e * kGraphSegs;
        g = e;
    } else if (nh == 0) {
        if (MODE == 0 && lane == 0) scnt[e] = 0;
        return;
    } else {
        hb = hoff[e];
        sb = MODE == 1 ? soff[e] : 0;
        g = goff[e];
    }
    if (lane < nh) {
        const bool first = lane < (mu_first ? cm : cp);
        const bool is_mu = first == mu_first;
        const int k = first ? lane : lane - (mu_first ? cm : cp);
        // (the source's columns picked pointer by pointer: a reference to either kernel argument would live in
        // scratch)
        const int64_t *ep = is_mu ? mu.event_ptr : pu.event_ptr;
        const int64_t n_rows = is_mu ? mu.n_rows : pu.n_rows;
        const int64_t lo = min(max(ep[e], (int64_t)0), n_rows);
        const int64_t row = lo + rows[((is_mu ? 0 : E) + e) * kChambers + k];
        const float z = (is_mu ? mu.z : pu.z)[row];
        const int t = (is_mu ? mu.type : pu.type)[row], st = (is_mu ? mu.station : pu.station)[row];
        const int rg = (is_mu ? mu.ring : pu.ring)[row];
        const int L = c_layer[chamber_of(t, st, rg)];
        const float r = (is_mu ? mu.r : pu.r)[row], phi = (is_mu ? mu.phi : pu.phi)[row];
        sr[lane] = r;
        sp[lane] = phi;
        sz[lane] = z;
        sv[lane] = (int8_t)(z > 0.f ? L : z < 0.f ? -L : 0);
        smu[lane] = is_mu;
        if (MODE != 0) {
            // gnn/Muon_graph.py:142: float32(float64(column)); the layer is L * np.sign(z): +0 for z = +-0
            float *x = out.X + (hb + lane) * 11;
            x[0] = z;
            x[1] = (is_mu ? mu.theta : pu.theta)[row];
            x[2] = phi;
            x[3] = r;
            x[4] = (float)(is_mu ? mu.bend : pu.bend)[row];
            x[5] = (float)(is_mu ? mu.tp1 : pu.tp1)[row];
            x[6] = (float)(is_mu ? mu.tp2 : pu.tp2)[row];
            x[7] = (float)st;
            x[8] = (float)rg;
            x[9] = (float)t;
            x[10] = (float)L * (z > 0.f ? 1.f : z < 0.f ? -1.f : 0.f);
            out.hit_source[hb + lane] = is_mu;
            out.hit_row[hb + lane] = row;
        }
    } else if (MODE == 2 && lane < kGraphHits) {
        float *x = out.X + (hb + lane) * 11;
        for (int f = 0; f < 11; ++f) x[f] = 0.f;
        out.hit_source[hb + lane] = -1;
        out.hit_row[hb + lane] = -1;
    }
    for (int i = lane; i < 128; i += kWave) tab[i] = kEmpty;
    if (lane < 25) lcnt[lane] = 0;
    __syncthreads();
    if (lane == 0) {
        // gnn/prepareMuonGraphs.py:234: list(set(vh_layer)) in row order - CPython's set insertion, table growth and
        // slot-order iteration
        unsigned mask = 7, fill = 0, slot;
        for (int k = 0; k < nh; ++k) {
            const int v = sv[k];
            if (v != 0 && lcnt[v + 12] < kLayerHits) lst[(v + 12) * kLayerHits + lcnt[v + 12]++] = (int8_t)k;
            if (set_probe(tab, mask, v, &slot)) continue;
            tab[slot] = (int8_t)v;
            if (++fill * 5 >= mask * 3) {
                unsigned size = 8, n_old = 0;
                while (size <= fill * 4) size <<= 1;
                for (unsigned i = 0; i <= mask; ++i)
                    if (tab[i] != kEmpty) tmp[n_old++] = tab[i];
                for (unsigned i = 0; i < size; ++i) tab[i] = kEmpty;
                mask = size - 1;
                for (unsigned i = 0; i < n_old; ++i) {
                    set_probe(tab, mask, tmp[i], &slot);
                    tab[slot] = tmp[i];
                }
            }
        }
        // :236-246: consecutive positive values (l[i], l[i+1]), then consecutive negative values (l[i+1], l[i])
        int np = 0, prev = 0;
        for (unsigned i = 0; i <= mask; ++i) {
            const int v = tab[i];
            if (v == kEmpty || v <= 0) continue;
            if (prev) { pd1[np] = (int8_t)prev; pd2[np] = (int8_t)v; ++np; }
            prev = v;
        }
        prev = 0;
        for (unsigned i = 0; i <= mask; ++i) {
            const int v = tab[i];
            if (v == kEmpty || v >= 0) continue;
            if (prev) { pd1[np] = (int8_t)v; pd2[np] = (int8_t)prev; ++np; }
            prev = v;
        }
        int acc = 0;
        for (int p = 0; p < np; ++p) {
            pre[p] = (int16_t)acc;
            acc += lcnt[pd1[p] + 12] * lcnt[pd2[p] + 12];
        }
        pre[np] = (int16_t)acc;
        npairs = np;
    }
    __syncthreads();
    const int np = npairs, T = pre[np];
    int kept = 0;
    // gnn/Muon_graph.py:60-115: candidate t = (pair, l1 hit, l2 hit) in the merge's order; the ballot keeps that order
    for (int t0 = 0; t0 < T; t0 += kWave) {
        const int t = t0 + lane;
        bool keep = false;
        int a = 0, b = 0;
        if (t < T) {
            int p = 0;
            while (p + 1 < np && pre[p + 1] <= t) ++p;
            const int d1 = pd1[p] + 12, d2 = pd2[p] + 12, q = t - pre[p], n2 = lcnt[d2];
            a = lst[d1 * kLayerHits + q / n2];
            b = lst[d2 * kLayerHits + q % n2];
            // gnn/Muon_graph.py:60-83 with the default thresholds: inf (dr = 0) is not kept either
            keep = keep_pair(sr[a], sp[a], sz[a], sr[b], sp[b], sz[b], kCutF, kCutF);
        }
        const unsigned long long msk = __ballot(keep);
        if (MODE != 0 && keep) {
            const int o = kept + __popcll(msk & ((1ull << lane) - 1));
            if (MODE == 1 || o < kGraphSegs) {
                out.src[sb + o] = (int32_t)(hb + a);
                out.dst[sb + o] = (int32_t)(hb + b);
                out.y[sb + o] = smu[a] && smu[b] ? 1.f : 0.f;
            }
        }
        kept += __popcll(msk);
    }
    if (MODE == 0) {
        if (lane == 0) scnt[e] = kept;
        return;
    }
    if (MODE == 2) {
        kept = min(kept, kGraphSegs);
        for (int o = kept + lane; o < kGraphSegs; o += kWave) {
            out.src[sb + o] = -1;
            out.dst[sb + o] = -1;
            out.y[sb + o] = 0.f;
        }
    }
    if (lane == 0) {
        // :254: vp row entry - start = e of the flat vp frame; the reference raises where it does not exist
        const bool missing = nh > 0 && e >= n_vp;
        out.entry[g] = entry_start + e;
        out.pt[g] = nh > 0 && !missing ? vp_pt[e] : __builtin_nanf("");
        out.eta[g] = nh > 0 && !missing ? vp_eta[e] : __builtin_nanf("");
        out.flags[g] = (nh > 0 ? kFlagPresent : 0) | (np > 0 ? kFlagWritten : 0) | (missing ? kFlagVpMissing : 0);
        out.graph_hits[g] = nh;
        out.graph_segments[g] = kept;
    }
}

__global__ __launch_bounds__(kBlock) void k_mg_final(int64_t E, int64_t stride, const int32_t *__restrict__ hc,
                                                     const int32_t *__restrict__ hoff, const int32_t *__restrict__ goff,
                                                     const int32_t *__restrict__ soff, const int32_t *__restrict__ status,
                                                     gnn_muon_graph_sizes_t *sizes, int64_t *__restrict__ hit_ptr,
                                                     int64_t *__restrict__ seg_ptr)
{
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e > E) return;
    if (e < E) {
        if (!hc[stride + e]) return;
        const int g = goff[e];
        hit_ptr[g] = hoff[e];
        seg_ptr[g] = soff[e];
        atomicMax(reinterpret_cast<unsigned long long *>(&sizes->max_graph_hits), (unsigned long long)hc[e]);
        atomicMax(reinterpret_cast<unsigned long long *>(&sizes->max_graph_segments),
                  (unsigned long long)(soff[e + 1] - soff[e]));
    } else {
        const int G = goff[E];
        hit_ptr[G] = hoff[E];
        seg_ptr[G] = soff[E];
        sizes->n_graphs = G;
        sizes->n_hits = hoff[E];
        sizes->n_segments = soff[E];
        sizes->status = *status;
    }
}

int check_args(const char *who, const gnn_emtf_hits_t *mu, const gnn_emtf_hits_t *pu, int64_t E)
{
    if (!mu || !pu || E < 1 || mu->n_rows < 0 || pu->n_rows < 0)
        return fail(GNN_ERR_BADARG, "%s: bad argument (n_entries %lld)", who, (long long)E);
    if (E > kMaxEntries) return fail(GNN_ERR_UNSUPPORTED, "%s: more than %d entries", who, kMaxEntries);
    for (const gnn_emtf_hits_t *h : {mu, pu}) {
        if (!h->event_ptr || (h->n_rows > 0 && (!h->z || !h->theta || !h->phi || !h->r || !h->bend || !h->tp1 ||
                                                !h->tp2 || !h->station || !h->ring || !h->type)))
            return fail(GNN_ERR_BADARG, "%s: a column pointer is missing", who);
    }
    return 0;
}

int check_out(const char *who, const gnn_muon_graph_out_t *o, bool segs)
{
    if (!o || !o->X || !o->hit_source || !o->hit_row || !o->entry || !o->pt || !o->eta || !o->flags ||
        !o->graph_hits || !o->graph_segments || (segs && (!o->src || !o->dst || !o->y)))
        return fail(GNN_ERR_BADARG, "%s: an output pointer is missing", who);
    return 0;
}

MgOut out_of(const gnn_muon_graph_out_t *o)
{
    return MgOut{o->X, o->src, o->dst, o->y, o->hit_source, o->hit_row, o->entry, o->pt, o->eta, o->flags,
                 o->graph_hits, o->graph_segments};
}

// the part both layouts share: checks, deduplication, ordinals, per-entry graph composition
int prologue(const gnn_emtf_hits_t *mu, const gnn_emtf_hits_t *pu, int64_t E, int muon_only, const MgWs &w,
             hipStream_t s)
{
    hipError_t err = hipMemsetAsync(w.status, 0, 256, s);
    if (err != hipSuccess) return fail(-(int)err, "muon graph: memset failed: %s", hipGetErrorString(err));
    const int64_t n = max(max(mu->n_rows, pu->n_rows), E);
    GNN_LAUNCH("k_mg_check", k_mg_check, grid_for(n), kBlock, s, *mu, *pu, E, w.status);
    GNN_LAUNCH("k_mg_entry", k_mg_entry, (unsigned)E, kWave, s, *mu, *pu, E, w.stride, w.cnt, w.rows, w.fl);
    if (int rc = scan_counts(w.fl, w.stride, 2, w.kmu, w.kpu, E, w.sums, s)) return rc;
    GNN_LAUNCH("k_mg_graph", k_mg_graph, grid_for(E), kBlock, s, E, w.stride, muon_only, w.fl, w.kmu, w.kpu, w.cnt,
               w.meta, w.hc);
    return 0;
}

}  // namespace
}  // namespace gnn

using namespace gnn;

extern "C" {

size_t gnn_muon_graph_workspace_bytes(int64_t n_entries)
{
    if (n_entries < 1 || n_entries > kMaxEntries) {
        fail(GNN_ERR_BADARG, "gnn_muon_graph_workspace_bytes: n_entries %lld outside [1, %d]", (long long)n_entries,
             kMaxEntries);
        return 0;
    }
    return carve_mg(nullptr, n_entries).bytes;
}

int gnn_muon_graph_sizes(const gnn_emtf_hits_t *muon, const gnn_emtf_hits_t *pu, int64_t n_entries, int32_t muon_only,
                         void *workspace, size_t workspace_bytes, gnn_muon_graph_sizes_t *sizes_out, int64_t *hit_ptr,
                         int64_t *seg_ptr, void *stream)
{
    ProfChain chain_;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t E = n_entries;
    if (int rc = check_args("gnn_muon_graph_sizes", muon, pu, E)) return rc;
    if (!sizes_out || !hit_ptr || !seg_ptr) return fail(GNN_ERR_BADARG, "gnn_muon_graph_sizes: pointer missing");
    if (int rc = check_workspace(workspace, workspace_bytes, carve_mg(nullptr, E).bytes)) return rc;
    const MgWs w = carve_mg(align_ws(workspace), E);
    hipError_t err = hipMemsetAsync(sizes_out, 0, sizeof(gnn_muon_graph_sizes_t), s);
    if (err != hipSuccess) return fail(-(int)err, "gnn_muon_graph_sizes: memset failed: %s", hipGetErrorString(err));
    if (int rc = prologue(muon, pu, E, muon_only, w, s)) return rc;
    if (int rc = scan_counts(w.hc, w.stride, 2, w.hoff, w.goff, E, w.sums, s)) return rc;
    GNN_LAUNCH("k_mg_count", k_mg_pairs<0>, (unsigned)E, kWave, s, *muon, *pu, E, w.meta, w.rows, w.hoff, w.goff,
               w.soff, w.scnt, nullptr, nullptr, (int64_t)0, (int64_t)0, MgOut{});
    if (int rc = scan_counts(w.scnt, 0, 1, w.soff, nullptr, E, w.sums, s)) return rc;
    GNN_LAUNCH("k_mg_final", k_mg_final, grid_for(E + 1), kBlock, s, E, w.stride, w.hc, w.hoff, w.goff, w.soff,
               w.status, sizes_out, hit_ptr, seg_ptr);
    return 0;
}

int gnn_muon_graph_fill(const gnn_emtf_hits_t *muon, const gnn_emtf_hits_t *pu, int64_t n_entries, int32_t muon_only,
                        const float *vp_pt, const float *vp_eta, int64_t n_vp, int64_t entry_start,
                        const gnn_muon_graph_sizes_t *sizes, void *workspace, size_t workspace_bytes,
                        const gnn_muon_graph_out_t *out, void *stream)
{
    ProfChain chain_;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t E = n_entries;
    if (int rc = check_args("gnn_muon_graph_fill", muon, pu, E)) return rc;
    if (!sizes || sizes->status != 0 || sizes->n_graphs < 0 || sizes->n_graphs > E || sizes->n_hits < 0 ||
        sizes->n_hits > kGraphHits * E || sizes->n_segments < 0 || sizes->n_segments > kGraphSegs * E)
        return fail(GNN_ERR_BADARG, "gnn_muon_graph_fill: sizes missing, flagged or not from this input");
    if (n_vp < 0 || (n_vp > 0 && (!vp_pt || !vp_eta)))
        return fail(GNN_ERR_BADARG, "gnn_muon_graph_fill: vp arrays missing");
    if (sizes->n_graphs == 0) return 0;
    if (int rc = check_out("gnn_muon_graph_fill", out, sizes->n_segments > 0)) return rc;
    if (int rc = check_workspace(workspace, workspace_bytes, carve_mg(nullptr, E).bytes)) return rc;
    const MgWs w = carve_mg(align_ws(workspace), E);
    GNN_LAUNCH("k_mg_fill", k_mg_pairs<1>, (unsigned)E, kWave, s, *muon, *pu, E, w.meta, w.rows, w.hoff, w.goff,
               w.soff, nullptr, vp_pt, vp_eta, n_vp, entry_start, out_of(out));
    return 0;
}

int gnn_muon_graph_padded(const gnn_emtf_hits_t *muon, const gnn_emtf_hits_t *pu, int64_t n_entries, int32_t muon_only,
                          const float *vp_pt, const float *vp_eta, int64_t n_vp, int64_t entry_start, void *workspace,
                          size_t workspace_bytes, const gnn_muon_graph_out_t *out, int32_t *status, void *stream)
{
    ProfChain chain_;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t E = n_entries;
    if (int rc = check_args("gnn_muon_graph_padded", muon, pu, E)) return rc;
    if (int rc = check_out("gnn_muon_graph_padded", out, true)) return rc;
    if (!status || n_vp < 0 || (n_vp > 0 && (!vp_pt || !vp_eta)))
        return fail(GNN_ERR_BADARG, "gnn_muon_graph_padded: status or vp arrays missing");
    if (int rc = check_workspace(workspace, workspace_bytes, carve_mg(nullptr, E).bytes)) return rc;
    const MgWs w = carve_mg(align_ws(workspace), E);
    if (int rc = prologue(muon, pu, E, muon_only, w, s)) return rc;
    GNN_LAUNCH("k_mg_padded", k_mg_pairs<2>, (unsigned)E, kWave, s, *muon, *pu, E, w.meta, w.rows, nullptr, nullptr,
               nullptr, nullptr, vp_pt, vp_eta, n_vp, entry_start, out_of(out));
    hipError_t err = hipMemcpyAsync(status, w.status, sizeof(int32_t), hipMemcpyDeviceToDevice, s);
    if (err != hipSuccess) return fail(-(int)err, "gnn_muon_graph_padded: copy failed: %s", hipGetErrorString(err));
    return 0;
}

}  // extern "C"
