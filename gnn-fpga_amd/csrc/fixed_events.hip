// fixed_events.hip - the fixed-point forward of SegmentClassifier for batches of SMALL graphs in one launch
// (include/gnn_hip_fixed_events.h): gnn/model.py:140-156 in the arithmetic of fixed_point.hip (fixed_ops.h), one
// workgroup per graph, as k_event / k_iter_event run the float models.
//
// Resident in LDS for the whole call: the ten weight tensors - every layer TRANSPOSED ([k][d], the streamed ones
// zero-padded to the hit rows' stride) - both tables, the graph's index arrays as local ids (event_passes.h), the hit
// rows H and Hn, mi | mo, the per-hit halves P | Q as int64, one score per segment.  Phases, a workgroup barrier after
// each:
//   set-up   weights, tables, local ids; x = quant(X) into the skip columns of H AND Hn (written once)
//   input    (hit, unit)            H[n][d] = T_tanh[requant(Win x + bin)]                    (gnn/model.py:144-146)
//   per pass t = 0 .. T:
//     pq     (hit, unit of 2 D)     P = W1[:, :C] h + (b1 << Fb), Q = W1[:, C:] h             (gnn/model.py:71-73,46)
//     edge   segment                e = T_sig[requant(W2 T_tanh[requant(P[src] + Q[dst])] + b2)]    (gnn/model.py:81)
//     agg    (hit, side, 16 bytes)  mi / mo = requant(sum e_j H[other end j]), pull                (gnn/model.py:114-119)
//     node1  (hit, unit)            q = T_tanh[requant(W3 [mi|mo|h] + b3)], in the space of P | Q   (gnn/model.py:120-124)
//     node2  (hit, unit)            Hn[n][d] = T_tanh[requant(W4 q + b4)]                           (gnn/model.py:125,154)
// Consecutive lanes take consecutive units d of one hit: the weight wT[k][d] is a conflict-free read of consecutive
// words, the input value h[k] one address for the D lanes of a hit.  A lane holds ONE int64 accumulator, so no shape
// needs more than a few dozen registers.  Every sum is an int64 sum of int32 x int32 products in plain C++: no order or
// split changes a bit, and the results equal fixed_point.hip's and fixed_forward_numpy's.
//
// Overflows: a lane counts a stage in a register, fx_count adds the wave by shuffles and issues at most one 64-bit
// atomic add per wave, stage and pass; the lane also keeps the total of its stages, which the waves add into one LDS word
// at the end - the graph's entry of graph_overflows.  Integer adds: the same counters in every run.
#include "common.h"
#include "event_passes.h"
#include "fixed_ops.h"
#include "gnn_hip_fixed_events.h"

namespace {
using namespace gnn;

constexpr int a4(int x) { return (x + 3) & ~3; }

// A workgroup may have all of a CU's 160 KB (fixed_point.hip's k_fx_mlp opts into the same): a graph beyond the limit
// falls back to the chain of per-module launches, and above 80 KB only one workgroup fits a CU whichever limit is set -
// 128 KB would refuse graphs and keep nothing resident that 160 KB loses.
constexpr size_t kFxEvLdsMax = 160 * 1024;

// int32 words of the weight block: WinT [F][D], bin, W1T [2][LDH][D], b1, W2, b2 (4), W3T [3][LDH][D], b3, W4T [D][D], b4
struct FxEvW {
    int oWin, obin, oW1, ob1, oW2, ob2, oW3, ob3, oW4, ob4, total;
    __host__ __device__ constexpr FxEvW(int F, int D)
        : oWin(0), obin(oWin + F * D), oW1(obin + D), ob1(oW1 + 2 * a4(F + D) * D), oW2(ob1 + D), ob2(oW2 + D),
          oW3(ob2 + 4), ob3(oW3 + 3 * a4(F + D) * D), oW4(ob3 + D), ob4(oW4 + D * D), total(ob4 + D)
    {
    }
};

// LDS words per graph: P | Q (int64) first, then H, Hn, mi | mo, the scores, the weights, both tables, the graph's
// overflow total (4 words keep the ids aligned), the local ids
size_t fxev_words(int F, int D, int tb, int64_t cap_h, int64_t cap_s)
{
    const int64_t ldh = a4(F + D);
    return (size_t)(cap_h * (4 * D + 4 * ldh) + ((cap_s + 3) & ~(int64_t)3) + FxEvW(F, D).total + 2 * ((int64_t)1 << tb) +
                    4 + ev_id_words(cap_h, cap_s));
}

extern __shared__ __attribute__((aligned(16))) char fxev_smem[];

template <int F, int D>
__global__ __launch_bounds__((EvCfg<D>::NT)) void k_fx_event(
    gnn_graph_t g, gnn_fx_params_t p, const int32_t *__restrict__ tanh_table, const int32_t *__restrict__ sigmoid_table,
    Fx f, float scale, float inv_scale, const int32_t *__restrict__ hit_ptr, const int32_t *__restrict__ seg_ptr,
    int cap_h, int cap_s, int T, int32_t *__restrict__ e_raw, float *__restrict__ e_float, int64_t *counts,
    int64_t *__restrict__ graph_overflows, int32_t *__restrict__ e_trace, int32_t *__restrict__ H_trace)
{
    constexpr int C = F + D, LDH = a4(C), NT = EvCfg<D>::NT, G = LDH / 4;
    constexpr FxEvW L(F, D);
    const int b = blockIdx.x;
    const int h0 = hit_ptr[b], nh = hit_ptr[b + 1] - h0;
    const int s0 = seg_ptr[b], ns = seg_ptr[b + 1] - s0;
    if (nh <= 0 && ns <= 0) {       // (uniform: before any barrier)
        if (threadIdx.x == 0 && graph_overflows) graph_overflows[b] = 0;
        return;
    }
    const int nt = 1 << f.tb;
    int64_t *PQ = reinterpret_cast<int64_t *>(fxev_smem);
    int32_t *q = reinterpret_cast<int32_t *>(PQ);                   // node layer 1's output: P | Q are dead by then
    int32_t *H = reinterpret_cast<int32_t *>(PQ + (size_t)cap_h * 2 * D), *Hn = H + cap_h * LDH, *M = Hn + cap_h * LDH,
            *es = M + cap_h * 2 * LDH, *w = es + ((cap_s + 3) & ~3), *sTt = w + L.total, *sTs = sTt + nt;
    unsigned long long *total = reinterpret_cast<unsigned long long *>(sTs + nt);
    EvIds ids;
    ids.ip = reinterpret_cast<int32_t *>(total) + 4;
    ids.op = ids.ip + cap_h + 1;
    ids.ie = ids.op + cap_h + 1;
    ids.inb = ids.ie + cap_s;
    ids.oe = ids.inb + cap_s;
    ids.onb = ids.oe + cap_s;
    ids.sl = ids.onb + cap_s;
    ids.dl = ids.sl + cap_s;
    const int32_t *WinT = w + L.oWin, *bin = w + L.obin, *W1T = w + L.oW1, *b1 = w + L.ob1, *W2 = w + L.oW2,
                  *b2 = w + L.ob2, *W3T = w + L.oW3, *b3 = w + L.ob3, *W4T = w + L.oW4, *b4 = w + L.ob4;

    // ---- set-up ----
    lds_copy_T(w + L.oWin, p.Win, D, F, 0, F, F);
    lds_copy(w + L.obin, p.bin, D);
    lds_copy_T(w + L.oW1, p.W1, D, 2 * C, 0, C, LDH);
    lds_copy_T(w + L.oW1 + LDH * D, p.W1, D, 2 * C, C, C, LDH);
    lds_copy(w + L.ob1, p.b1, D);
    lds_copy(w + L.oW2, p.W2, D);
    lds_copy(w + L.ob2, p.b2, 1);
    if (T > 0) {
        for (int blk = 0; blk < 3; ++blk) lds_copy_T(w + L.oW3 + blk * LDH * D, p.W3, D, 3 * C, blk * C, C, LDH);
        lds_copy(w + L.ob3, p.b3, D);
        lds_copy_T(w + L.oW4, p.W4, D, D, 0, D, D);
        lds_copy(w + L.ob4, p.b4, D);
    }
    lds_copy(sTt, tanh_table, nt);
    lds_copy(sTs, sigmoid_table, nt);
    if (threadIdx.x == 0) *total = 0;
    // (a graph of no hits - a padded batch's empty graph owns padded segments only - has no lists: in_ptr[h0] may lie
    // behind the arrays)
    if (nh > 0) ev_local_lists<NT>(g, h0, nh, s0, ids);
    ev_local_ends<NT>(g, h0, s0, ns, ids);
    for (int i = threadIdx.x; i < nh * (LDH - D); i += NT) {
        const int n = i / (LDH - D), k = i - n * (LDH - D);
        const int32_t x = k < F ? fx_quant(g.X[(int64_t)(h0 + n) * F + k], scale, f) : 0;
        H[n * LDH + D + k] = x;
        Hn[n * LDH + D + k] = x;
    }
    __syncthreads();

    long long mine = 0;         // this lane's overflows, all stages and passes
    // ---- input network ----
    {
        int over = 0;
        for (int i = threadIdx.x; i < nh * D; i += NT) {
            const int n = i / D, d = i - n * D;
            const int32_t *x = H + n * LDH + D;
            int64_t acc = (int64_t)bin[d] << f.Fb;
#pragma unroll
            for (int k = 0; k < F; ++k) acc += (int64_t)WinT[k * D + d] * x[k];
            H[n * LDH + d] = fx_tanh(sTt, fx_requant(acc, f, over), f);
        }
        mine += over;
        fx_count(over, counts);
    }
    __syncthreads();

    // acc += sum_k wT[k][d] * row[k] over one zero-padded row of LDH words (16-byte pieces, the same address in the D
    // lanes of a hit)
    auto row_mac = [](int64_t acc, const int32_t *wT, const int32_t *row) {
        const int4 *r4 = reinterpret_cast<const int4 *>(row);
#pragma unroll
        for (int k4 = 0; k4 < G; ++k4) {
            const int4 h = r4[k4];
            const int32_t *wk = wT + 4 * k4 * D;
            acc += (int64_t)wk[0] * h.x;
            acc += (int64_t)wk[D] * h.y;
            acc += (int64_t)wk[2 * D] * h.z;
            acc += (int64_t)wk[3 * D] * h.w;
        }
        return acc;
    };

    const int64_t N = g.n_hits, E = g.n_segments;
    for (int t = 0;; ++t) {
        int64_t *row = counts + (size_t)t * GNN_FX_STAGES;
        const bool last = t == T;
        if (H_trace)
            for (int i = threadIdx.x; i < nh * C; i += NT) {
                const int n = i / C, c = i - n * C;
                H_trace[((int64_t)t * N + h0 + n) * C + c] = H[n * LDH + c];
            }
        // ---- the per-hit halves of the edge network's first layer ----
        if (ns > 0)
            for (int i = threadIdx.x; i < nh * 2 * D; i += NT) {
                const int n = i / (2 * D), u = i - n * (2 * D);
                const int half = u >= D, d = u - half * D;
                PQ[i] = row_mac(half ? 0 : (int64_t)b1[d] << f.Fb, W1T + half * LDH * D + d, H + n * LDH);
            }
        __syncthreads();
        // ---- edge network: one segment per lane ----
        {
            int over1 = 0, over2 = 0;
            for (int j = threadIdx.x; j < ns; j += NT) {
                const int s = ids.sl[j], d = ids.dl[j];
                int64_t acc = (int64_t)b2[0] << f.Fb;
                if (s >= 0) {
                    const int64_t *P = PQ + s * 2 * D, *Q = PQ + d * 2 * D + D;
#pragma unroll 4
                    for (int k = 0; k < D; ++k)
                        acc += (int64_t)W2[k] * fx_tanh(sTt, fx_requant(P[k] + Q[k], f, over1), f);
                } else {        // a padded segment: zero rows, so the first layer sees its bias alone
#pragma unroll 4
                    for (int k = 0; k < D; ++k)
                        acc += (int64_t)W2[k] * fx_tanh(sTt, fx_requant((int64_t)b1[k] << f.Fb, f, over1), f);
                }
                const int32_t e = fx_sigmoid(sTs, fx_requant(acc, f, over2), f);
                es[j] = e;
                if (e_trace) e_trace[(int64_t)t * E + s0 + j] = e;
                if (last) {
                    e_raw[s0 + j] = e;
                    e_float[s0 + j] = (float)e * inv_scale;      // |e| < 2^24 and a power of two: exact
                }
            }
            mine += over1 + over2;
            fx_count(over1, row + 1);
            fx_count(over2, row + 2);
        }
        if (last) break;
        __syncthreads();
        // ---- aggregate: a lane owns 4 columns of mi or of mo of one hit and pulls its list ----
        {
            int over = 0;
            for (int i = threadIdx.x; i < nh * 2 * G; i += NT) {
                const int n = i / (2 * G), r = i - n * (2 * G);
                const int side = r >= G, c4 = r - side * G;
                const int32_t *ptr = side ? ids.op : ids.ip, *eid = side ? ids.oe : ids.ie, *nbr = side ? ids.onb : ids.inb;
                int64_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
                const int k1 = ptr[n + 1];
                for (int k = ptr[n]; k < k1; ++k) {
                    const int64_t wgt = es[eid[k]];
                    const int4 v = reinterpret_cast<const int4 *>(H + nbr[k] * LDH)[c4];
                    a0 += wgt * v.x;
                    a1 += wgt * v.y;
                    a2 += wgt * v.z;
                    a3 += wgt * v.w;
                }
                reinterpret_cast<int4 *>(M + n * 2 * LDH + side * LDH)[c4] =
                    make_int4(fx_requant(a0, f, over), fx_requant(a1, f, over), fx_requant(a2, f, over),
                              fx_requant(a3, f, over));
            }
            mine += over;
            fx_count(over, row + 3);
        }
        __syncthreads();
        // ---- node network, layer 1 ----
        {
            int over = 0;
            for (int i = threadIdx.x; i < nh * D; i += NT) {
                const int n = i / D, d = i - n * D;
                int64_t acc = (int64_t)b3[d] << f.Fb;
                acc = row_mac(acc, W3T + d, M + n * 2 * LDH);
                acc = row_mac(acc, W3T + LDH * D + d, M + n * 2 * LDH + LDH);
                acc = row_mac(acc, W3T + 2 * LDH * D + d, H + n * LDH);
                q[i] = fx_tanh(sTt, fx_requant(acc, f, over), f);
            }
            mine += over;
            fx_count(over, row + 4);
        }
        __syncthreads();
        // ---- node network, layer 2 (the skip columns of Hn hold x since the set-up: gnn/model.py:154) ----
        {
            int over = 0;
            for (int i = threadIdx.x; i < nh * D; i += NT) {
                const int n = i / D, d = i - n * D;
                const int4 *q4 = reinterpret_cast<const int4 *>(q + n * D);
                int64_t acc = (int64_t)b4[d] << f.Fb;
#pragma unroll 4
                for (int k4 = 0; k4 < D / 4; ++k4) {
                    const int4 v = q4[k4];
                    const int32_t *wk = W4T + 4 * k4 * D + d;
                    acc += (int64_t)wk[0] * v.x;
                    acc += (int64_t)wk[D] * v.y;
                    acc += (int64_t)wk[2 * D] * v.z;
                    acc += (int64_t)wk[3 * D] * v.w;
                }
                Hn[n * LDH + d] = fx_tanh(sTt, fx_requant(acc, f, over), f);
            }
            mine += over;
            fx_count(over, row + 5);
        }
        __syncthreads();
        int32_t *sw = H;
        H = Hn;
        Hn = sw;
    }

    // ---- the graph's total ----
    if (graph_overflows) {              // (uniform)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
        if ((threadIdx.x & 63) == 0 && mine) atomicAdd(total, (unsigned long long)mine);
        __syncthreads();
        if (threadIdx.x == 0) graph_overflows[b] = (int64_t)*total;
    }
}

template <int F, int D>
int run_fx_events(const gnn_graph_t *g, const gnn_fx_params_t *p, const Fx &f, const gnn_fx_tables_t *tb,
                  const int32_t *hit_ptr, const int32_t *seg_ptr, int64_t n_graphs, int cap_h, int cap_s, int T,
                  int32_t *e_raw, float *e_float, int64_t *counts, int64_t *graph_overflows, int32_t *e_trace,
                  int32_t *H_trace, hipStream_t s)
{
    ProfChain chain;
    hipError_t err = hipMemsetAsync(counts, 0, (size_t)(T + 1) * GNN_FX_STAGES * sizeof(int64_t), s);
    if (err != hipSuccess) return fail(-(int)err, "memset of the overflow counters failed");
    if (n_graphs <= 0) return 0;
    static DevOnce attr_done;     // dynamic LDS above 64 KB must be opted into, once per device
    if (attr_done.need())
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_fx_event<F, D>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFxEvLdsMax);
    const size_t lds = 4 * fxev_words(F, D, f.tb, cap_h, cap_s);
    const float scale = (float)(1 << f.Fb), inv_scale = 1.0f / scale;
    GNN_LAUNCH_SH("k_fx_event", (k_fx_event<F, D>), (unsigned)n_graphs, EvCfg<D>::NT, lds, s, *g, *p, tb->tanh_table,
                  tb->sigmoid_table, f, scale, inv_scale, hit_ptr, seg_ptr, cap_h, cap_s, T, e_raw, e_float, counts,
                  graph_overflows, e_trace, H_trace);
    return 0;
}

}  // namespace

using namespace gnn;

extern "C" {

size_t gnn_fxev_lds_bytes(int32_t F, int32_t D, int32_t table_bits, int64_t max_hits, int64_t max_segments)
{
    if (!gnn_shape_supported(F, D) || table_bits < 4 || table_bits > 12 || max_hits < 0 || max_segments < 0 ||
        max_hits > INT32_MAX || max_segments > INT32_MAX)
        return 0;
    return 4 * fxev_words(F, D, table_bits, max_hits, max_segments);
}

int gnn_fxev_supported(int32_t F, int32_t D, int32_t table_bits, int64_t max_hits, int64_t max_segments)
{
    const size_t need = gnn_fxev_lds_bytes(F, D, table_bits, max_hits, max_segments);
    return need > 0 && need <= kFxEvLdsMax;
}

int gnn_fxev_forward(const gnn_graph_t *g, const gnn_fx_params_t *p, const gnn_fx_format_t *fmt,
                     const gnn_fx_tables_t *tables, const int32_t *hit_ptr, const int32_t *seg_ptr, int64_t n_graphs,
                     int32_t max_hits, int32_t max_segments, int32_t n_iters, int32_t *e_raw, float *e_float,
                     int64_t *counts, int64_t *graph_overflows, int32_t *e_trace, int32_t *H_trace, void *stream)
{
    if (!g || !p || !fmt || !tables) return fail(GNN_ERR_BADARG, "gnn_fxev_forward: null graph, params, format or tables");
    if (n_graphs < 0 || n_graphs > INT32_MAX) return fail(GNN_ERR_BADARG, "gnn_fxev_forward: n_graphs must be in [0, 2^31)");
    if (n_iters < 0) return fail(GNN_ERR_BADARG, "gnn_fxev_forward: n_iters must be >= 0");
    if (max_hits < 0 || max_segments < 0)
        return fail(GNN_ERR_BADARG, "gnn_fxev_forward: max_hits and max_segments must be >= 0");
    const int64_t N = g->n_hits, E = g->n_segments;
    if (N < 0 || E < 0 || N > INT32_MAX || E > INT32_MAX)
        return fail(GNN_ERR_BADARG, "gnn_fxev_forward: n_hits and n_segments must be in [0, 2^31)");
    if (fmt->rounding != GNN_FX_TRN && fmt->rounding != GNN_FX_RND)
        return fail(GNN_ERR_BADARG, "gnn_fxev_forward: rounding must be GNN_FX_TRN or GNN_FX_RND");
    if (fmt->overflow != GNN_FX_WRAP && fmt->overflow != GNN_FX_SAT)
        return fail(GNN_ERR_BADARG, "gnn_fxev_forward: overflow must be GNN_FX_WRAP or GNN_FX_SAT");
    if (!gnn_fx_supported(p->F, p->D, fmt->total_bits, fmt->int_bits, fmt->table_bits))
        return fail(GNN_ERR_UNSUPPORTED, "gnn_fxev_forward: no kernel for input_dim=%d hidden_dim=%d, or a format outside "
                    "total_bits 4..24, int_bits 2..total_bits, table_bits 4..12 (got %d, %d, %d)", p->F, p->D,
                    fmt->total_bits, fmt->int_bits, fmt->table_bits);
    if (!gnn_fxev_supported(p->F, p->D, fmt->table_bits, max_hits, max_segments))
        return fail(GNN_ERR_UNSUPPORTED, "gnn_fxev_forward: graphs of up to %d hits / %d segments need %zu bytes of LDS at "
                    "input_dim=%d hidden_dim=%d table_bits=%d, a workgroup has %zu", max_hits, max_segments,
                    gnn_fxev_lds_bytes(p->F, p->D, fmt->table_bits, max_hits, max_segments), p->F, p->D, fmt->table_bits,
                    kFxEvLdsMax);
    if (!p->Win || !p->bin || !p->W1 || !p->b1 || !p->W2 || !p->b2 || !p->W3 || !p->b3 || !p->W4 || !p->b4)
        return fail(GNN_ERR_BADARG, "gnn_fxev_forward: a weight pointer is null");
    if (!tables->tanh_table || !tables->sigmoid_table) return fail(GNN_ERR_BADARG, "gnn_fxev_forward: a table pointer is null");
    if (!counts) return fail(GNN_ERR_BADARG, "gnn_fxev_forward: counts is null");
    if (n_graphs > 0 && (!hit_ptr || !seg_ptr)) return fail(GNN_ERR_BADARG, "gnn_fxev_forward: hit_ptr or seg_ptr is null");
    if (n_graphs == 0 && (N > 0 || E > 0))
        return fail(GNN_ERR_BADARG, "gnn_fxev_forward: n_graphs is 0 but the batch has hits or segments");
    if (N > 0 && (!g->X || !g->in_ptr || !g->out_ptr)) return fail(GNN_ERR_BADARG, "gnn_fxev_forward: X, in_ptr or out_ptr is null");
    if (E > 0 && (!g->src || !g->dst || !e_raw || !e_float))
        return fail(GNN_ERR_BADARG, "gnn_fxev_forward: src, dst, e_raw or e_float is null");
    if (E > 0 && N > 0 && (!g->in_eid || !g->in_nbr || !g->out_eid || !g->out_nbr))
        return fail(GNN_ERR_BADARG, "gnn_fxev_forward: a segment list is null");
    const Fx f = fx_of(*fmt);
    return ModelShapes::find<int>(p->F, p->D, GNN_ERR_UNSUPPORTED, [&](auto sh) {      // (gnn_fx_supported: the shape is listed)
        return run_fx_events<sh.F, sh.D>(g, p, f, tables, hit_ptr, seg_ptr, n_graphs, max_hits, max_segments, n_iters,
                                         e_raw, e_float, counts, graph_overflows, e_trace, H_trace,
                                         static_cast<hipStream_t>(stream)); });
}

}  // extern "C"
