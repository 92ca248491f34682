// fixed_point.hip - the fixed-point forward of SegmentClassifier (include/gnn_hip_fixed.h): gnn/model.py:140-156 in
// two's-complement words of a chosen width, as an HLS design would run it.
//
// One kernel per reference module, over the lists of gnn_graph_t, as the float per-module path of gnn_kernels.hip:
//   k_fx_input   X -> x = quant(X), H0 = [T_tanh[requant(Win x + bin)] | x | 0]              (gnn/model.py:144-146)
//   k_fx_pq      per hit P = W1[:, :C] h + (b1 << Fb), Q = W1[:, C:] h, exact int64          (gnn/model.py:71-73,46)
//   k_fx_edge    per segment z1 = requant(P[src] + Q[dst]), e = T_sig[requant(W2 T_tanh[z1] + b2)]  (gnn/model.py:81)
//   k_fx_agg     per hit mi = requant(sum e_j H[src j]) over its in list, mo over its out list      (gnn/model.py:114-119)
//   k_fx_mlp     per hit H' = T_tanh[requant(W4 T_tanh[requant(W3 [mi|mo|h] + b3)] + b4)], [H' | x]  (gnn/model.py:120-125,154)
// Every sum is an int64 sum of int32 x int32 products (v_mad_i64_i32), so no order or split of a sum changes a bit:
// the per-hit halves P / Q stand for W1 [H_s | H_d], and the lanes of k_fx_agg split a row by columns.
//
// Weights and tables live in LDS, weights of the layers that stream their inputs TRANSPOSED ([k][d]: the D products of
// one input value read D consecutive words, the same address in every lane - a broadcast, 16 bytes at a time) and
// zero-padded to the hit rows' stride, so that the loops run over whole 16-byte pieces of a row.  A lane keeps one
// hit's D accumulators (2 D registers) and never its 3 C inputs: at hidden_dim 64 that is 128 + 64 registers
// against 400 for the register-resident form of k_node.  The node MLP's LDS is 3 LDH D + D D + 2^tb + 2 D words: 85 KB
// at (4, 64) with 12 table bits, one workgroup per CU; every other kernel stays under 64 KB.
//
// The overflow counters are the only atomics: a lane counts in a register, a wave adds its lanes by shuffles and lane
// 0 issues one 64-bit atomic add per stage with a non-zero count.
#include "common.h"
#include "fixed_ops.h"
#include "gnn_hip_fixed.h"

#include <algorithm>

namespace {
using namespace gnn;

// acc[d] += wT[k][d] * row[k] over one zero-padded row of LDH int32 (16-byte aligned), wT in LDS [LDH][D]
template <int LDH, int D>
__device__ __forceinline__ void fx_row_mac(int64_t (&acc)[D], const int32_t *wT, const int32_t *__restrict__ row)
{
    const int4 *r4 = reinterpret_cast<const int4 *>(row);
#pragma unroll 1
    for (int k4 = 0; k4 < LDH / 4; ++k4) {
        const int4 h = r4[k4];
        const int32_t hv[4] = {h.x, h.y, h.z, h.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int32_t *w = wT + (4 * k4 + u) * D;
#pragma unroll
            for (int d = 0; d < D; ++d) acc[d] += (int64_t)w[d] * hv[u];
        }
    }
}

extern __shared__ __attribute__((aligned(16))) char fx_smem[];

// -------------------------------------------------------------------------------------------------------------------
// LDS words of each kernel (host and device agree through these)
constexpr int fx_input_words(int F, int D, int tb) { return D * F + D + (1 << tb); }
constexpr int fx_pq_words(int LDH, int D) { return 2 * LDH * D + D; }
constexpr int fx_edge_words(int D, int tb) { return 2 * (1 << tb) + 2 * D + 4; }
constexpr int fx_mlp_words(int LDH, int D, int tb) { return 3 * LDH * D + D * D + 2 * D + (1 << tb); }

template <int F, int D>
__global__ __launch_bounds__(kBlock) void k_fx_input(const float *__restrict__ X, const int32_t *__restrict__ Win,
                                                     const int32_t *__restrict__ bin,
                                                     const int32_t *__restrict__ tanh_table, Fx f, float scale,
                                                     int32_t *__restrict__ H, int64_t n_hits, int64_t *counter)
{
    constexpr int LDH = Shape<F, D>::LDH;
    int32_t *sWin = reinterpret_cast<int32_t *>(fx_smem), *sbin = sWin + D * F, *sT = sbin + D;
    lds_copy(sWin, Win, D * F);
    lds_copy(sbin, bin, D);
    lds_copy(sT, tanh_table, 1 << f.tb);
    __syncthreads();
    int over = 0;
    for (int64_t n = (int64_t)blockIdx.x * kBlock + threadIdx.x; n < n_hits; n += (int64_t)gridDim.x * kBlock) {
        int32_t x[F];
#pragma unroll
        for (int k = 0; k < F; ++k) x[k] = fx_quant(X[n * F + k], scale, f);
        int4 *row = reinterpret_cast<int4 *>(H + n * LDH);
#pragma unroll 1
        for (int d4 = 0; d4 < D / 4; ++d4) {
            int32_t o[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int d = 4 * d4 + u;
                int64_t acc = (int64_t)sbin[d] << f.Fb;
#pragma unroll
                for (int k = 0; k < F; ++k) acc += (int64_t)sWin[d * F + k] * x[k];
                o[u] = fx_tanh(sT, fx_requant(acc, f, over), f);
            }
            row[d4] = make_int4(o[0], o[1], o[2], o[3]);
        }
        int32_t tail[LDH - D];
#pragma unroll
        for (int k = 0; k < LDH - D; ++k) tail[k] = k < F ? x[k] : 0;
#pragma unroll
        for (int v = 0; v < (LDH - D) / 4; ++v)
            row[D / 4 + v] = make_int4(tail[4 * v], tail[4 * v + 1], tail[4 * v + 2], tail[4 * v + 3]);
    }
    fx_count(over, counter);
}

template <int F, int D>
__global__ __launch_bounds__(kBlock) void k_fx_pq(const int32_t *__restrict__ H, const int32_t *__restrict__ W1,
                                                  const int32_t *__restrict__ b1, Fx f, int64_t *__restrict__ PQ,
                                                  int64_t n_hits)
{
    constexpr int C = Shape<F, D>::C, LDH = Shape<F, D>::LDH;
    int32_t *sW = reinterpret_cast<int32_t *>(fx_smem), *sb = sW + 2 * LDH * D;
    lds_copy_T(sW, W1, D, 2 * C, 0, C, LDH);
    lds_copy_T(sW + LDH * D, W1, D, 2 * C, C, C, LDH);
    lds_copy(sb, b1, D);
    __syncthreads();
    for (int64_t n = (int64_t)blockIdx.x * kBlock + threadIdx.x; n < n_hits; n += (int64_t)gridDim.x * kBlock) {
#pragma unroll 1
        for (int half = 0; half < 2; ++half) {
            int64_t acc[D];
#pragma unroll
            for (int d = 0; d < D; ++d) acc[d] = half ? 0 : (int64_t)sb[d] << f.Fb;
            fx_row_mac<LDH, D>(acc, sW + half * LDH * D, H + n * LDH);
            longlong2 *o = reinterpret_cast<longlong2 *>(PQ + n * 2 * D + half * D);
#pragma unroll
            for (int v = 0; v < D / 2; ++v) o[v] = make_longlong2(acc[2 * v], acc[2 * v + 1]);
        }
    }
}

template <int D>
__global__ __launch_bounds__(kBlock) void k_fx_edge(const int32_t *__restrict__ src, const int32_t *__restrict__ dst,
                                                    const int64_t *__restrict__ PQ, const int32_t *__restrict__ b1,
                                                    const int32_t *__restrict__ W2, const int32_t *__restrict__ b2,
                                                    const int32_t *__restrict__ tanh_table,
                                                    const int32_t *__restrict__ sigmoid_table, Fx f, float inv_scale,
                                                    int32_t *__restrict__ e_a, int32_t *__restrict__ e_b,
                                                    float *__restrict__ e_float, int64_t n_segments, int64_t *counters)
{
    const int nt = 1 << f.tb;
    int32_t *sTt = reinterpret_cast<int32_t *>(fx_smem), *sTs = sTt + nt, *sW2 = sTs + nt, *sb1 = sW2 + D, *sb2 = sb1 + D;
    lds_copy(sTt, tanh_table, nt);
    lds_copy(sTs, sigmoid_table, nt);
    lds_copy(sW2, W2, D);
    lds_copy(sb1, b1, D);
    lds_copy(sb2, b2, 1);
    __syncthreads();
    int over1 = 0, over2 = 0;
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < n_segments; j += (int64_t)gridDim.x * kBlock) {
        const int s = src[j], d = dst[j];
        int64_t acc = (int64_t)sb2[0] << f.Fb;
        if (s >= 0) {
            const longlong2 *p = reinterpret_cast<const longlong2 *>(PQ + (int64_t)s * 2 * D);
            const longlong2 *q = reinterpret_cast<const longlong2 *>(PQ + (int64_t)d * 2 * D + D);
#pragma unroll 4
            for (int v = 0; v < D / 2; ++v) {
                const longlong2 a = p[v], b = q[v];
                acc += (int64_t)sW2[2 * v] * fx_tanh(sTt, fx_requant(a.x + b.x, f, over1), f);
                acc += (int64_t)sW2[2 * v + 1] * fx_tanh(sTt, fx_requant(a.y + b.y, f, over1), f);
            }
        } else {            // a padded segment: zero rows, so the first layer sees its bias alone
#pragma unroll 4
            for (int k = 0; k < D; ++k)
                acc += (int64_t)sW2[k] * fx_tanh(sTt, fx_requant((int64_t)sb1[k] << f.Fb, f, over1), f);
        }
        const int32_t e = fx_sigmoid(sTs, fx_requant(acc, f, over2), f);
        e_a[j] = e;
        if (e_b) e_b[j] = e;
        if (e_float) e_float[j] = (float)e * inv_scale;      // |e| < 2^24 and a power of two: exact
    }
    fx_count(over1, counters + 1);
    fx_count(over2, counters + 2);
}

// LDH / 4 lanes per hit, lane p owns columns 4 p .. 4 p + 3 of mi and of mo
template <int LDH>
__global__ __launch_bounds__(kBlock) void k_fx_agg(const int32_t *__restrict__ H, const int32_t *__restrict__ e,
                                                   const int32_t *__restrict__ in_ptr, const int32_t *__restrict__ in_eid,
                                                   const int32_t *__restrict__ in_nbr, const int32_t *__restrict__ out_ptr,
                                                   const int32_t *__restrict__ out_eid,
                                                   const int32_t *__restrict__ out_nbr, Fx f, int32_t *__restrict__ M,
                                                   int64_t n_hits, int64_t *counter)
{
    constexpr int G = LDH / 4;
    int over = 0;
    const int64_t total = n_hits * G;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += (int64_t)gridDim.x * kBlock) {
        const int64_t n = t / G;
        const int p = (int)(t - n * G);
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const int32_t *ptr = side ? out_ptr : in_ptr, *eid = side ? out_eid : in_eid, *nbr = side ? out_nbr : in_nbr;
            int64_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
            const int k1 = ptr[n + 1];
            for (int k = ptr[n]; k < k1; ++k) {
                const int64_t w = e[eid[k]];
                const int4 r = reinterpret_cast<const int4 *>(H + (int64_t)nbr[k] * LDH)[p];
                a0 += w * r.x;
                a1 += w * r.y;
                a2 += w * r.z;
                a3 += w * r.w;
            }
            reinterpret_cast<int4 *>(M + n * 2 * LDH + side * LDH)[p] =
                make_int4(fx_requant(a0, f, over), fx_requant(a1, f, over), fx_requant(a2, f, over),
                          fx_requant(a3, f, over));
        }
    }
    fx_count(over, counter);
}

template <int F, int D>
__global__ __launch_bounds__(kBlock) void k_fx_mlp(const int32_t *__restrict__ H, const int32_t *__restrict__ M,
                                                   const int32_t *__restrict__ W3, const int32_t *__restrict__ b3,
                                                   const int32_t *__restrict__ W4, const int32_t *__restrict__ b4,
                                                   const int32_t *__restrict__ tanh_table, Fx f,
                                                   int32_t *__restrict__ Hn, int64_t n_hits, int64_t *counters)
{
    constexpr int C = Shape<F, D>::C, LDH = Shape<F, D>::LDH;
    int32_t *sW3 = reinterpret_cast<int32_t *>(fx_smem), *sW4 = sW3 + 3 * LDH * D, *sb3 = sW4 + D * D, *sb4 = sb3 + D,
            *sT = sb4 + D;
    for (int b = 0; b < 3; ++b) lds_copy_T(sW3 + b * LDH * D, W3, D, 3 * C, b * C, C, LDH);
    lds_copy(sW4, W4, D * D);
    lds_copy(sb3, b3, D);
    lds_copy(sb4, b4, D);
    lds_copy(sT, tanh_table, 1 << f.tb);
    __syncthreads();
    int over3 = 0, over4 = 0;
    for (int64_t n = (int64_t)blockIdx.x * kBlock + threadIdx.x; n < n_hits; n += (int64_t)gridDim.x * kBlock) {
        int64_t acc[D];
#pragma unroll
        for (int d = 0; d < D; ++d) acc[d] = (int64_t)sb3[d] << f.Fb;
        fx_row_mac<LDH, D>(acc, sW3, M + n * 2 * LDH);
        fx_row_mac<LDH, D>(acc, sW3 + LDH * D, M + n * 2 * LDH + LDH);
        fx_row_mac<LDH, D>(acc, sW3 + 2 * LDH * D, H + n * LDH);
        int32_t q[D];
#pragma unroll
        for (int d = 0; d < D; ++d) q[d] = fx_tanh(sT, fx_requant(acc[d], f, over3), f);
        int4 *row = reinterpret_cast<int4 *>(Hn + n * LDH);
#pragma unroll 1
        for (int d4 = 0; d4 < D / 4; ++d4) {
            int32_t o[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int d = 4 * d4 + u;
                int64_t a = (int64_t)sb4[d] << f.Fb;
#pragma unroll
                for (int k = 0; k < D; ++k) a += (int64_t)sW4[d * D + k] * q[k];
                o[u] = fx_tanh(sT, fx_requant(a, f, over4), f);
            }
            row[d4] = make_int4(o[0], o[1], o[2], o[3]);
        }
        const int4 *old = reinterpret_cast<const int4 *>(H + n * LDH);       // skip concat of x (gnn/model.py:154)
#pragma unroll
        for (int v = D / 4; v < LDH / 4; ++v) row[v] = old[v];
    }
    fx_count(over3, counters + 4);
    fx_count(over4, counters + 5);
}

// H (padded rows) -> one unpadded trace row [N, C]
__global__ __launch_bounds__(kBlock) void k_fx_unpad(const int32_t *__restrict__ H, int ldh, int C,
                                                     int32_t *__restrict__ out, int64_t total)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock)
        out[i] = H[(i / C) * ldh + i % C];
}

// -------------------------------------------------------------------------------------------------------------------
struct FxWs {
    int32_t *Ha, *Hb, *M, *e;
    int64_t *PQ;
    size_t bytes;
};
FxWs carve_fx(char *ws, int64_t N, int64_t E, int F, int D)
{
    const int64_t ldh = (F + D + 3) & ~3;
    Carver c{ws};
    FxWs w;
    w.Ha = c.take<int32_t>((size_t)N * ldh);
    w.Hb = c.take<int32_t>((size_t)N * ldh);
    w.M = c.take<int32_t>((size_t)N * 2 * ldh);
    w.e = c.take<int32_t>((size_t)E);
    w.PQ = c.take<int64_t>((size_t)N * 2 * D);
    w.bytes = c.bytes();
    return w;
}

// grid-stride launches: enough workgroups to fill the chip `per_cu` times over, never more than the work.  A workgroup
// fills its LDS (up to 85 KB of weights and tables) before its first item, so the kernels that keep a layer there take
// few workgroups and many items each; the segment and column kernels (tables only, or no LDS) take more
constexpr int kHitBlocksPerCu = 2, kItemBlocksPerCu = 4;
unsigned fx_grid(int64_t items, int per_cu)
{
    const int64_t want = (items + kBlock - 1) / kBlock, cap = (int64_t)device_cus() * per_cu;
    return (unsigned)std::max<int64_t>(1, std::min(want, cap));
}

constexpr size_t kFxLdsMax = 160 * 1024;

template <int F, int D>
int fx_forward_impl(const gnn_graph_t *g, const gnn_fx_params_t *p, const Fx &f, const gnn_fx_tables_t *tb, int T,
                    int32_t *e_raw, float *e_float, int64_t *counts, int32_t *e_trace, int32_t *H_trace, char *ws,
                    hipStream_t s)
{
    constexpr int C = Shape<F, D>::C, LDH = Shape<F, D>::LDH;
    ProfChain chain;
    const int64_t N = g->n_hits, E = g->n_segments;
    const FxWs w = carve_fx(ws, N, E, F, D);
    const float scale = (float)(1 << f.Fb), inv_scale = 1.0f / scale;
    const size_t lds_in = 4 * (size_t)fx_input_words(F, D, f.tb), lds_pq = 4 * (size_t)fx_pq_words(LDH, D),
                 lds_edge = 4 * (size_t)fx_edge_words(D, f.tb), lds_mlp = 4 * (size_t)fx_mlp_words(LDH, D, f.tb);
    static DevOnce attr_done;     // dynamic LDS above 64 KB must be opted into, once per device
    if (attr_done.need())
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_fx_mlp<F, D>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFxLdsMax);
    hipError_t err = hipMemsetAsync(counts, 0, (size_t)(T + 1) * GNN_FX_STAGES * sizeof(int64_t), s);
    if (err != hipSuccess) return fail(-(int)err, "memset of the overflow counters failed");

    const unsigned g_hit = fx_grid(N, kHitBlocksPerCu), g_seg = fx_grid(E, kItemBlocksPerCu),
                   g_col = fx_grid(N * (LDH / 4), kItemBlocksPerCu), g_unpad = fx_grid(N * C, kItemBlocksPerCu);
    int32_t *H = w.Ha, *Hn = w.Hb;
    if (N > 0)
        GNN_LAUNCH_SH("k_fx_input", (k_fx_input<F, D>), g_hit, kBlock, lds_in, s, g->X, p->Win, p->bin, tb->tanh_table, f,
                      scale, H, N, counts);
    for (int t = 0;; ++t) {
        int64_t *row = counts + (size_t)t * GNN_FX_STAGES;
        if (H_trace && N > 0)
            GNN_LAUNCH("k_fx_unpad", k_fx_unpad, g_unpad, kBlock, s, H, LDH, C, H_trace + (size_t)t * N * C, N * C);
        const bool last = t == T;
        if (N > 0 && E > 0)
            GNN_LAUNCH_SH("k_fx_pq", (k_fx_pq<F, D>), g_hit, kBlock, lds_pq, s, H, p->W1, p->b1, f, w.PQ, N);
        if (E > 0)
            GNN_LAUNCH_SH("k_fx_edge", (k_fx_edge<D>), g_seg, kBlock, lds_edge, s, g->src, g->dst, w.PQ, p->b1, p->W2,
                          p->b2, tb->tanh_table, tb->sigmoid_table, f, inv_scale, last ? e_raw : w.e,
                          e_trace ? e_trace + (size_t)t * E : nullptr, last ? e_float : nullptr, E, row);
        if (last) break;
        if (N > 0) {
            GNN_LAUNCH("k_fx_agg", (k_fx_agg<LDH>), g_col, kBlock, s, H, w.e, g->in_ptr, g->in_eid, g->in_nbr, g->out_ptr,
                       g->out_eid, g->out_nbr, f, w.M, N, row + 3);
            GNN_LAUNCH_SH("k_fx_mlp", (k_fx_mlp<F, D>), g_hit, kBlock, lds_mlp, s, H, w.M, p->W3, p->b3, p->W4, p->b4,
                          tb->tanh_table, f, Hn, N, row);
        }
        std::swap(H, Hn);
    }
    return 0;
}

}  // namespace

using namespace gnn;

extern "C" {

int gnn_fx_supported(int32_t F, int32_t D, int32_t total_bits, int32_t int_bits, int32_t table_bits)
{
    if (!gnn_shape_supported(F, D) || !fx_format_ok(total_bits, int_bits, table_bits)) return 0;
    const int ldh = (F + D + 3) & ~3;
    return 4 * (size_t)fx_mlp_words(ldh, D, table_bits) <= kFxLdsMax;
}

size_t gnn_fx_workspace_bytes(int64_t n_hits, int64_t n_segments, int32_t F, int32_t D)
{
    if (n_hits < 0 || n_segments < 0 || n_hits > INT32_MAX || n_segments > INT32_MAX) {
        fail(GNN_ERR_BADARG, "gnn_fx_workspace_bytes: n_hits and n_segments must be in [0, 2^31)");
        return 0;
    }
    if (!gnn_shape_supported(F, D)) {
        fail(GNN_ERR_UNSUPPORTED, "no fixed-point kernel for input_dim=%d hidden_dim=%d", F, D);
        return 0;
    }
    return carve_fx(nullptr, n_hits, n_segments, F, D).bytes;
}

int gnn_fx_forward(const gnn_graph_t *g, const gnn_fx_params_t *p, const gnn_fx_format_t *fmt,
                   const gnn_fx_tables_t *tables, int32_t n_iters, int32_t *e_raw, float *e_float, int64_t *counts,
                   int32_t *e_trace, int32_t *H_trace, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!g || !p || !fmt || !tables) return fail(GNN_ERR_BADARG, "gnn_fx_forward: null graph, params, format or tables");
    if (n_iters < 0) return fail(GNN_ERR_BADARG, "gnn_fx_forward: n_iters must be >= 0");
    const int64_t N = g->n_hits, E = g->n_segments;
    if (N < 0 || E < 0 || N > INT32_MAX || E > INT32_MAX)
        return fail(GNN_ERR_BADARG, "gnn_fx_forward: n_hits and n_segments must be in [0, 2^31)");
    if (fmt->rounding != GNN_FX_TRN && fmt->rounding != GNN_FX_RND)
        return fail(GNN_ERR_BADARG, "gnn_fx_forward: rounding must be GNN_FX_TRN or GNN_FX_RND");
    if (fmt->overflow != GNN_FX_WRAP && fmt->overflow != GNN_FX_SAT)
        return fail(GNN_ERR_BADARG, "gnn_fx_forward: overflow must be GNN_FX_WRAP or GNN_FX_SAT");
    if (!gnn_fx_supported(p->F, p->D, fmt->total_bits, fmt->int_bits, fmt->table_bits))
        return fail(GNN_ERR_UNSUPPORTED, "gnn_fx_forward: no kernel for input_dim=%d hidden_dim=%d, or a format outside "
                    "total_bits 4..24, int_bits 2..total_bits, table_bits 4..12 (got %d, %d, %d)", p->F, p->D,
                    fmt->total_bits, fmt->int_bits, fmt->table_bits);
    if (!p->Win || !p->bin || !p->W1 || !p->b1 || !p->W2 || !p->b2 || !p->W3 || !p->b3 || !p->W4 || !p->b4)
        return fail(GNN_ERR_BADARG, "gnn_fx_forward: a weight pointer is null");
    if (!tables->tanh_table || !tables->sigmoid_table) return fail(GNN_ERR_BADARG, "gnn_fx_forward: a table pointer is null");
    if (!counts) return fail(GNN_ERR_BADARG, "gnn_fx_forward: counts is null");
    if (N > 0 && (!g->X || !g->in_ptr || !g->out_ptr)) return fail(GNN_ERR_BADARG, "gnn_fx_forward: X, in_ptr or out_ptr is null");
    if (E > 0 && (!g->src || !g->dst || !e_raw || !e_float))
        return fail(GNN_ERR_BADARG, "gnn_fx_forward: src, dst, e_raw or e_float is null");
    if (E > 0 && N > 0 && (!g->in_eid || !g->in_nbr || !g->out_eid || !g->out_nbr))
        return fail(GNN_ERR_BADARG, "gnn_fx_forward: a segment list is null");
    if (int rc = check_workspace(workspace, workspace_bytes, carve_fx(nullptr, N, E, p->F, p->D).bytes)) return rc;
    const Fx f = fx_of(*fmt);
    return ModelShapes::find<int>(p->F, p->D, GNN_ERR_UNSUPPORTED, [&](auto sh) {      // (gnn_fx_supported: the shape is listed)
        return fx_forward_impl<sh.F, sh.D>(g, p, f, tables, n_iters, e_raw, e_float, counts, e_trace, H_trace,
                                           align_ws(workspace), static_cast<hipStream_t>(stream));
    });
}

}  // extern "C"
