// gnn_kernels.hip - SegmentClassifier message-passing forward for gfx950 (MI355X, CDNA4).
//
// What the reference does with dense one-hot incidence matrices and bmm
// (gnn/model.py:69-81,113-125,140-156) is done here in index form, one lane per
// segment (edge pass) or per hit (node pass), wave64, fp32 throughout:
//
//   k_input  H0[n] = [tanh(Win X[n] + bin) | X[n]]                       model.py:144-146
//   k_edge   e[j]  = sigmoid(W2 tanh(P[src j] + Q[dst j]) + b2)          model.py:71-73,45-49
//   k_node   mi/mo = CSR pull segment sums of e[j] * H[nbr]; H' = tanh(W4 tanh(W3 M + b3) + b4)
//                                                                        model.py:114-125,154
//
// The first edge-MLP layer is linear in the concatenated pair [H_src | H_dst], so it is
// split per hit:  W1 [H_s | H_d] + b1 = (W1[:, :C] H_s + b1) + W1[:, C:] H_d = P[s] + Q[d].
// P and Q (D floats each) are produced by the kernel that produces H (k_input / k_node), which
// turns the per-segment 2C x D contraction into a per-hit one (E/N ~ 10x fewer FMAs) and
// shrinks the per-segment gather from 2 x C to 2 x D floats.
//
// Weights are tiny (569 floats at F=3, D=8): every weight address is wave-uniform, so the
// compiler keeps them on the scalar path (s_load / SGPR operands) - no LDS, no VGPR copies.
// No MFMA here by design: at D <= 16 the work is HBM/gather-bound integer-indexed traffic.
//
// Host side (below the kernels): choose_fwd_route fixes the route of a call before its first launch, FwdRun has the
// one launch site of every kernel, forward_impl is the loop over it.  The route, with `wide` open to D >= 32 while
// GNN_NODE_ONE_LANE is unset (read_fwd_switches, once per call):
//   input pass  k_input (H0 and P | Q);  wide at >= 2048 hits when P | Q is wanted: k_input (H0), k_pq_mlpW (P | Q)
//   edge pass   k_edge
//   node pass   k_node;  wide at >= 2048 hits, and with a NodeClassifier's head at every size: k_node_walkW, k_node_mlpW
//   gnn_input_fwd / gnn_edge_fwd (k_pq, k_edge) / gnn_node_fwd: one lane per item at every size
// k_event / run_events: the same forward for batches of small graphs, one launch, one workgroup per graph.
// The C ABI at the end of the file is that of these kernels only: gnn_input_fwd, gnn_edge_fwd, gnn_node_fwd,
// gnn_forward_workspace_bytes, gnn_segclf_forward(_train), gnn_nodeclf_forward(_train), gnn_events_supported,
// gnn_segclf_forward_events, gnn_segclf_forward_train_events.  (The library's core - last error, profiler, ABI version,
// shape queries - is core.hip; the fused pipeline, the backward and the dense-to-index adapter own their entry points.)
#include "common.h"
#include "lane_ops.h"
#include "event_passes.h"

#include <type_traits>

namespace {
using namespace gnn;

// P = W1[:, :C] h + b1, Q = W1[:, C:] h  -> PQ row [P(D) | Q(D)], stored as float4s.
template <int F, int D>
__device__ __forceinline__ void store_pq(const float *h, const float *__restrict__ W1,
                                         const float *__restrict__ b1, float *__restrict__ pq_row)
{
    constexpr int C = F + D;
    float pq[2 * D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        float p = b1[d], q = 0.0f;
#pragma unroll
        for (int k = 0; k < C; ++k) {
            p = fmaf(W1[d * 2 * C + k], h[k], p);
            q = fmaf(W1[d * 2 * C + C + k], h[k], q);
        }
        pq[d] = p;
        pq[D + d] = q;
    }
    float4 *o = reinterpret_cast<float4 *>(pq_row);
#pragma unroll
    for (int v = 0; v < 2 * D / 4; ++v)
        o[v] = make_float4(pq[4 * v], pq[4 * v + 1], pq[4 * v + 2], pq[4 * v + 3]);
}

// NodeClassifier's output network on a finished hit row h = [H'_T | X]: sigmoid(Wo h + bo), Wo [1, C]
// (gnn/MPNN_HitClassifier.ipynb cell 21), k ascending from the bias in every kernel that runs it
template <int C>
__device__ __forceinline__ float head_score(const float *h, const float *__restrict__ Wo, const float *__restrict__ bo)
{
    float acc = bo[0];
#pragma unroll
    for (int k = 0; k < C; ++k) acc = fmaf(Wo[k], h[k], acc);
    return sigmoid_f(acc);
}

// ---------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------
// input network + skip concat (+ P/Q of the first edge pass).  One hit per lane.
template <int F, int D>
__global__ __launch_bounds__(kBlock) void k_input(const float *__restrict__ X,
                                                  const float *__restrict__ Win,
                                                  const float *__restrict__ bin,
                                                  const float *__restrict__ W1,
                                                  const float *__restrict__ b1,
                                                  float *__restrict__ H, int ldh,
                                                  float *__restrict__ PQ, int64_t n_hits,
                                                  const float *__restrict__ Wo = nullptr,
                                                  const float *__restrict__ bo = nullptr,
                                                  float *__restrict__ y = nullptr)
{
    constexpr int LDH = Shape<F, D>::LDH;
    const int64_t n = xcd_block() * kBlock + threadIdx.x;
    if (n >= n_hits) return;
    float h[LDH];
#pragma unroll
    for (int k = 0; k < F; ++k) h[D + k] = X[n * F + k];
#pragma unroll
    for (int k = D + F; k < LDH; ++k) h[k] = 0.0f;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        float acc = bin[d];
#pragma unroll
        for (int k = 0; k < F; ++k) acc = fmaf(Win[d * F + k], h[D + k], acc);
        h[d] = tanh_f(acc);
    }
    store_vec<LDH>(H + n * ldh, h);
    if (PQ) store_pq<F, D>(h, W1, b1, PQ + n * 2 * D);
    if (y) y[n] = head_score<F + D>(h, Wo, bo);           // n_iters = 0: the output network reads H0
}

// P/Q from an existing H (stand-alone EdgeNetwork entry point).
template <int F, int D>
__global__ __launch_bounds__(kBlock) void k_pq(const float *__restrict__ H, int ldh,
                                               const float *__restrict__ W1,
                                               const float *__restrict__ b1,
                                               float *__restrict__ PQ, int64_t n_hits)
{
    constexpr int C = F + D;
    const int64_t n = xcd_block() * kBlock + threadIdx.x;
    if (n >= n_hits) return;
    float h[C];
#pragma unroll
    for (int k = 0; k < C; ++k) h[k] = H[n * ldh + k];
    store_pq<F, D>(h, W1, b1, PQ + n * 2 * D);
}

// edge pass: one segment per lane; coalesced src/dst reads and e writes, two D-float gathers.
template <int D>
__global__ __launch_bounds__(kBlock) void k_edge(const int32_t *__restrict__ src,
                                                 const int32_t *__restrict__ dst,
                                                 const float *__restrict__ PQ,
                                                 const float *__restrict__ b1,
                                                 const float *__restrict__ W2,
                                                 const float *__restrict__ b2,
                                                 float *__restrict__ e, int64_t n_segments)
{
    const int64_t j = xcd_block() * kBlock + threadIdx.x;
    if (j >= n_segments) return;
    const int s = src[j], d = dst[j];
    float z[D];
    if (s >= 0) {
        const float4 *p = reinterpret_cast<const float4 *>(PQ + (int64_t)s * 2 * D);
        const float4 *q = reinterpret_cast<const float4 *>(PQ + (int64_t)d * 2 * D + D);
#pragma unroll
        for (int v = 0; v < D / 4; ++v) {
            const float4 a = p[v], b = q[v];
            z[4 * v] = a.x + b.x;
            z[4 * v + 1] = a.y + b.y;
            z[4 * v + 2] = a.z + b.z;
            z[4 * v + 3] = a.w + b.w;
        }
    } else {  // padded column: gathered rows are zero -> first layer output is b1
#pragma unroll
        for (int k = 0; k < D; ++k) z[k] = b1[k];
    }
    float acc = b2[0];
#pragma unroll
    for (int k = 0; k < D; ++k) acc = fmaf(W2[k], tanh_f(z[k]), acc);
    e[j] = sigmoid_f(acc);
}

// node pass: one hit per lane; pull-mode segment sums over the two CSRs in ascending segment
// id, fused 3C -> D -> D tanh MLP, skip concat, and P/Q for the next edge pass.
template <int F, int D>
__global__ __launch_bounds__(kBlock) void k_node(
    const float *__restrict__ H, int ldh, const float *__restrict__ e,
    const int32_t *__restrict__ in_ptr, const int32_t *__restrict__ in_eid,
    const int32_t *__restrict__ in_nbr, const int32_t *__restrict__ out_ptr,
    const int32_t *__restrict__ out_eid, const int32_t *__restrict__ out_nbr,
    const float *__restrict__ W3, const float *__restrict__ b3, const float *__restrict__ W4,
    const float *__restrict__ b4, const float *__restrict__ W1, const float *__restrict__ b1,
    float *__restrict__ Hn, int ldhn, float *__restrict__ PQ, float *__restrict__ Qkeep, int64_t n_hits,
    const float *__restrict__ Wo, const float *__restrict__ bo, float *__restrict__ y)
{
    constexpr int C = Shape<F, D>::C;
    constexpr int LDH = Shape<F, D>::LDH;
    const int64_t n = xcd_block() * kBlock + threadIdx.x;
    if (n >= n_hits) return;

    float M[3 * LDH];   // [mi | mo | h], each padded to LDH
#pragma unroll
    for (int k = 0; k < 2 * LDH; ++k) M[k] = 0.0f;
    {
        const float4 *hp = reinterpret_cast<const float4 *>(H + n * ldh);
#pragma unroll
        for (int v = 0; v < LDH / 4; ++v) {
            const float4 a = hp[v];
            M[2 * LDH + 4 * v] = a.x;
            M[2 * LDH + 4 * v + 1] = a.y;
            M[2 * LDH + 4 * v + 2] = a.z;
            M[2 * LDH + 4 * v + 3] = a.w;
        }
    }
    // segments ending here: weight e[j], features of the start hit      (model.py:117-118)
    constexpr int U = D <= 16 ? 4 : 1;
    csr_walk<LDH / 4, U>(in_ptr[n], in_ptr[n + 1],
                         [&](int k) { return H + (int64_t)in_nbr[k] * ldh; },
                         [&](int k) { return e[in_eid[k]]; },
                         [&](float w, const float *a) {
#pragma unroll
                             for (int c = 0; c < LDH; ++c) M[c] = fmaf(w, a[c], M[c]);
                         });
    // segments starting here: weight e[j], features of the end hit      (model.py:116,119)
    csr_walk<LDH / 4, U>(out_ptr[n], out_ptr[n + 1],
                         [&](int k) { return H + (int64_t)out_nbr[k] * ldh; },
                         [&](int k) { return e[out_eid[k]]; },
                         [&](float w, const float *a) {
#pragma unroll
                             for (int c = 0; c < LDH; ++c) M[LDH + c] = fmaf(w, a[c], M[LDH + c]);
                         });
    // MLP on M = [mi | mo | h]                                          (model.py:120,94-98)
    float q[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        float acc = b3[d];
#pragma unroll
        for (int k = 0; k < C; ++k) acc = fmaf(W3[d * 3 * C + k], M[k], acc);
#pragma unroll
        for (int k = 0; k < C; ++k) acc = fmaf(W3[d * 3 * C + C + k], M[LDH + k], acc);
#pragma unroll
        for (int k = 0; k < C; ++k) acc = fmaf(W3[d * 3 * C + 2 * C + k], M[2 * LDH + k], acc);
        q[d] = tanh_f(acc);
    }
    if (Qkeep) store_vec<D>(Qkeep + n * D, q);         // training: the backward needs no second list walk
    float hn[LDH];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        float acc = b4[d];
#pragma unroll
        for (int k = 0; k < D; ++k) acc = fmaf(W4[d * D + k], q[k], acc);
        hn[d] = tanh_f(acc);
    }
#pragma unroll
    for (int k = D; k < LDH; ++k) hn[k] = M[2 * LDH + k];   // skip concat of X (model.py:154)
    store_vec<LDH>(Hn + n * ldhn, hn);
    if (PQ) store_pq<F, D>(hn, W1, b1, PQ + n * 2 * D);
    if (y) y[n] = head_score<C>(hn, Wo, bo);             // last node pass of a NodeClassifier: its output network
}

// ---------------------------------------------------------------------------------------------
// node pass for WIDE hidden layers (hidden_dim 32 / 64) at detector size, in two kernels
// ---------------------------------------------------------------------------------------------
// k_node keeps M = [mi | mo | h] (3C = 201 floats at D = 64) in one lane's registers and feeds the MLP
// scalar weight operands: 100 KB of weights per wave through the scalar cache, 0.42 ms per pass at
// 50 k hits.  Here (1) k_node_walkW: 16 lanes per hit walk the two lists (lane p gathers 16-byte
// chunk p of a neighbour's row; list entries and scores one per lane, broadcast in the quad) and
// store mi | mo; (2) k_node_mlpW: the MLP of 256 hits as exact fp32 matrix-core products
// (v_mfma_f32_16x16x4_f32 accumulates in k order from the bias: the same fma chain as k_node's loops)
// from transposed LDS stagings of mi, mo, h, then q, then [H' | x].
template <int LDH>
__device__ __forceinline__ void row16_walk(int beg, int end, int n, int p, const int32_t *__restrict__ nbr,
                                           const int32_t *__restrict__ eid, const float *__restrict__ e,
                                           const float *__restrict__ H, int ldh, float (*acc)[4])
{
    constexpr int NCH = LDH / 4, CPL = (NCH + 15) / 16;
    const int q = p & 3;
    for (int k = beg; k < end; k += 4) {
        const int kk = k + q;
        const bool ok = kk < end;
        const int nb = ok ? nbr[kk] : n;
        const float ev = ok ? e[eid[kk]] : 0.0f;
        float4 r[4][CPL];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int nbj = j == 0   ? quad_bcast<0>(nb)
                            : j == 1 ? quad_bcast<1>(nb)
                            : j == 2 ? quad_bcast<2>(nb)
                                     : quad_bcast<3>(nb);
            const float4 *row = reinterpret_cast<const float4 *>(H + (int64_t)nbj * ldh);
#pragma unroll
            for (int c = 0; c < CPL; ++c)
                r[j][c] = (p + 16 * c < NCH) ? row[p + 16 * c] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float w = j == 0   ? quad_bcast<0>(ev)
                            : j == 1 ? quad_bcast<1>(ev)
                            : j == 2 ? quad_bcast<2>(ev)
                                     : quad_bcast<3>(ev);
            if (k + j < end) {                              // (row-uniform; the sums are those of k_node)
#pragma unroll
                for (int c = 0; c < CPL; ++c) {
                    acc[c][0] = fmaf(w, r[j][c].x, acc[c][0]);
                    acc[c][1] = fmaf(w, r[j][c].y, acc[c][1]);
                    acc[c][2] = fmaf(w, r[j][c].z, acc[c][2]);
                    acc[c][3] = fmaf(w, r[j][c].w, acc[c][3]);
                }
            }
        }
    }
}

constexpr int kWalkBlock = 1024, kWalkHits = kWalkBlock / 16;
constexpr int64_t kNodeWideMinHits = 2048;
inline unsigned grid_walk(int64_t n)
{
    const unsigned g = (unsigned)((n + kWalkHits - 1) / kWalkHits);
    return g > 8 ? (g + 7) & ~7u : g;
}

template <int F, int D>
__global__ __launch_bounds__(kWalkBlock) void k_node_walkW(
    const float *__restrict__ H, int ldh, const float *__restrict__ e,
    const int32_t *__restrict__ in_ptr, const int32_t *__restrict__ in_eid, const int32_t *__restrict__ in_nbr,
    const int32_t *__restrict__ out_ptr, const int32_t *__restrict__ out_eid, const int32_t *__restrict__ out_nbr,
    float *__restrict__ M, int64_t n_hits)
{
    constexpr int LDH = Shape<F, D>::LDH, NCH = LDH / 4, CPL = (NCH + 15) / 16;
    const int p = threadIdx.x & 15;
    const int64_t n = xcd_block() * kWalkHits + (threadIdx.x >> 4);
    if (n >= n_hits) return;                            // (whole 16-lane rows leave together)
    float mi[CPL][4], mo[CPL][4];
#pragma unroll
    for (int c = 0; c < CPL; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) mi[c][i] = mo[c][i] = 0.0f;
    row16_walk<LDH>(in_ptr[n], in_ptr[n + 1], (int)n, p, in_nbr, in_eid, e, H, ldh, mi);       // model.py:117-118
    row16_walk<LDH>(out_ptr[n], out_ptr[n + 1], (int)n, p, out_nbr, out_eid, e, H, ldh, mo);   // model.py:116,119
    float4 *row = reinterpret_cast<float4 *>(M + n * 2 * LDH);
#pragma unroll
    for (int c = 0; c < CPL; ++c)
        if (p + 16 * c < NCH) {
            row[p + 16 * c] = make_float4(mi[c][0], mi[c][1], mi[c][2], mi[c][3]);
            row[NCH + p + 16 * c] = make_float4(mo[c][0], mo[c][1], mo[c][2], mo[c][3]);
        }
}

template <int F, int D>
__global__ __launch_bounds__(kBlock) void k_node_mlpW(
    const float *__restrict__ H, int ldh, const float *__restrict__ M, const float *__restrict__ W3,
    const float *__restrict__ b3, const float *__restrict__ W4, const float *__restrict__ b4,
    const float *__restrict__ W1, const float *__restrict__ b1, float *__restrict__ Hn, int ldhn,
    float *__restrict__ PQ, float *__restrict__ Qkeep, int64_t n_hits, const float *__restrict__ Wo,
    const float *__restrict__ bo, float *__restrict__ y)
{
    constexpr int C = Shape<F, D>::C, LDH = Shape<F, D>::LDH, RS = kBlock + 4;
    constexpr int RT = D / 16, KS = (C + 3) / 4, ROWS = 4 * KS > D ? 4 * KS : D;
    __shared__ __attribute__((aligned(16))) float lds[ROWS * RS];   // [k][hit]: one operand block at a time
    const int64_t n0 = xcd_block() * kBlock, n = n0 + threadIdx.x;
    const bool active = n < n_hits;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r16 = lane & 15, g4 = lane >> 4;
    const int hcol = 64 * wv + r16;
    float hp[LDH];
#pragma unroll
    for (int k = 0; k < LDH; ++k) hp[k] = 0.0f;
    if (active) {
        const float4 *row = reinterpret_cast<const float4 *>(H + n * ldh);
#pragma unroll
        for (int v = 0; v < LDH / 4; ++v) {
            const float4 a = row[v];
            hp[4 * v] = a.x; hp[4 * v + 1] = a.y; hp[4 * v + 2] = a.z; hp[4 * v + 3] = a.w;
        }
    }
    // ---- q = tanh(W3 [mi | mo | h] + b3): three k-chunks of C rows            (model.py:120)
    f4_t cq[RT][4];
#pragma unroll
    for (int it = 0; it < RT; ++it) {
        const f4_t bias = *reinterpret_cast<const f4_t *>(b3 + 16 * it + 4 * g4);
#pragma unroll
        for (int ht = 0; ht < 4; ++ht) cq[it][ht] = bias;
    }
#pragma unroll 1
    for (int chunk = 0; chunk < 3; ++chunk) {
        if (chunk) __syncthreads();
        {
            float v[LDH];
            if (chunk < 2) {
#pragma unroll
                for (int k = 0; k < LDH; ++k) v[k] = 0.0f;
                if (active) {
                    const float4 *row = reinterpret_cast<const float4 *>(M + n * 2 * LDH + chunk * LDH);
#pragma unroll
                    for (int u = 0; u < LDH / 4; ++u) {
                        const float4 a = row[u];
                        v[4 * u] = a.x; v[4 * u + 1] = a.y; v[4 * u + 2] = a.z; v[4 * u + 3] = a.w;
                    }
                }
            } else {
#pragma unroll
                for (int k = 0; k < LDH; ++k) v[k] = hp[k];
            }
#pragma unroll
            for (int k = 0; k < 4 * KS; ++k) lds[k * RS + threadIdx.x] = k < C ? v[k < LDH ? k : 0] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < RT; ++it) {
            const int i = 16 * it + r16;
#pragma unroll 4
            for (int st = 0; st < KS; ++st) {
                const int kk = 4 * st + g4;
                const float aw = kk < C ? W3[i * 3 * C + chunk * C + kk] : 0.0f;
                const float *bv = lds + kk * RS + hcol;
#pragma unroll
                for (int ht = 0; ht < 4; ++ht) cq[it][ht] = __builtin_amdgcn_mfma_f32_16x16x4f32(aw, bv[16 * ht], cq[it][ht], 0, 0, 0);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < RT; ++it)
#pragma unroll
        for (int ht = 0; ht < 4; ++ht) {
            const f4_t q = {tanh_f(cq[it][ht].x), tanh_f(cq[it][ht].y), tanh_f(cq[it][ht].z), tanh_f(cq[it][ht].w)};
            float *x = lds + (16 * it + 4 * g4) * RS + hcol + 16 * ht;
            x[0] = q.x; x[RS] = q.y; x[2 * RS] = q.z; x[3 * RS] = q.w;
            const int64_t nn = n0 + hcol + 16 * ht;
            if (Qkeep && nn < n_hits) *reinterpret_cast<f4_t *>(Qkeep + nn * D + 16 * it + 4 * g4) = q;
        }
    __syncthreads();
    // ---- H' = tanh(W4 q + b4)                                                   (model.py:94-98)
    f4_t hn[RT][4];
#pragma unroll
    for (int it = 0; it < RT; ++it) {
        const f4_t bias = *reinterpret_cast<const f4_t *>(b4 + 16 * it + 4 * g4);
#pragma unroll
        for (int ht = 0; ht < 4; ++ht) hn[it][ht] = bias;
        const int i = 16 * it + r16;
#pragma unroll 4
        for (int st = 0; st < D / 4; ++st) {
            const float aw = W4[i * D + 4 * st + g4];
            const float *bv = lds + (4 * st + g4) * RS + hcol;
#pragma unroll
            for (int ht = 0; ht < 4; ++ht) hn[it][ht] = __builtin_amdgcn_mfma_f32_16x16x4f32(aw, bv[16 * ht], hn[it][ht], 0, 0, 0);
        }
#pragma unroll
        for (int ht = 0; ht < 4; ++ht) {
            hn[it][ht] = f4_t{tanh_f(hn[it][ht].x), tanh_f(hn[it][ht].y), tanh_f(hn[it][ht].z), tanh_f(hn[it][ht].w)};
            const int64_t nn = n0 + hcol + 16 * ht;
            if (nn < n_hits) *reinterpret_cast<f4_t *>(Hn + nn * ldhn + 16 * it + 4 * g4) = hn[it][ht];
        }
    }
    if (active) {                                        // skip concat of X (and the row's padding), model.py:154
#pragma unroll
        for (int v = D / 4; v < LDH / 4; ++v)
            reinterpret_cast<float4 *>(Hn + n * ldhn)[v] = make_float4(hp[4 * v], hp[4 * v + 1], hp[4 * v + 2], hp[4 * v + 3]);
    }
    if (y) {                                             // (kernel-uniform) last node pass of a NodeClassifier:
        // y = sigmoid(Wo [H' | x] + bo) - H' goes through LDS back to the thread that owns the hit
        __syncthreads();
#pragma unroll
        for (int it = 0; it < RT; ++it)
#pragma unroll
            for (int ht = 0; ht < 4; ++ht) {
                float *x = lds + (16 * it + 4 * g4) * RS + hcol + 16 * ht;
                x[0] = hn[it][ht].x; x[RS] = hn[it][ht].y; x[2 * RS] = hn[it][ht].z; x[3 * RS] = hn[it][ht].w;
            }
        __syncthreads();
        if (active) {
            float h[C];
#pragma unroll
            for (int k = 0; k < C; ++k) h[k] = k < D ? lds[k * RS + threadIdx.x] : hp[k];
            y[n] = head_score<C>(h, Wo, bo);
        }
    }
    if (!PQ) return;                                     // (kernel-uniform)
    // ---- P = W1a [H' | x] + b1, Q = W1b [H' | x] for the next edge pass
    __syncthreads();
#pragma unroll
    for (int it = 0; it < RT; ++it)
#pragma unroll
        for (int ht = 0; ht < 4; ++ht) {
            float *x = lds + (16 * it + 4 * g4) * RS + hcol + 16 * ht;
            x[0] = hn[it][ht].x; x[RS] = hn[it][ht].y; x[2 * RS] = hn[it][ht].z; x[3 * RS] = hn[it][ht].w;
        }
#pragma unroll
    for (int k = D; k < 4 * KS; ++k) lds[k * RS + threadIdx.x] = k < C ? hp[k < LDH ? k : 0] : 0.0f;
    __syncthreads();
#pragma unroll 1
    for (int it = 0; it < RT; ++it) {
        const int i = 16 * it + r16;
        f4_t cp[4], cqq[4];
        const f4_t bias = *reinterpret_cast<const f4_t *>(b1 + 16 * it + 4 * g4);
#pragma unroll
        for (int ht = 0; ht < 4; ++ht) { cp[ht] = bias; cqq[ht] = f4_t{0.0f, 0.0f, 0.0f, 0.0f}; }
#pragma unroll 4
        for (int st = 0; st < KS; ++st) {
            const int kk = 4 * st + g4;
            const float ap = kk < C ? W1[i * 2 * C + kk] : 0.0f, aq = kk < C ? W1[i * 2 * C + C + kk] : 0.0f;
            const float *bv = lds + kk * RS + hcol;
#pragma unroll
            for (int ht = 0; ht < 4; ++ht) {
                const float bb = bv[16 * ht];
                cp[ht] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap, bb, cp[ht], 0, 0, 0);
                cqq[ht] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq, bb, cqq[ht], 0, 0, 0);
            }
        }
#pragma unroll
        for (int ht = 0; ht < 4; ++ht) {
            const int64_t nn = n0 + hcol + 16 * ht;
            if (nn < n_hits) {
                *reinterpret_cast<f4_t *>(PQ + nn * 2 * D + 16 * it + 4 * g4) = cp[ht];
                *reinterpret_cast<f4_t *>(PQ + nn * 2 * D + D + 16 * it + 4 * g4) = cqq[ht];
            }
        }
    }
}

// P / Q rows of 256 hits from their H rows, wide hidden layers: the same products as k_node_mlpW's last
// stage (exact fp32, k ascending from the bias), H staged transposed with coalesced loads.  k_input /
// k_pq feed these products scalar weight operands: 0.13 ms for 50 k hits at D = 64.
template <int F, int D>
__global__ __launch_bounds__(kBlock) void k_pq_mlpW(const float *__restrict__ H, int ldh, const float *__restrict__ W1,
                                                    const float *__restrict__ b1, float *__restrict__ PQ, int64_t n_hits)
{
    constexpr int C = Shape<F, D>::C, LDH = Shape<F, D>::LDH, RS = kBlock + 4;
    constexpr int RT = D / 16, KS = (C + 3) / 4;
    static_assert(LDH == 4 * KS, "a padded H row is the k-steps of the products");
    __shared__ __attribute__((aligned(16))) float lds[LDH * RS];
    const int64_t n0 = xcd_block() * kBlock;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r16 = lane & 15, g4 = lane >> 4;
    const int hcol = 64 * wv + r16;
#pragma unroll 4
    for (int j = threadIdx.x; j < kBlock * (LDH / 4); j += kBlock) {      // consecutive threads, consecutive 16-byte pieces
        const int hit = j / (LDH / 4), c = j % (LDH / 4);
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (n0 + hit < n_hits) v = *reinterpret_cast<const float4 *>(H + (n0 + hit) * ldh + 4 * c);
        float *d = lds + (4 * c) * RS + hit;
        d[0] = v.x; d[RS] = v.y; d[2 * RS] = v.z; d[3 * RS] = v.w;
    }
    __syncthreads();
#pragma unroll 1
    for (int it = 0; it < RT; ++it) {
        const int i = 16 * it + r16;
        f4_t cp[4], cq[4];
        const f4_t bias = *reinterpret_cast<const f4_t *>(b1 + 16 * it + 4 * g4);
#pragma unroll
        for (int ht = 0; ht < 4; ++ht) { cp[ht] = bias; cq[ht] = f4_t{0.0f, 0.0f, 0.0f, 0.0f}; }
#pragma unroll 4
        for (int st = 0; st < KS; ++st) {
            const int kk = 4 * st + g4;
            const float ap = kk < C ? W1[i * 2 * C + kk] : 0.0f, aq = kk < C ? W1[i * 2 * C + C + kk] : 0.0f;
            const float *bv = lds + kk * RS + hcol;
#pragma unroll
            for (int ht = 0; ht < 4; ++ht) {
                const float bb = bv[16 * ht];
                cp[ht] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap, bb, cp[ht], 0, 0, 0);
                cq[ht] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq, bb, cq[ht], 0, 0, 0);
            }
        }
#pragma unroll
        for (int ht = 0; ht < 4; ++ht) {
            const int64_t nn = n0 + hcol + 16 * ht;
            if (nn < n_hits) {
                *reinterpret_cast<f4_t *>(PQ + nn * 2 * D + 16 * it + 4 * g4) = cp[ht];
                *reinterpret_cast<f4_t *>(PQ + nn * 2 * D + D + 16 * it + 4 * g4) = cq[ht];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// small events: the WHOLE forward of one graph in one workgroup, one launch for the batch
// ---------------------------------------------------------------------------------------------
// The per-module kernels above cost one launch per pass (2T + 2 launches, ~5 us each on the
// stream): for the reference's muon graphs (tens of hits, gnn/prepareMuonGraphs.py) that is all
// of the time.  Here a workgroup owns one graph of the block-diagonal batch: H (two buffers),
// the P/Q rows and the edge scores live in LDS for all T iterations, hits and segments are dealt
// to the lanes, a barrier separates the passes.  Same arithmetic, in the same order, as
// k_input / k_edge / k_node (the parity tests compare them bit for bit).
// Requires every segment of graph i to join hits of graph i and to lie in
// [seg_ptr[i], seg_ptr[i+1]) (HitGraphBatch.event_layout checks this on the host).
// sizes / LDS offsets (floats, 16-byte aligned) of the ten weight tensors in state_dict order
template <int F, int D>
struct EvWeights {
    static constexpr int C = F + D;
    static constexpr int size(int a)
    {
        return a == 0 ? D * F : a == 2 ? D * 2 * C : a == 5 ? 1 : a == 6 ? D * 3 * C : a == 8 ? D * D : D;
    }
    static constexpr int off(int a)
    {
        int o = 0;
        for (int i = 0; i < a; ++i) o += (size(i) + 3) & ~3;
        return o;
    }
    static constexpr int total = off(10);
};

struct EvW {
    const float *__restrict__ Win, *__restrict__ bin, *__restrict__ W1, *__restrict__ b1,
        *__restrict__ W2, *__restrict__ b2, *__restrict__ W3, *__restrict__ b3, *__restrict__ W4,
        *__restrict__ b4;
};

template <int F, int D>
__global__ __launch_bounds__((EvCfg<D>::NT)) void k_event(
    gnn_graph_t g, const float *__restrict__ Win, const float *__restrict__ bin,
    const float *__restrict__ W1, const float *__restrict__ b1, const float *__restrict__ W2,
    const float *__restrict__ b2, const float *__restrict__ W3, const float *__restrict__ b3,
    const float *__restrict__ W4, const float *__restrict__ b4,
    const int32_t *__restrict__ hit_ptr, const int32_t *__restrict__ seg_ptr, int n_iters,
    float *__restrict__ e_out, int cap_hits, int cap_segments, float *__restrict__ e_all,
    float *__restrict__ H_all)
{   // e_all / H_all (training forward): every pass's scores [T+1, E] and hit rows [T+1, N, LDH]
    constexpr int C = Shape<F, D>::C;
    constexpr int LDH = Shape<F, D>::LDH;
    constexpr int NT = EvCfg<D>::NT, NWV = EvCfg<D>::NWV;
    constexpr int RW = D / NWV;          // output rows of a D-row layer per wavefront
    constexpr int RP = 2 * D / NWV;      // rows of the stacked [P; Q] per wavefront
    static_assert(D % NWV == 0 && RW >= 1, "rows are dealt to the wavefronts");
    extern __shared__ __attribute__((aligned(16))) float ev_lds[];
    float *H = ev_lds, *Hn = H + cap_hits * LDH, *PQ = Hn + cap_hits * LDH,
          *qb = PQ + cap_hits * 2 * D, *Mb = qb + cap_hits * D, *es = Mb + cap_hits * 2 * LDH;
    // (hit_ptr == NULL: the batch is ONE graph - a never-seen single event needs no offset arrays on the device)
    const int h0 = hit_ptr ? hit_ptr[blockIdx.x] : 0, nh = hit_ptr ? hit_ptr[blockIdx.x + 1] - h0 : (int)g.n_hits;
    const int s0 = hit_ptr ? seg_ptr[blockIdx.x] : 0, ns = hit_ptr ? seg_ptr[blockIdx.x + 1] - s0 : (int)g.n_segments;
    const float *__restrict__ X = g.X;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    // The weights (953 floats at F = 11, D = 8) are copied to LDS once and read from there with
    // broadcast ds_reads: a graph is a handful of wavefronts, nothing hides scalar-load latency
    // (measured 38 us per launch on the s_load path).  A hit is a lane; the output rows of every
    // layer are dealt to the wavefronts (each reads its share of the weights and runs its share
    // of the FMAs), layers meet through LDS.  Inputs stream through in 4-float pieces, so the
    // register footprint does not grow with D.  Per row the arithmetic and its order are those of
    // k_input / k_node, so the scores are bit-identical to the per-module kernels.
    using W = EvWeights<F, D>;
    float *wl = es + ((cap_segments + 3) & ~3);
    {
        const float *srcs[10] = {Win, bin, W1, b1, W2, b2, W3, b3, W4, b4};
#pragma unroll
        for (int a = 0; a < 10; ++a)
            for (int i = threadIdx.x; i < W::size(a); i += NT) wl[W::off(a) + i] = srcs[a][i];
    }
    const EvW p = {wl + W::off(0), wl + W::off(1), wl + W::off(2), wl + W::off(3), wl + W::off(4),
                   wl + W::off(5), wl + W::off(6), wl + W::off(7), wl + W::off(8), wl + W::off(9)};
    // The graph's index arrays too, as LOCAL ids: the pull loops below chase eid -> score and
    // nbr -> feature row per list entry, and from global memory every hop is a dependent
    // round trip.  One coalesced pass here instead.
    int32_t *ip = reinterpret_cast<int32_t *>(wl + W::total), *op = ip + cap_hits + 1,
            *ie = op + cap_hits + 1, *inb = ie + cap_segments, *oe = inb + cap_segments,
            *onb = oe + cap_segments, *sl = onb + cap_segments, *dl = sl + cap_segments;
    const bool raw = g.in_ptr == nullptr;            // no segment lists from the caller: built below, in LDS
    const EvIds ids = {ip, op, ie, inb, oe, onb, sl, dl};       // the graph's index arrays as LOCAL ids
    if (nh > 0 && !raw) ev_local_lists<NT>(g, h0, nh, s0, ids);
    ev_local_ends<NT>(g, h0, s0, ns, ids);
    if (raw) {
        // The two lists of a graph nobody has seen before (trigger-style use, gnn/Inference.ipynb cell 3: one event
        // in, scores out), from its (src, dst) alone - what gnn_csr_build does with four launches, here inside the
        // one launch: counts (LDS atomics) -> scan -> slots claimed in arrival order -> every entry's final slot
        // = list base + the number of ids in its list below its own.  Ascending ids whatever the arrival order: the
        // same lists as the caller-built ones, so the scores stay bit-identical to them (and to every other run).
        int *cur_i = reinterpret_cast<int *>(Mb), *cur_o = cur_i + cap_hits, *tmp = reinterpret_cast<int *>(es);
        for (int n = threadIdx.x; n <= nh; n += NT) ip[n] = op[n] = 0;
        __syncthreads();
        for (int j = threadIdx.x; j < ns; j += NT)
            if (sl[j] >= 0) {
                atomicAdd(&ip[dl[j] + 1], 1);
                atomicAdd(&op[sl[j] + 1], 1);
            }
        __syncthreads();
        if (wv < 2) {                                // wavefront 0 scans the in-counts, wavefront 1 the out-counts
            int *ptr = wv ? op : ip;
            const int per = (nh + 64) / 64, b = 1 + lane * per, e = min(b + per, nh + 1);
            int sum = 0;
            for (int n = b; n < e; ++n) sum += ptr[n];
            int incl = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int u = __shfl_up(incl, o, 64);
                if (lane >= o) incl += u;
            }
            int run = incl - sum;
            for (int n = b; n < e; ++n) {
                run += ptr[n];
                ptr[n] = run;
            }
        }
        __syncthreads();
        for (int n = threadIdx.x; n < nh; n += NT) { cur_i[n] = ip[n]; cur_o[n] = op[n]; }
        __syncthreads();
        for (int j = threadIdx.x; j < ns; j += NT)
            if (sl[j] >= 0) tmp[atomicAdd(&cur_i[dl[j]], 1)] = j;
        __syncthreads();
        for (int j = threadIdx.x; j < ns; j += NT)
            if (sl[j] >= 0) {
                const int b = ip[dl[j]], e = ip[dl[j] + 1];
                int r = 0;
                for (int k = b; k < e; ++k) r += tmp[k] < j;
                ie[b + r] = j;
                inb[b + r] = sl[j];
            }
        __syncthreads();
        for (int j = threadIdx.x; j < ns; j += NT)
            if (sl[j] >= 0) tmp[atomicAdd(&cur_o[sl[j]], 1)] = j;
        __syncthreads();
        for (int j = threadIdx.x; j < ns; j += NT)
            if (sl[j] >= 0) {
                const int b = op[sl[j]], e = op[sl[j] + 1];
                int r = 0;
                for (int k = b; k < e; ++k) r += tmp[k] < j;
                oe[b + r] = j;
                onb[b + r] = dl[j];
            }
    }
    // input rows: X into the skip columns of H (k_input), zero padding
    for (int i = threadIdx.x; i < nh * (LDH - D); i += NT) {
        const int n = i / (LDH - D), k = i % (LDH - D);
        H[n * LDH + D + k] = k < F ? X[(int64_t)(h0 + n) * F + k] : 0.0f;
    }
    __syncthreads();

    // acc[r] += sum_j w[r][4c + j] * v[j] over one 4-float piece of the input (k ascending)
    auto fma_piece = [&](float *acc, const float *wrow0, int ldw, int c, const float4 v, auto rows) {
        constexpr int R = decltype(rows)::value;
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * c + j < C)
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = fmaf(wrow0[r * ldw + 4 * c + j], vv[j], acc[r]);
    };

    // rows [wv*RP, (wv+1)*RP) of [P; Q] for every hit, from the full feature rows in `Hsrc`
    auto pq_rows = [&](const float *Hsrc) {
        const int row0 = wv * RP, d0 = row0 % D;
        const bool isq = row0 >= D;                          // wave-uniform (RP divides D)
        for (int n = lane; n < nh; n += 64) {
            float acc[RP];
#pragma unroll
            for (int r = 0; r < RP; ++r) acc[r] = isq ? 0.0f : p.b1[d0 + r];
#pragma unroll
            for (int c = 0; c < LDH / 4; ++c)
                fma_piece(acc, p.W1 + d0 * 2 * C + (isq ? C : 0), 2 * C, c,
                          *reinterpret_cast<const float4 *>(Hsrc + n * LDH + 4 * c),
                          std::integral_constant<int, RP>{});
#pragma unroll
            for (int r = 0; r < RP; ++r) PQ[n * 2 * D + row0 + r] = acc[r];
        }
    };

    // input network (k_input): rows of tanh(Win x + bin) per wavefront
    for (int n = lane; n < nh; n += 64) {
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            const int d = wv * RW + r;
            float acc = p.bin[d];
#pragma unroll
            for (int k = 0; k < F; ++k) acc = fmaf(p.Win[d * F + k], H[n * LDH + D + k], acc);
            H[n * LDH + d] = tanh_f(acc);
        }
    }
    __syncthreads();
    auto keep_rows = [&](const float *Hsrc, int t) {
        if (H_all)
            for (int i = threadIdx.x; i < nh * LDH; i += NT)
                H_all[((int64_t)t * g.n_hits + h0) * LDH + i] = Hsrc[i];
    };
    keep_rows(H, 0);
    pq_rows(H);
    __syncthreads();

    for (int t = 0;; ++t) {
        const bool last = (t == n_iters);
        // edge pass (k_edge): one segment per lane of the workgroup
        for (int j = threadIdx.x; j < ns; j += NT) {
            const int s = sl[j], d = dl[j];
            float acc = p.b2[0];
#pragma unroll
            for (int v = 0; v < D / 4; ++v) {
                float4 z;
                if (s >= 0) {
                    const float4 a = reinterpret_cast<const float4 *>(PQ + s * 2 * D)[v];
                    const float4 b = reinterpret_cast<const float4 *>(PQ + d * 2 * D + D)[v];
                    z = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
                } else {
                    z = make_float4(p.b1[4 * v], p.b1[4 * v + 1], p.b1[4 * v + 2], p.b1[4 * v + 3]);
                }
                acc = fmaf(p.W2[4 * v], tanh_f(z.x), acc);
                acc = fmaf(p.W2[4 * v + 1], tanh_f(z.y), acc);
                acc = fmaf(p.W2[4 * v + 2], tanh_f(z.z), acc);
                acc = fmaf(p.W2[4 * v + 3], tanh_f(z.w), acc);
            }
            const float e = sigmoid_f(acc);
            if (e_all) e_all[(int64_t)t * g.n_segments + s0 + j] = e;
            if (!last)
                es[j] = e;
            else if (e_out)
                e_out[s0 + j] = e;
        }
        if (last) break;
        __syncthreads();
        // node pass (k_node).  Step 1: the segment sums mi, mo of every hit, one (hit, part, 4-float
        // piece) per thread, into LDS (pull over the local CSR, ascending segment id).
        for (int i = threadIdx.x; i < nh * 2 * (LDH / 4); i += NT) {
            const int n = i / (2 * (LDH / 4)), part = (i / (LDH / 4)) & 1, c = i % (LDH / 4);
            const int32_t *el = part ? oe : ie, *nl = part ? onb : inb;
            float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            for (int k = part ? op[n] : ip[n], k1 = part ? op[n + 1] : ip[n + 1]; k < k1; ++k) {
                const float w = es[el[k]];
                const float4 a = *reinterpret_cast<const float4 *>(H + nl[k] * LDH + 4 * c);
                m.x = fmaf(w, a.x, m.x);
                m.y = fmaf(w, a.y, m.y);
                m.z = fmaf(w, a.z, m.z);
                m.w = fmaf(w, a.w, m.w);
            }
            *reinterpret_cast<float4 *>(Mb + n * 2 * LDH + part * LDH + 4 * c) = m;
        }
        __syncthreads();
        // Step 2: first layer, rows per wavefront; M = [mi | mo | h] streams through in pieces
        for (int n = lane; n < nh; n += 64) {
            const int d0 = wv * RW;
            float acc[RW];
#pragma unroll
            for (int r = 0; r < RW; ++r) acc[r] = p.b3[d0 + r];
#pragma unroll 1
            for (int part = 0; part < 3; ++part) {
                const float *mrow = part == 2 ? H + n * LDH : Mb + n * 2 * LDH + part * LDH;
#pragma unroll
                for (int c = 0; c < LDH / 4; ++c)
                    fma_piece(acc, p.W3 + d0 * 3 * C + part * C, 3 * C, c,
                              *reinterpret_cast<const float4 *>(mrow + 4 * c), std::integral_constant<int, RW>{});
            }
#pragma unroll
            for (int r = 0; r < RW; ++r) qb[n * D + d0 + r] = tanh_f(acc[r]);
        }
        for (int i = threadIdx.x; i < nh * (LDH - D); i += NT) {   // skip concat of X (model.py:154)
            const int n = i / (LDH - D), k = D + i % (LDH - D);
            Hn[n * LDH + k] = H[n * LDH + k];
        }
        __syncthreads();
        for (int n = lane; n < nh; n += 64) {                // second layer: rows per wavefront
            const int d0 = wv * RW;
            float acc[RW];
#pragma unroll
            for (int r = 0; r < RW; ++r) acc[r] = p.b4[d0 + r];
#pragma unroll
            for (int c = 0; c < D / 4; ++c) {
                const float4 v = *reinterpret_cast<const float4 *>(qb + n * D + 4 * c);
                const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < RW; ++r) acc[r] = fmaf(p.W4[(d0 + r) * D + 4 * c + j], vv[j], acc[r]);
            }
#pragma unroll
            for (int r = 0; r < RW; ++r) Hn[n * LDH + d0 + r] = tanh_f(acc[r]);
        }
        __syncthreads();
        keep_rows(Hn, t + 1);
        pq_rows(Hn);                                         // nobody reads PQ or H in this step
        __syncthreads();
        float *tmp = H; H = Hn; Hn = tmp;
    }
}

constexpr size_t kEventLdsMax = 128 * 1024;     // of the CU's 160 KB

inline size_t event_lds_bytes(int F, int D, int64_t cap_hits, int64_t cap_segments)
{
    const int C = F + D;
    auto a4 = [](int x) { return (x + 3) & ~3; };
    const int wfl = a4(D * F) + a4(D * 2 * C) + a4(1) + a4(D * 3 * C) + a4(D * D) + 5 * a4(D);   // EvWeights::total
    return ev_fwd_lds_bytes(F, D, cap_hits, cap_segments, wfl);
}

template <int F, int D>
int run_events(const gnn_graph_t *g, const gnn_params_t *p, const int32_t *hit_ptr,
               const int32_t *seg_ptr, int64_t n_graphs, int cap_hits, int cap_segments,
               int n_iters, float *e_out, hipStream_t s, float *e_all = nullptr,
               float *H_all = nullptr)
{
    if (n_graphs <= 0) return 0;
    const size_t lds = event_lds_bytes(F, D, cap_hits, cap_segments);
    static DevOnce attr_done;     // dynamic LDS above 64 KB must be opted into, once per device
    if (attr_done.need())
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_event<F, D>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)kEventLdsMax);
    GNN_LAUNCH_SH("k_event", (k_event<F, D>), (unsigned)n_graphs, EvCfg<D>::NT, lds, s, *g, p->Win, p->bin, p->W1,
                  p->b1, p->W2, p->b2, p->W3, p->b3, p->W4, p->b4, hit_ptr, seg_ptr, n_iters, e_out,
                  cap_hits, cap_segments, e_all, H_all);
    return 0;
}

// H (padded rows) -> unpadded [n_hits, C] trace rows (parity tests only).
__global__ __launch_bounds__(kBlock) void k_unpad(const float *__restrict__ H, int ldh, int C,
                                                  float *__restrict__ out, int64_t total)
{
    const int64_t i = xcd_block() * kBlock + threadIdx.x;
    if (i >= total) return;
    out[i] = H[(i / C) * ldh + (i % C)];
}

// ---------------------------------------------------------------------------------------------
// host side of the per-pass forward
// ---------------------------------------------------------------------------------------------
// the miss of this unit's shape dispatch (ModelShapes, common.h)
int no_kernel(int F, int D) { return fail(GNN_ERR_UNSUPPORTED, "no kernel for input_dim=%d hidden_dim=%d", F, D); }

// The environment switch of the per-pass forward (A / B runs, tests): this is its one reader, called once per library
// call and not cached, like read_bwd_switches - tests flip it inside one process.
struct FwdSwitches { bool node_one_lane; };
FwdSwitches read_fwd_switches() { return {getenv("GNN_NODE_ONE_LANE") != nullptr}; }

// Which kernels a forward takes: fixed by choose_fwd_route before the first launch.  One lane per hit (k_input with
// P / Q, k_node), or wide: the P / Q products on the matrix cores (k_input, k_pq_mlpW) and the 16-lane list walk with
// the matrix-core MLP (k_node_walkW, k_node_mlpW).  The edge pass has one kernel.
struct FwdRoute { bool wide_input, wide_node; };
constexpr FwdRoute kOneLane = {false, false};       // the module entry points: one lane per item at every size

template <int F, int D>
FwdRoute choose_fwd_route(int64_t n_hits, bool have_head, int n_iters, const FwdSwitches &sw)
{
    // wide needs hidden layers of 32 or 64 units, and the switch off
    const bool can_wide = D >= 32 && !sw.node_one_lane;
    const bool detector_size = n_hits >= kNodeWideMinHits;
    // the node pass is wide at detector size; a NodeClassifier's at every size: at the notebook's 32 x 50 hits the one-lane
    // k_node<4, 64> spills (0.21 ms a pass against 0.075 ms for k_node_walkW + k_node_mlpW, profiles/nodeclf_kernel_trace.txt)
    const bool wide_node = can_wide && (detector_size || have_head);
    // the input pass is wide at detector size (a NodeClassifier's too: it keeps the threshold) when P / Q is wanted at
    // all - a head without message passing scores the hits from H0 and has no edge pass
    const bool wide_input = can_wide && detector_size && !(have_head && n_iters == 0);
    return {wide_input, wide_node};
}

struct FwdWs {
    float *Ha, *Hb, *PQ, *e, *M;
    size_t bytes;
};

FwdWs carve_fwd(char *b, int64_t N, int64_t E, int F, int D)
{
    const size_t ldh = (F + D + 3) & ~3;
    Carver c{b};
    FwdWs w;
    w.Ha = c.take<float>((size_t)N * ldh);
    w.Hb = c.take<float>((size_t)N * ldh);
    w.PQ = c.take<float>((size_t)N * 2 * D);
    w.e = c.take<float>((size_t)E);
    w.M = c.take<float>(D >= 32 ? (size_t)N * 2 * ldh : 0);      // wide shapes: [mi | mo] between k_node_walkW and k_node_mlpW
    w.bytes = c.bytes();
    return w;
}

// NodeClassifier's output network in place of the final edge pass: y [n_hits] = sigmoid(Wo [H'_T | X] + bo)
struct Head {
    const float *Wo, *bo;
    float *y;
};

#define FWD_LISTS g->in_ptr, g->in_eid, g->in_nbr, g->out_ptr, g->out_eid, g->out_nbr
// One forward in flight: what its launchers share.  A launcher takes what differs between its calls - the H / e / P|Q /
// Q rows of the pass and the head, if this pass scores the hits - and skips an empty batch.  `ws` null (the module
// entry points, on the one-lane route): nothing is carved, every row is the caller's.
template <int F, int D>
struct FwdRun {
    static constexpr int C = Shape<F, D>::C, LDH = Shape<F, D>::LDH;
    const gnn_graph_t *g;
    const gnn_params_t *p;
    hipStream_t s;
    int64_t N, E;
    FwdWs w;
    FwdRoute route;
    FwdRun(const gnn_graph_t *g_, const gnn_params_t *p_, char *ws, hipStream_t s_, FwdRoute route_)
        : g(g_), p(p_), s(s_), N(g_->n_hits), E(g_->n_segments), w(carve_fwd(ws, N, E, F, D)), route(route_) {}
    // input network: H = [tanh(Win X + bin) | X | 0], P | Q of it into PQ (null: none), the head's scores from H0
    int input(float *H, int ldh, float *PQ, const Head *head) const
    {
        if (N <= 0) return 0;
        GNN_LAUNCH("k_input", (k_input<F, D>), grid_for(N), kBlock, s, g->X, p->Win, p->bin, p->W1, p->b1, H, ldh,
                   route.wide_input ? nullptr : PQ, N, head ? head->Wo : nullptr, head ? head->bo : nullptr,
                   head ? head->y : nullptr);
        if constexpr (D >= 32)
            if (route.wide_input) GNN_LAUNCH("k_pq_mlpW", (k_pq_mlpW<F, D>), grid_for(N), kBlock, s, H, ldh, p->W1, p->b1, PQ, N);
        return 0;
    }
    // P | Q of an H somebody else made (the EdgeNetwork entry point)
    int pq(const float *H, int ldh, float *PQ) const
    {
        if (N > 0) GNN_LAUNCH("k_pq", (k_pq<F, D>), grid_for(N), kBlock, s, H, ldh, p->W1, p->b1, PQ, N);
        return 0;
    }
    int edge(const float *PQ, float *e) const
    {
        if (E > 0) GNN_LAUNCH("k_edge", (k_edge<D>), grid_for(E), kBlock, s, g->src, g->dst, PQ, p->b1, p->W2, p->b2, e, E);
        return 0;
    }
    // node pass (H, e -> Hn), P | Q of Hn into PQ and its hidden layer into Qkeep (null: none), the head's scores from Hn
    int node(const float *H, int ldh, const float *e, float *Hn, float *PQ, float *Qkeep, const Head *head) const
    {
        if (N <= 0) return 0;
        const float *Wo = head ? head->Wo : nullptr, *bo = head ? head->bo : nullptr;
        float *y = head ? head->y : nullptr;
        if constexpr (D >= 32)
            if (route.wide_node) {
                GNN_LAUNCH("k_node_walkW", (k_node_walkW<F, D>), grid_walk(N), kWalkBlock, s, H, ldh, e, FWD_LISTS, w.M, N);
                GNN_LAUNCH("k_node_mlpW", (k_node_mlpW<F, D>), grid_for(N), kBlock, s, H, ldh, w.M, p->W3, p->b3, p->W4,
                           p->b4, p->W1, p->b1, Hn, ldh, PQ, Qkeep, N, Wo, bo, y);
                return 0;
            }
        GNN_LAUNCH("k_node", (k_node<F, D>), grid_for(N), kBlock, s, H, ldh, e, FWD_LISTS, p->W3, p->b3, p->W4, p->b4,
                   p->W1, p->b1, Hn, ldh, PQ, Qkeep, N, Wo, bo, y);
        return 0;
    }
    // H (padded rows) -> one unpadded trace row [N, C]
    int unpad(const float *H, float *out) const
    {
        if (N > 0) GNN_LAUNCH("k_unpad", k_unpad, grid_for(N * C), kBlock, s, H, LDH, C, out, N * C);
        return 0;
    }
};

// where a forward's results go; null: not wanted
struct FwdOut {
    float *e_out;           // the final edge pass [E]
    float *e_trace;         // every edge pass, row t of E floats (row n_iters = e_out's values)
    float *H_trace;         // every H unpadded, row t of [N, C]
    float *H_all;           // training forward: every iteration's H is kept here, no ping-pong
    float *Q_all;           // training forward: the node passes' hidden layers, row t of [N, D]
    const Head *head;       // NodeClassifier
};

// head null: SegmentClassifier (n_iters x (edge pass, node pass), final edge pass -> e_out).  With a head:
// NodeClassifier - the loop ends after the last node pass, whose kernel scores the hits (k_input's for
// n_iters = 0): no final edge pass and no P / Q for it; e_trace then has n_iters rows.
template <int F, int D>
int forward_impl(const gnn_graph_t *g, const gnn_params_t *p, int n_iters, const FwdOut &o, char *ws, hipStream_t s)
{
    const FwdRoute route = choose_fwd_route<F, D>(g->n_hits, o.head, n_iters, read_fwd_switches());
    const FwdRun<F, D> c(g, p, ws, s, route);
    const size_t row = (size_t)c.N * c.LDH;
    float *H = o.H_all ? o.H_all : c.w.Ha, *Hn = o.H_all ? o.H_all + row : c.w.Hb;
    const bool head0 = o.head && n_iters == 0;
    int rc = c.input(H, c.LDH, head0 ? nullptr : c.w.PQ, head0 ? o.head : nullptr);
    for (int t = 0; !rc; ++t) {
        if (o.H_trace && (rc = c.unpad(H, o.H_trace + (size_t)t * c.N * c.C))) break;
        const bool last = t == n_iters;
        if (last && o.head) break;
        float *e_t = o.e_trace ? o.e_trace + (size_t)t * c.E : (last ? o.e_out : c.w.e);
        if ((rc = c.edge(c.w.PQ, e_t))) break;
        if (last) {
            if (o.e_trace && c.E > 0 && o.e_out != e_t) {
                hipError_t err = hipMemcpyAsync(o.e_out, e_t, (size_t)c.E * sizeof(float), hipMemcpyDeviceToDevice, s);
                if (err != hipSuccess) return fail(-(int)err, "copy of final scores failed");
            }
            break;
        }
        const Head *tail = t == n_iters - 1 ? o.head : nullptr;          // the node pass that feeds the head
        rc = c.node(H, c.LDH, e_t, Hn, tail ? nullptr : c.w.PQ, o.Q_all ? o.Q_all + (size_t)t * c.N * D : nullptr, tail);
        if (o.H_all) {
            H = Hn;
            Hn = H + row;
        } else {
            std::swap(H, Hn);
        }
    }
    return rc;
}

// What the whole-model entry points share.  The last of their argument checks: the shape has kernels and the workspace
// holds gnn_forward_workspace_bytes; then the 256-byte alignment and the shape dispatch.
int check_forward(const gnn_graph_t *g, const gnn_params_t *p, const void *ws, size_t ws_bytes)
{
    if (!ModelShapes::has(p->F, p->D)) return no_kernel(p->F, p->D);
    return check_workspace(ws, ws_bytes, carve_fwd(nullptr, g->n_hits, g->n_segments, p->F, p->D).bytes);
}
int forward(const gnn_graph_t *g, const gnn_params_t *p, int n_iters, const FwdOut &o, void *ws, void *stream)
{
    return ModelShapes::find<int>(p->F, p->D, GNN_ERR_UNSUPPORTED, [&](auto sh) {
        return forward_impl<sh.F, sh.D>(g, p, n_iters, o, align_ws(ws), static_cast<hipStream_t>(stream)); });
}

}  // namespace

using namespace gnn;

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" {

int gnn_events_supported(int32_t F, int32_t D, int64_t max_hits, int64_t max_segments)
{
    if (!gnn_shape_supported(F, D) || max_hits < 0 || max_segments < 0) return 0;
    return event_lds_bytes(F, D, max_hits, max_segments) <= kEventLdsMax;
}

// what the two one-launch forwards end with: the last of their checks - the largest graph fits one workgroup's LDS at a
// shape with kernels - and the launch
static int events_forward(const gnn_graph_t *g, const gnn_params_t *p, const int32_t *hit_ptr, const int32_t *seg_ptr,
                          int64_t n_graphs, int32_t max_hits, int32_t max_segments, int32_t n_iters, float *e_out,
                          float *e_all, float *H_all, void *stream)
{
    if (!gnn_events_supported(p->F, p->D, max_hits, max_segments))
        return fail(GNN_ERR_UNSUPPORTED, "events of up to %d hits / %d segments do not fit one workgroup's LDS at input_dim=%d hidden_dim=%d",
                    max_hits, max_segments, p->F, p->D);
    return ModelShapes::find<int>(p->F, p->D, GNN_ERR_UNSUPPORTED, [&](auto sh) {
        return run_events<sh.F, sh.D>(g, p, hit_ptr, seg_ptr, n_graphs, max_hits, max_segments, n_iters, e_out,
                                      static_cast<hipStream_t>(stream), e_all, H_all); });
}

int gnn_segclf_forward_events(const gnn_graph_t *g, const gnn_params_t *p, const int32_t *hit_ptr,
                              const int32_t *seg_ptr, int64_t n_graphs, int32_t max_hits,
                              int32_t max_segments, int32_t n_iters, float *e_out, void *stream)
{
    if (!g || !p || n_iters < 0 || n_graphs < 0 || max_hits < 0 || max_segments < 0)
        return fail(GNN_ERR_BADARG, "gnn_segclf_forward_events: bad argument");
    if (n_graphs > 1 && (!hit_ptr || !seg_ptr)) return fail(GNN_ERR_BADARG, "gnn_segclf_forward_events: graph offsets missing");
    if (n_graphs == 1 && !hit_ptr != !seg_ptr) return fail(GNN_ERR_BADARG, "gnn_segclf_forward_events: one of hit_ptr / seg_ptr missing");
    if (g->n_segments > 0 && (!e_out || !g->src || !g->dst)) return fail(GNN_ERR_BADARG, "gnn_segclf_forward_events: segment arrays missing");
    if (g->n_hits > 0 && !g->X) return fail(GNN_ERR_BADARG, "gnn_segclf_forward_events: hit features missing");
    // the six list arrays come together or not at all (NULL: the kernel builds them in LDS)
    if (g->in_ptr ? (!g->out_ptr || (g->n_segments > 0 && (!g->in_eid || !g->in_nbr || !g->out_eid || !g->out_nbr)))
                  : (g->out_ptr || g->in_eid || g->in_nbr || g->out_eid || g->out_nbr) != 0)
        return fail(GNN_ERR_BADARG, "gnn_segclf_forward_events: segment lists incomplete (all six arrays, or none)");
    return events_forward(g, p, hit_ptr, seg_ptr, n_graphs, max_hits, max_segments, n_iters, e_out, nullptr, nullptr, stream);
}

int gnn_input_fwd(const float *X, const float *Win, const float *bin, float *H, int64_t n_hits,
                  int32_t F, int32_t D, int32_t ldh, void *stream)
{
    if (!X || !Win || !bin || !H || n_hits < 0) return fail(GNN_ERR_BADARG, "gnn_input_fwd: bad argument");
    if (ldh < ((F + D + 3) & ~3) || (ldh & 3)) return fail(GNN_ERR_BADARG, "gnn_input_fwd: ldh must be a multiple of 4 >= C");
    gnn_graph_t g = {};
    gnn_params_t p = {};
    g.X = X, g.n_hits = n_hits;
    p.Win = Win, p.bin = bin;
    if (!ModelShapes::has(F, D)) return no_kernel(F, D);
    return ModelShapes::find<int>(F, D, GNN_ERR_UNSUPPORTED, [&](auto sh) {
        return FwdRun<sh.F, sh.D>(&g, &p, nullptr, static_cast<hipStream_t>(stream), kOneLane).input(H, ldh, nullptr, nullptr); });
}

int gnn_edge_fwd(const float *H, int32_t ldh, const int32_t *src, const int32_t *dst,
                 const float *W1, const float *b1, const float *W2, const float *b2, float *e,
                 float *pq_ws, int64_t n_hits, int64_t n_segments, int32_t F, int32_t D,
                 void *stream)
{
    if (!H || !src || !dst || !W1 || !b1 || !W2 || !b2 || !e || !pq_ws || n_hits < 0 || n_segments < 0)
        return fail(GNN_ERR_BADARG, "gnn_edge_fwd: bad argument");
    if (ldh < F + D) return fail(GNN_ERR_BADARG, "gnn_edge_fwd: ldh < C");
    gnn_graph_t g = {};
    gnn_params_t p = {};
    g.src = src, g.dst = dst, g.n_hits = n_hits, g.n_segments = n_segments;
    p.W1 = W1, p.b1 = b1, p.W2 = W2, p.b2 = b2;
    if (!ModelShapes::has(F, D)) return no_kernel(F, D);
    return ModelShapes::find<int>(F, D, GNN_ERR_UNSUPPORTED, [&](auto sh) {
        const FwdRun<sh.F, sh.D> c(&g, &p, nullptr, static_cast<hipStream_t>(stream), kOneLane);
        if (int rc = c.pq(H, ldh, pq_ws)) return rc;
        return c.edge(pq_ws, e); });
}

int gnn_node_fwd(const float *H, int32_t ldh, const float *e, const gnn_graph_t *g,
                 const float *W3, const float *b3, const float *W4, const float *b4, float *Hnext,
                 int32_t F, int32_t D, void *stream)
{
    if (!H || !e || !g || !W3 || !b3 || !W4 || !b4 || !Hnext || g->n_hits < 0)
        return fail(GNN_ERR_BADARG, "gnn_node_fwd: bad argument");
    if (g->n_hits > 0 && (!g->in_ptr || !g->out_ptr)) return fail(GNN_ERR_BADARG, "gnn_node_fwd: CSR missing");
    if (ldh < ((F + D + 3) & ~3) || (ldh & 3)) return fail(GNN_ERR_BADARG, "gnn_node_fwd: ldh must be a multiple of 4 >= C");
    if (Hnext == H) return fail(GNN_ERR_BADARG, "gnn_node_fwd: Hnext must not alias H");
    gnn_params_t p = {};
    p.W3 = W3, p.b3 = b3, p.W4 = W4, p.b4 = b4;
    if (!ModelShapes::has(F, D)) return no_kernel(F, D);
    return ModelShapes::find<int>(F, D, GNN_ERR_UNSUPPORTED, [&](auto sh) {
        return FwdRun<sh.F, sh.D>(g, &p, nullptr, static_cast<hipStream_t>(stream), kOneLane)
            .node(H, ldh, e, Hnext, nullptr, nullptr, nullptr); });
}

size_t gnn_forward_workspace_bytes(int64_t n_hits, int64_t n_segments, int32_t F, int32_t D)
{
    if (n_hits < 0 || n_segments < 0 || F <= 0 || D <= 0) return 0;
    return carve_fwd(nullptr, n_hits, n_segments, F, D).bytes;
}

int gnn_segclf_forward(const gnn_graph_t *g, const gnn_params_t *p, int32_t n_iters, float *e_out,
                       float *e_trace, float *H_trace, void *workspace, size_t workspace_bytes,
                       void *stream)
{
    gnn::ProfChain chain_;
    if (!g || !p || n_iters < 0 || g->n_hits < 0 || g->n_segments < 0)
        return fail(GNN_ERR_BADARG, "gnn_segclf_forward: bad argument");
    if (g->n_segments > 0 && (!e_out || !g->src || !g->dst))
        return fail(GNN_ERR_BADARG, "gnn_segclf_forward: segment arrays missing");
    if (g->n_hits > 0 && (!g->X || !g->in_ptr || !g->out_ptr))
        return fail(GNN_ERR_BADARG, "gnn_segclf_forward: hit arrays missing");
    if (!params_complete(p)) return fail(GNN_ERR_BADARG, "gnn_segclf_forward: weight pointer missing");
    if (int rc = check_forward(g, p, workspace, workspace_bytes)) return rc;
    return forward(g, p, n_iters, {e_out, e_trace, H_trace, nullptr, nullptr, nullptr}, workspace, stream);
}

int gnn_segclf_forward_train(const gnn_graph_t *g, const gnn_params_t *p, int32_t n_iters,
                             float *e_all, float *H_all, float *Q_all, void *workspace,
                             size_t workspace_bytes, void *stream)
{
    gnn::ProfChain chain_;
    if (!g || !p || n_iters < 0 || g->n_hits < 0 || g->n_segments < 0)
        return fail(GNN_ERR_BADARG, "gnn_segclf_forward_train: bad argument");
    if ((g->n_segments > 0 && (!e_all || !g->src || !g->dst)) || (g->n_hits > 0 && (!H_all || !g->X || !g->in_ptr || !g->out_ptr)))
        return fail(GNN_ERR_BADARG, "gnn_segclf_forward_train: array missing");
    if (int rc = check_forward(g, p, workspace, workspace_bytes)) return rc;
    // e_trace = e_all makes every edge pass land in its row; the "final scores" copy goes to the
    // last row itself (no-op copy avoided by passing that row as e_out)
    float *last = e_all ? e_all + (size_t)n_iters * g->n_segments : nullptr;
    return forward(g, p, n_iters, {last, e_all, nullptr, H_all, Q_all, nullptr}, workspace, stream);
}

// ---- NodeClassifier (gnn/MPNN_HitClassifier.ipynb cells 20-21): the trunk above, the output network in place
// of the final edge pass ------------------------------------------------------------------------------------
static int nodeclf_check(const char *who, const gnn_graph_t *g, const gnn_params_t *p, const float *Wo, const float *bo,
                         int32_t n_iters, const float *y, const void *workspace, size_t workspace_bytes)
{
    if (!g || !p || !Wo || !bo || n_iters < 0 || g->n_hits < 0 || g->n_segments < 0)
        return fail(GNN_ERR_BADARG, "%s: bad argument", who);
    if (g->n_hits > 0 && (!y || !g->X || !g->in_ptr || !g->out_ptr))
        return fail(GNN_ERR_BADARG, "%s: hit arrays missing", who);
    if (n_iters > 0 && g->n_segments > 0 && (!g->src || !g->dst))
        return fail(GNN_ERR_BADARG, "%s: segment arrays missing", who);
    if (!params_complete(p)) return fail(GNN_ERR_BADARG, "%s: weight pointer missing", who);
    return check_forward(g, p, workspace, workspace_bytes);
}

int gnn_nodeclf_forward(const gnn_graph_t *g, const gnn_params_t *p, const float *Wo, const float *bo, int32_t n_iters,
                        float *y_out, float *H_trace, void *workspace, size_t workspace_bytes, void *stream)
{
    gnn::ProfChain chain_;
    if (int rc = nodeclf_check("gnn_nodeclf_forward", g, p, Wo, bo, n_iters, y_out, workspace, workspace_bytes)) return rc;
    const Head head = {Wo, bo, y_out};
    return forward(g, p, n_iters, {nullptr, nullptr, H_trace, nullptr, nullptr, &head}, workspace, stream);
}

int gnn_nodeclf_forward_train(const gnn_graph_t *g, const gnn_params_t *p, const float *Wo, const float *bo,
                              int32_t n_iters, float *e_all, float *H_all, float *Q_all, float *y_out, void *workspace,
                              size_t workspace_bytes, void *stream)
{
    gnn::ProfChain chain_;
    if (int rc = nodeclf_check("gnn_nodeclf_forward_train", g, p, Wo, bo, n_iters, y_out, workspace, workspace_bytes)) return rc;
    if ((n_iters > 0 && g->n_segments > 0 && !e_all) || (g->n_hits > 0 && !H_all))
        return fail(GNN_ERR_BADARG, "gnn_nodeclf_forward_train: array missing");
    const Head head = {Wo, bo, y_out};
    return forward(g, p, n_iters, {nullptr, e_all, nullptr, H_all, Q_all, &head}, workspace, stream);
}

int gnn_segclf_forward_train_events(const gnn_graph_t *g, const gnn_params_t *p, const int32_t *hit_ptr,
                                    const int32_t *seg_ptr, int64_t n_graphs, int32_t max_hits,
                                    int32_t max_segments, int32_t n_iters, float *e_all, float *H_all,
                                    void *stream)
{
    if (!g || !p || n_iters < 0 || n_graphs < 0 || max_hits < 0 || max_segments < 0)
        return fail(GNN_ERR_BADARG, "gnn_segclf_forward_train_events: bad argument");
    if (n_graphs > 0 && (!hit_ptr || !seg_ptr)) return fail(GNN_ERR_BADARG, "gnn_segclf_forward_train_events: graph offsets missing");
    if (g->n_segments > 0 && (!e_all || !g->src || !g->dst)) return fail(GNN_ERR_BADARG, "gnn_segclf_forward_train_events: segment arrays missing");
    if (g->n_hits > 0 && (!H_all || !g->X || !g->in_ptr || !g->out_ptr)) return fail(GNN_ERR_BADARG, "gnn_segclf_forward_train_events: hit arrays missing");
    return events_forward(g, p, hit_ptr, seg_ptr, n_graphs, max_hits, max_segments, n_iters, nullptr, e_all, H_all, stream);
}

}  // extern "C"
