// gcn.hip - the graph-convolution classifiers of gnn/GCN_Seg_Toy2D.ipynb (cells 20-21) and gnn/GCN_Toy2D.ipynb
// (cells 11, 13, 14) for gfx950: GraphConv / GraphConvSelfInt layers inside GCNBinaryClassifier and
// GCRNBinaryClassifier, forward and backward, exact fp32.
//
// The notebooks hand the model a dense [B, N, N] adjacency and call torch.matmul(a, x) once per layer: ~20 small
// launches forward, and a row of the segment adjacency has at most 10 non-zeros out of 225.  Here
//
//   k_gcn_rows / k_gcn_cols   compress A once: per-row and per-column (transposed) lists of (index, value), ascending
//                             index, one uniform width for the whole tensor (a batch slice is a view)
//   k_gcn_fwd                 the whole model in ONE launch, one workgroup per graph: h and x stay in LDS across the
//                             layers, each row pulls its neighbours from the row lists
//   k_gcn_bwd                 the whole backward in ONE launch, one workgroup per graph: A^T gz is a pull over the
//                             column lists (no float atomics), weight gradients are per-graph partial sums
//   k_gcn_reduce              one fixed-order sum of the partial sums over the graphs
//
// Math (ReLU derivative [z > 0], i.e. the mask is h > 0 of the stored post-ReLU h - or h NaN: relu_f, relu_open):
//   h0 = relu(x Wf^T + bf);  per layer hin = h (GCN) or [h | x] (GCRN)
//   GraphConvSelfInt: z = hin Wn^T + bn + (A hin) Wg^T        GraphConv: z = (A hin) Wl^T + bl
//   h' = relu(z);  out = h Wc^T + bc
// Backward per layer, with gz = gh' * [h' > 0] and q = A^T gz:
//   gWn = gz^T hin, gbn = sum_i gz, gWg = (A hin)^T gz = q^T hin, ghin = gz Wn + A^T (gz Wg) = gz Wn + q Wg
// so one pulled matrix q serves both the neighbour weights and the input gradient, and A hin is never rebuilt.
//
// LDS: two [N][ld] row buffers (ld odd: a thread per row walks its row without bank conflicts) + x [N][F]
// (+ the layer's weights, transposed, when they fit).  The forward, whose rows are F wider, reads x from global
// memory instead when the row buffers fit and x beside them does not.  Both in-place row updates (z over h, ghin
// over gz) are row-local, so a pass owns whole rows: compute - barrier - write.
#include "common.h"

namespace gnn {
namespace {

constexpr int kGcnLdsMax = 160 * 1024;       // LDS of one CU; one workgroup may take all of it
constexpr int kGcnMaxWidth = 256;            // an output row of a layer is spread over the 256 threads of a pass
constexpr int kGcnMaxFeatures = 64;
constexpr int kGcnMaxNodes = 4096;

__host__ __device__ inline int gcn_ld(int maxw, int F) { return (maxw + F) | 1; }

// forward: the two row buffers, which it cannot do without, and x, which it stages beside them when it fits
inline size_t gcn_fwd_rows_lds(int N, int F, int maxw) { return (size_t)2 * N * gcn_ld(maxw, F) * 4; }
inline size_t gcn_fwd_lds(int N, int F, int maxw) { return gcn_fwd_rows_lds(N, F, maxw) + (size_t)N * F * 4; }
inline size_t gcn_bwd_lds(int N, int F, int maxw) { return ((size_t)2 * N * gcn_ld(maxw, 0) + (size_t)N * F + N) * 4; }

// Sums over the nodes of a graph (and over the graphs) run in FOUR interleaved chains, i = 0, 1, 2, 3 mod 4, combined as
// (s0 + s1) + (s2 + s3): a fixed order - the same bits in every run - whose rounding error grows with n / 4, and four
// independent FMA chains instead of one.
template <typename Term>
__device__ __forceinline__ float sum4(int n, Term term)
{
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    int i = 0;
    for (; i + 4 <= n; i += 4) {
        s0 += term(i);
        s1 += term(i + 1);
        s2 += term(i + 2);
        s3 += term(i + 3);
    }
    if (i < n) s0 += term(i);
    if (i + 1 < n) s1 += term(i + 1);
    if (i + 2 < n) s2 += term(i + 2);
    return (s0 + s1) + (s2 + s3);
}

// ReLU as torch computes it: relu(NaN) = NaN (fmaxf(NaN, 0) is 0), and its derivative lets the gradient through
// wherever h <= 0 does not hold - at h > 0 and at a NaN h (threshold_backward).  A NaN weight or feature then reaches
// the logits and the gradients instead of turning into a plausible zero.
__device__ __forceinline__ float relu_f(float z) { return z <= 0.0f ? 0.0f : z; }
__device__ __forceinline__ bool relu_open(float h) { return !(h <= 0.0f); }

// ---- compression ---------------------------------------------------------------------------------------------------
// info[0] = widest list (atomicMax), info[1] = status (bit 0: a non-finite entry).  Integer atomics only.
template <bool FILL>
__global__ __launch_bounds__(kBlock) void k_gcn_rows(const float *__restrict__ a, int64_t n_rows, int N, int W,
                                                     int32_t *__restrict__ cnt_out, int32_t *__restrict__ idx,
                                                     float *__restrict__ val, int32_t *__restrict__ info)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (row >= n_rows) return;                                   // (whole waves leave: the ballots below are full)
    const float *ar = a + row * N;
    int cnt = 0, bad = 0;
    for (int j0 = 0; j0 < N; j0 += 64) {
        const int j = j0 + lane;
        const float v = j < N ? ar[j] : 0.0f;
        const bool nz = v != 0.0f;                               // NaN != 0: kept, and flagged
        bad |= !__builtin_isfinite(v);
        const unsigned long long m = __ballot(nz);
        if (FILL && nz) {
            const int pos = cnt + __popcll(m & ((1ull << lane) - 1ull));
            if (pos < W) {
                idx[row * W + pos] = j;
                val[row * W + pos] = v;
            }
        }
        cnt += __popcll(m);
    }
    if (!FILL) {
        const unsigned long long b = __ballot(bad != 0);
        if (lane == 0) {
            cnt_out[row] = cnt;
            atomicMax(info, cnt);
            if (b) atomicOr(info + 1, 1);
        }
    }
}

template <bool FILL>
__global__ __launch_bounds__(kBlock) void k_gcn_cols(const float *__restrict__ a, int64_t n_cols, int N, int W,
                                                     int32_t *__restrict__ cnt_out, int32_t *__restrict__ idx,
                                                     float *__restrict__ val, int32_t *__restrict__ info)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int cnt = 0;
    if (t < n_cols) {
        const int64_t b = t / N;
        const int j = (int)(t - b * N);
        const float *ab = a + b * N * N + j;                     // consecutive threads: consecutive columns
        for (int i = 0; i < N; ++i) {
            const float v = ab[(int64_t)i * N];
            if (v != 0.0f) {
                if (FILL && cnt < W) {
                    idx[t * W + cnt] = i;
                    val[t * W + cnt] = v;
                }
                ++cnt;
            }
        }
        if (!FILL) cnt_out[t] = cnt;
    }
    if (!FILL) {
        int m = cnt;
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) m = max(m, __shfl_xor(m, s, 64));
        if ((threadIdx.x & 63) == 0) atomicMax(info, m);
    }
}

// ---- forward -------------------------------------------------------------------------------------------------------
// XSTAGE: x of the graph is copied to LDS first; without it x is read where it lies (the row buffers left no room)
template <bool XSTAGE>
__global__ __launch_bounds__(kBlock) void k_gcn_fwd(gnn_gcn_adj_t adj, gnn_gcn_net_t net, const float *__restrict__ x,
                                                    float *__restrict__ out, float *__restrict__ H_all, int ld,
                                                    int wstage)
{
    extern __shared__ float lds[];
    const int N = adj.N, W = adj.W, F = net.F, L = net.n_dims - 1, maxw = net.max_width;
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    float *hA = lds, *hB = hA + (size_t)N * ld, *xl = hB + (size_t)N * ld, *wl = xl + (XSTAGE ? (size_t)N * F : 0);
    const int32_t *rcnt = adj.row_cnt + b * N;
    const int32_t *ridx = adj.row_idx + b * N * W;
    const float *rval = adj.row_val + b * N * W;
    float *Hb = H_all ? H_all + b * net.n_dims * N * maxw : nullptr;

    x += b * N * F;
    const float *xs = XSTAGE ? xl : x;
    if (XSTAGE) {
        for (int t = tid; t < N * F; t += kBlock) xl[t] = x[t];
        __syncthreads();
    }

    // feature extractor: h0 = relu(x Wf^T + bf)
    {
        const int d = net.dims[0];
        for (int t = tid; t < N * d; t += kBlock) {
            const int i = t / d, o = t - i * d;
            float acc = net.bf[o];
            for (int f = 0; f < F; ++f) acc = fmaf(xs[i * F + f], net.Wf[o * F + f], acc);
            acc = relu_f(acc);
            hA[i * ld + o] = acc;
            if (Hb) Hb[(size_t)i * maxw + o] = acc;
        }
    }

    for (int l = 0; l < L; ++l) {
        const int din = net.dims[l], dout = net.dims[l + 1];
        const int cin = din + (net.residual ? F : 0);
        const float *Wn = net.Wn[l], *bn = net.bn[l], *Wg = net.Wg[l];
        if (net.residual)                                        // GCRN: hin = [h | x]
            for (int t = tid; t < N * F; t += kBlock) {
                const int i = t / F, f = t - i * F;
                hA[i * ld + din + f] = xs[t];
            }
        if (wstage) {                                            // W^T in LDS: a pass reads it with consecutive o
            for (int t = tid; t < dout * cin; t += kBlock) {
                const int o = t / cin, c = t - o * cin;
                wl[c * dout + o] = Wg[t];
                if (Wn) wl[(cin + c) * dout + o] = Wn[t];
            }
        }
        __syncthreads();
        // hB = A hin: each row pulls its neighbours, in list (ascending index) order
        for (int t = tid; t < N * cin; t += kBlock) {
            const int i = t / cin, c = t - i * cin;
            const int n = rcnt[i];
            const int32_t *ix = ridx + (size_t)i * W;
            const float *vx = rval + (size_t)i * W;
            float acc = 0.0f;
            for (int k = 0; k < n; ++k) acc = fmaf(vx[k], hA[ix[k] * ld + c], acc);
            hB[i * ld + c] = acc;
        }
        __syncthreads();
        // z over h, in place: a pass owns rpp whole rows (compute - barrier - write)
        const int rpp = kBlock / dout;
        const int r = tid / dout, o = tid - r * dout;
        float *Hl = Hb ? Hb + (size_t)(l + 1) * N * maxw : nullptr;
        for (int i0 = 0; i0 < N; i0 += rpp) {
            const int i = i0 + r;
            const bool active = r < rpp && i < N;
            float z = 0.0f;
            if (active) {
                float an = bn[o], ag = 0.0f;
                const float *hi = hA + i * ld, *gi = hB + i * ld;
                if (wstage) {
                    for (int c = 0; c < cin; ++c) ag = fmaf(gi[c], wl[c * dout + o], ag);
                    if (Wn)
                        for (int c = 0; c < cin; ++c) an = fmaf(hi[c], wl[(cin + c) * dout + o], an);
                } else {
                    for (int c = 0; c < cin; ++c) ag = fmaf(gi[c], Wg[o * cin + c], ag);
                    if (Wn)
                        for (int c = 0; c < cin; ++c) an = fmaf(hi[c], Wn[o * cin + c], an);
                }
                z = relu_f(an + ag);
            }
            __syncthreads();
            if (active) {
                hA[i * ld + o] = z;
                if (Hl) Hl[(size_t)i * maxw + o] = z;
            }
        }
        __syncthreads();
    }
    if (L == 0) __syncthreads();

    // classifier: logits
    const int dL = net.dims[L];
    for (int i = tid; i < N; i += kBlock) {
        float acc = net.bc[0];
        for (int c = 0; c < dL; ++c) acc = fmaf(hA[i * ld + c], net.Wc[c], acc);
        out[b * N + i] = acc;
    }
}

// ---- backward ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_gcn_bwd(gnn_gcn_adj_t adj, gnn_gcn_net_t net, const float *__restrict__ x,
                                                    const float *__restrict__ H_all, const float *__restrict__ gout,
                                                    float *__restrict__ gpart, int ld)
{
    extern __shared__ float lds[];
    const int N = adj.N, W = adj.W, F = net.F, L = net.n_dims - 1, maxw = net.max_width;
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    float *G = lds, *Q = G + (size_t)N * ld, *xs = Q + (size_t)N * ld, *go = xs + (size_t)N * F;
    const int32_t *ccnt = adj.col_cnt + b * N;
    const int32_t *cidx = adj.col_idx + b * N * W;
    const float *cval = adj.col_val + b * N * W;
    const float *Hb = H_all + b * net.n_dims * N * maxw;
    float *gp = gpart + b * net.n_params;

    x += b * N * F;
    for (int t = tid; t < N * F; t += kBlock) xs[t] = x[t];
    for (int i = tid; i < N; i += kBlock) go[i] = gout[b * N + i];
    __syncthreads();

    // classifier: gWc = go^T h_L, gbc = sum go, gz_L = (go Wc) * [h_L > 0]
    {
        const int dL = net.dims[L];
        const float *HL = Hb + (size_t)L * N * maxw;
        for (int c = tid; c < dL; c += kBlock) {
            gp[net.off_c + c] = sum4(N, [&](int i) { return go[i] * HL[(size_t)i * maxw + c]; });
        }
        if (tid == kBlock - 1) {
            gp[net.off_bc] = sum4(N, [&](int i) { return go[i]; });
        }
        for (int t = tid; t < N * dL; t += kBlock) {
            const int i = t / dL, o = t - i * dL;
            G[i * ld + o] = relu_open(HL[(size_t)i * maxw + o]) ? go[i] * net.Wc[o] : 0.0f;
        }
    }
    __syncthreads();

    for (int l = L - 1; l >= 0; --l) {
        const int din = net.dims[l], dout = net.dims[l + 1];
        const int cin = din + (net.residual ? F : 0);
        const float *Wn = net.Wn[l], *Wg = net.Wg[l];
        const float *Hin = Hb + (size_t)l * N * maxw;
        // q = A^T gz: each node pulls over its column list, in ascending row order
        for (int t = tid; t < N * dout; t += kBlock) {
            const int k = t / dout, o = t - k * dout;
            const int n = ccnt[k];
            const int32_t *ix = cidx + (size_t)k * W;
            const float *vx = cval + (size_t)k * W;
            float acc = 0.0f;
            for (int m = 0; m < n; ++m) acc = fmaf(vx[m], G[ix[m] * ld + o], acc);
            Q[k * ld + o] = acc;
        }
        __syncthreads();
        // weight gradients of this graph: sums over the nodes in index order
        for (int t = tid; t < dout * cin; t += kBlock) {
            const int o = t / cin, c = t - o * cin;
            const float *hc = c < din ? Hin + c : xs + (c - din);             // column c of hin = [h | x]
            const int hs = c < din ? maxw : F;
            gp[net.off_g[l] + t] = sum4(N, [&](int i) { return Q[i * ld + o] * hc[(size_t)i * hs]; });
            if (Wn) gp[net.off_n[l] + t] = sum4(N, [&](int i) { return G[i * ld + o] * hc[(size_t)i * hs]; });
        }
        for (int o = tid; o < dout; o += kBlock) gp[net.off_b[l] + o] = sum4(N, [&](int i) { return G[i * ld + o]; });
        // gz of the layer below over gz, in place: ghin = gz Wn + q Wg, masked by [h > 0]; a pass owns whole rows
        const int rpp = kBlock / din;
        const int r = tid / din, c = tid - r * din;
        for (int i0 = 0; i0 < N; i0 += rpp) {
            const int i = i0 + r;
            const bool active = r < rpp && i < N;
            float g = 0.0f;
            if (active && relu_open(Hin[(size_t)i * maxw + c])) {
                float an = 0.0f, ag = 0.0f;
                const float *gi = G + i * ld, *qi = Q + i * ld;
                for (int o = 0; o < dout; ++o) ag = fmaf(qi[o], Wg[o * cin + c], ag);
                if (Wn)
                    for (int o = 0; o < dout; ++o) an = fmaf(gi[o], Wn[o * cin + c], an);
                g = an + ag;
            }
            __syncthreads();
            if (active) G[i * ld + c] = g;
        }
        __syncthreads();
    }

    // feature extractor: gWf = gz0^T x, gbf = sum gz0
    const int d0 = net.dims[0];
    for (int t = tid; t < d0 * F; t += kBlock) {
        const int o = t / F, f = t - o * F;
        gp[net.off_f + t] = sum4(N, [&](int i) { return G[i * ld + o] * xs[i * F + f]; });
    }
    for (int o = tid; o < d0; o += kBlock) gp[net.off_bf + o] = sum4(N, [&](int i) { return G[i * ld + o]; });
}

// grads[p] = sum over the graphs, in a fixed order (sum4): the same bits in every run
__global__ __launch_bounds__(kBlock) void k_gcn_reduce(const float *__restrict__ gpart, int64_t B, int P,
                                                       float *__restrict__ grads)
{
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= P) return;
    grads[p] = sum4((int)B, [&](int b) { return gpart[(int64_t)b * P + p]; });
}

int gcn_shape_check(int N, int F, int maxw, int list_width)
{
    if (N < 1 || N > kGcnMaxNodes)
        return fail(GNN_ERR_UNSUPPORTED, "gcn: %d nodes per graph, the kernels take 1 to %d", N, kGcnMaxNodes);
    if (F < 1 || F > kGcnMaxFeatures)
        return fail(GNN_ERR_UNSUPPORTED, "gcn: input_dim %d, the kernels take 1 to %d", F, kGcnMaxFeatures);
    if (maxw < 1 || maxw > kGcnMaxWidth)
        return fail(GNN_ERR_UNSUPPORTED, "gcn: a hidden width of %d, the kernels take 1 to %d", maxw, kGcnMaxWidth);
    if (list_width < 0 || list_width > N)
        return fail(GNN_ERR_UNSUPPORTED, "gcn: a list width of %d for %d nodes (at most one entry per node)",
                    list_width, N);
    const size_t need = max(gcn_fwd_rows_lds(N, F, maxw), gcn_bwd_lds(N, F, maxw));
    if (need > (size_t)kGcnLdsMax)
        return fail(GNN_ERR_UNSUPPORTED, "gcn: %d nodes x (width %d + %d features) needs %zu bytes of LDS for the two "
                    "row buffers of the forward or the backward's two and x, the limit is %d bytes (160 KB per workgroup)",
                    N, maxw, F, need, kGcnLdsMax);
    return 0;
}

int gcn_args_check(const char *who, const gnn_gcn_adj_t *adj, const gnn_gcn_net_t *net)
{
    if (!adj || !net) return fail(GNN_ERR_BADARG, "%s: pointer missing", who);
    if (adj->B < 0 || adj->B > 0x7fffffffLL || adj->W < 1)
        return fail(GNN_ERR_BADARG, "%s: bad adjacency (B %lld, W %d)", who, (long long)adj->B, adj->W);
    if (net->n_dims < 1 || net->n_dims > GNN_GCN_MAX_LAYERS + 1)
        return fail(GNN_ERR_UNSUPPORTED, "%s: %d graph-convolution layers, the kernels take at most %d", who,
                    net->n_dims - 1, GNN_GCN_MAX_LAYERS);
    int maxw = 0;
    for (int l = 0; l < net->n_dims; ++l) {
        if (net->dims[l] < 1) return fail(GNN_ERR_BADARG, "%s: hidden_dims[%d] = %d", who, l, net->dims[l]);
        maxw = max(maxw, net->dims[l]);
    }
    if (maxw != net->max_width) return fail(GNN_ERR_BADARG, "%s: max_width %d != max(dims) %d", who, net->max_width, maxw);
    if (!net->Wf || !net->bf || !net->Wc || !net->bc) return fail(GNN_ERR_BADARG, "%s: weight pointer missing", who);
    for (int l = 0; l + 1 < net->n_dims; ++l)
        if (!net->bn[l] || !net->Wg[l]) return fail(GNN_ERR_BADARG, "%s: weight pointer missing (layer %d)", who, l);
    if (adj->B > 0 && (!adj->row_cnt || !adj->row_idx || !adj->row_val || !adj->col_cnt || !adj->col_idx || !adj->col_val))
        return fail(GNN_ERR_BADARG, "%s: adjacency pointer missing", who);
    return gcn_shape_check(adj->N, net->F, maxw, adj->W);
}

}  // namespace
}  // namespace gnn

using namespace gnn;

extern "C" {

int gnn_gcn_supported(int32_t N, int32_t F, int32_t max_width, int32_t list_width)
{
    return gcn_shape_check(N, F, max_width, list_width) == 0 ? 1 : 0;
}

int gnn_gcn_compress_count(const float *a, int64_t B, int32_t N, int32_t *row_cnt, int32_t *col_cnt, int32_t *info,
                           void *stream)
{
    ProfChain chain_;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (B < 0 || N < 1 || N > kGcnMaxNodes || B * N > 0x7fffffffLL * (kBlock / 64))
        return fail(GNN_ERR_BADARG, "gnn_gcn_compress_count: bad shape (B %lld, N %d)", (long long)B, N);
    if (!info || (B > 0 && (!a || !row_cnt || !col_cnt)))
        return fail(GNN_ERR_BADARG, "gnn_gcn_compress_count: pointer missing");
    const hipError_t err = hipMemsetAsync(info, 0, 2 * sizeof(int32_t), s);
    if (err != hipSuccess) return fail(-(int)err, "gnn_gcn_compress_count: memset failed: %s", hipGetErrorString(err));
    if (B == 0) return 0;
    const int64_t n = B * N;
    GNN_LAUNCH("k_gcn_rows", k_gcn_rows<false>, (unsigned)((n + 3) / 4), kBlock, s, a, n, N, 0, row_cnt,
               (int32_t *)nullptr, (float *)nullptr, info);
    GNN_LAUNCH("k_gcn_cols", k_gcn_cols<false>, (unsigned)((n + kBlock - 1) / kBlock), kBlock, s, a, n, N, 0, col_cnt,
               (int32_t *)nullptr, (float *)nullptr, info);
    return 0;
}

int gnn_gcn_compress_fill(const float *a, int64_t B, int32_t N, int32_t W, int32_t *row_idx, float *row_val,
                          int32_t *col_idx, float *col_val, void *stream)
{
    ProfChain chain_;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (B < 0 || N < 1 || N > kGcnMaxNodes || W < 1 || B * N > 0x7fffffffLL * (kBlock / 64))
        return fail(GNN_ERR_BADARG, "gnn_gcn_compress_fill: bad shape (B %lld, N %d, W %d)", (long long)B, N, W);
    if (B == 0) return 0;
    if (!a || !row_idx || !row_val || !col_idx || !col_val)
        return fail(GNN_ERR_BADARG, "gnn_gcn_compress_fill: pointer missing");
    const int64_t n = B * N;
    GNN_LAUNCH("k_gcn_rows", k_gcn_rows<true>, (unsigned)((n + 3) / 4), kBlock, s, a, n, N, W, (int32_t *)nullptr,
               row_idx, row_val, (int32_t *)nullptr);
    GNN_LAUNCH("k_gcn_cols", k_gcn_cols<true>, (unsigned)((n + kBlock - 1) / kBlock), kBlock, s, a, n, N, W,
               (int32_t *)nullptr, col_idx, col_val, (int32_t *)nullptr);
    return 0;
}

int gnn_gcn_forward(const gnn_gcn_adj_t *adj, const gnn_gcn_net_t *net, const float *x, float *out, float *H_all,
                    void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = gcn_args_check("gnn_gcn_forward", adj, net);
    if (rc) return rc;
    if (adj->B == 0) return 0;
    if (!x || !out) return fail(GNN_ERR_BADARG, "gnn_gcn_forward: pointer missing");
    const int N = adj->N, F = net->F, maxw = net->max_width;
    const int ld = gcn_ld(maxw, F);
    const int xstage = gcn_fwd_lds(N, F, maxw) <= (size_t)kGcnLdsMax;
    size_t lds = xstage ? gcn_fwd_lds(N, F, maxw) : gcn_fwd_rows_lds(N, F, maxw);
    // the widest layer's two matrices, transposed, beside the row buffers when they fit
    size_t wfl = 0;
    for (int l = 0; l + 1 < net->n_dims; ++l)
        wfl = max(wfl, (size_t)2 * (net->dims[l] + (net->residual ? F : 0)) * net->dims[l + 1]);
    const int wstage = wfl > 0 && lds + wfl * 4 <= (size_t)kGcnLdsMax;
    if (wstage) lds += wfl * 4;
    static DevOnce attr_done;     // dynamic LDS above 64 KB must be opted into, once per device
    if (attr_done.need()) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_gcn_fwd<true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, kGcnLdsMax);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_gcn_fwd<false>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, kGcnLdsMax);
    }
    if (xstage)
        GNN_LAUNCH_SH("k_gcn_fwd", k_gcn_fwd<true>, (unsigned)adj->B, kBlock, lds, s, *adj, *net, x, out, H_all, ld,
                      wstage);
    else
        GNN_LAUNCH_SH("k_gcn_fwd", k_gcn_fwd<false>, (unsigned)adj->B, kBlock, lds, s, *adj, *net, x, out, H_all, ld,
                      wstage);
    return 0;
}

size_t gnn_gcn_backward_workspace_bytes(int64_t B, int32_t n_params)
{
    if (B < 0 || n_params < 1) return 0;
    return align256((size_t)max((int64_t)1, B) * n_params * sizeof(float));
}

int gnn_gcn_backward(const gnn_gcn_adj_t *adj, const gnn_gcn_net_t *net, const float *x, const float *H_all,
                     const float *grad_out, float *grads, void *workspace, size_t workspace_bytes, void *stream)
{
    ProfChain chain_;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = gcn_args_check("gnn_gcn_backward", adj, net);
    if (rc) return rc;
    if (!grads || net->n_params < 1) return fail(GNN_ERR_BADARG, "gnn_gcn_backward: pointer missing");
    const size_t need = gnn_gcn_backward_workspace_bytes(adj->B, net->n_params);
    if (workspace_bytes < need || !workspace) return fail(GNN_ERR_WORKSPACE, "workspace too small: need %zu bytes", need);
    if (adj->B > 0 && (!x || !H_all || !grad_out)) return fail(GNN_ERR_BADARG, "gnn_gcn_backward: pointer missing");
    const int N = adj->N, F = net->F, maxw = net->max_width;
    float *gpart = static_cast<float *>(workspace);
    if (adj->B > 0) {
        static DevOnce attr_done;
        if (attr_done.need())
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_gcn_bwd),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, kGcnLdsMax);
        GNN_LAUNCH_SH("k_gcn_bwd", k_gcn_bwd, (unsigned)adj->B, kBlock, gcn_bwd_lds(N, F, maxw), s, *adj, *net, x, H_all,
                      grad_out, gpart, gcn_ld(maxw, 0));
    }
    GNN_LAUNCH("k_gcn_reduce", k_gcn_reduce, (unsigned)((net->n_params + kBlock - 1) / kBlock), kBlock, s, gpart,
               adj->B, net->n_params, grads);
    return 0;
}

}  // extern "C"
