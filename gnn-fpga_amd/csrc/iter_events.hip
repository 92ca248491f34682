// iter_events.hip - the per-iteration segment classifier of gnn/MPNN_Seg_Toy2D.ipynb cell 14 (include/gnn_hip_iter.h):
// the whole forward and the whole backward of one small graph in one workgroup, a different weight set per pass.
//
// Counterparts of k_event (gnn_kernels.hip) and k_event_bwd (backward.hip).  The wavefronts per graph, the LDS byte
// counts, the backward's LDS layout and the local-id copy are theirs too (event_passes.h); the stages per hit, per
// segment and per list entry are written out here, the same statements in the same order: shared functions compile to
// other register counts (profiles/event_passes_ab.txt), so a fix in a stage is made in both files.  What differs:
//   - the weights of ONE pass live in LDS (an edge set and a node set: 6 593 floats at F = 2, D = 32); the next
//     pass's set is copied in as soon as the last reader of the current one is past a barrier;
//   - the backward keeps no gradient in registers across passes: after every pass each element of that pass's
//     gradient tensors is summed over the graph's hits by ONE thread and stored to the pass's slot of the graph's row
//     of partial gradients; k_iter_fold then adds the rows in graph order.  No atomics anywhere.
#include "common.h"
#include "event_passes.h"
#include "gnn_hip_iter.h"

namespace {
using namespace gnn;

// the shapes of ModelShapes (common.h) up to hidden_dim 32 (at 64 one pass's weights alone take 103 KB of LDS)
using IterShapes = ShapeList<Shape<2, 4>, Shape<2, 8>, Shape<2, 16>, Shape<2, 32>, Shape<3, 4>, Shape<3, 8>, Shape<3, 16>,
                             Shape<3, 32>, Shape<4, 8>, Shape<4, 16>, Shape<4, 32>, Shape<11, 4>, Shape<11, 8>,
                             Shape<11, 16>>;

constexpr size_t kIterLdsMax = 128 * 1024;      // of the CU's 160 KB, as k_event

constexpr int a4(int x) { return (x + 3) & ~3; }

// where a pass's gradients go in a graph's row = the flat gradient of cell 14's SegmentClassifier in state_dict order
struct IterLayout {
    int nin, n1, n3, T;
    int ob1, oW2, ob2, ob3, oW4, ob4;           // inside an edge slot (W1 at 0) / a node slot (W3 at 0)
    __host__ __device__ IterLayout(int F, int D, int T_) : T(T_)
    {
        const int C = F + D;
        nin = D * F + D;
        ob1 = D * 2 * C, oW2 = ob1 + D, ob2 = oW2 + D, n1 = ob2 + 1;
        ob3 = D * 3 * C, oW4 = ob3 + D, ob4 = oW4 + D * D, n3 = ob4 + D;
    }
    __host__ __device__ int edge_slot(int t) const { return t < T ? nin + t * n1 : nin + T * n1 + T * n3; }
    __host__ __device__ int node_slot(int t) const { return nin + T * n1 + t * n3; }
    __host__ __device__ int stride() const { return nin + (T + 1) * n1 + T * n3; }
    __host__ __device__ int shared_floats() const { return nin + n1 + n3; }
};

// ---------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------
template <int F, int D>
struct ItFwd {
    static constexpr int C = F + D, LDH = a4(C);
    static constexpr int NWV = EvCfg<D>::NWV, NT = EvCfg<D>::NT;
    // LDS offsets (floats, 16-byte aligned) of the input network and of one pass's edge and node sets
    static constexpr int oWin = 0, obin = oWin + a4(D * F), oW1 = obin + D, ob1 = oW1 + a4(D * 2 * C), oW2 = ob1 + D,
                         ob2 = oW2 + D, oW3 = ob2 + 4, ob3 = oW3 + a4(D * 3 * C), oW4 = ob3 + D, ob4 = oW4 + D * D,
                         w_total = ob4 + D;
};

template <int F, int D>
__global__ __launch_bounds__((ItFwd<F, D>::NT)) void k_iter_event(
    gnn_graph_t g, gnn_iter_params_t p, const int32_t *__restrict__ hit_ptr, const int32_t *__restrict__ seg_ptr,
    float *__restrict__ e_out, int cap_hits, int cap_segments, float *__restrict__ e_all, float *__restrict__ H_all)
{
    using L = ItFwd<F, D>;
    constexpr int C = L::C, LDH = L::LDH, NT = L::NT, NWV = L::NWV;
    constexpr int RW = D / NWV;          // output rows of a D-row layer per wavefront
    constexpr int RP = 2 * D / NWV;      // rows of the stacked [P; Q] per wavefront
    static_assert(D % NWV == 0 && RW >= 1, "rows are dealt to the wavefronts");
    extern __shared__ __attribute__((aligned(16))) float it_lds[];
    float *H = it_lds, *Hn = H + cap_hits * LDH, *PQ = Hn + cap_hits * LDH, *qb = PQ + cap_hits * 2 * D,
          *Mb = qb + cap_hits * D, *es = Mb + cap_hits * 2 * LDH, *wl = es + ((cap_segments + 3) & ~3);
    int32_t *ip = reinterpret_cast<int32_t *>(wl + L::w_total), *op = ip + cap_hits + 1, *ie = op + cap_hits + 1,
            *inb = ie + cap_segments, *oe = inb + cap_segments, *onb = oe + cap_segments, *sl = onb + cap_segments,
            *dl = sl + cap_segments;
    const int h0 = hit_ptr[blockIdx.x], nh = hit_ptr[blockIdx.x + 1] - h0;
    const int s0 = seg_ptr[blockIdx.x], ns = seg_ptr[blockIdx.x + 1] - s0;
    const int T = p.n_iters;
    const float *__restrict__ X = g.X;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;

    auto copy_in = [&](float *dst, const float *__restrict__ src, int n) {
        for (int i = threadIdx.x; i < n; i += NT) dst[i] = src[i];
    };
    // edge pass t reads edge_networks[t]; the pass after the last node pass reads output_network
    auto stage_edge = [&](int t) {
        const gnn_iter_set_t s = t < T ? p.edge[t] : p.out;
        copy_in(wl + L::oW1, s.Wa, D * 2 * C);
        copy_in(wl + L::ob1, s.ba, D);
        copy_in(wl + L::oW2, s.Wb, D);
        copy_in(wl + L::ob2, s.bb, 1);
    };
    auto stage_node = [&](int t) {
        const gnn_iter_set_t s = p.node[t];
        copy_in(wl + L::oW3, s.Wa, D * 3 * C);
        copy_in(wl + L::ob3, s.ba, D);
        copy_in(wl + L::oW4, s.Wb, D * D);
        copy_in(wl + L::ob4, s.bb, D);
    };
    const float *Win = wl + L::oWin, *bin = wl + L::obin, *W1 = wl + L::oW1, *b1 = wl + L::ob1, *W2 = wl + L::oW2,
                *b2 = wl + L::ob2, *W3 = wl + L::oW3, *b3 = wl + L::ob3, *W4 = wl + L::oW4, *b4 = wl + L::ob4;
    copy_in(wl + L::oWin, p.Win, D * F);
    copy_in(wl + L::obin, p.bin, D);
    stage_edge(0);
    if (T > 0) stage_node(0);
    // the graph's index arrays as LOCAL ids: the text of ev_local_lists / ev_local_ends (event_passes.h), kept here -
    // through the shared functions this kernel alone compiles to 13 more SGPR spills at hidden_dim 32
    if (nh > 0) {
        const int ib = g.in_ptr[h0], ob = g.out_ptr[h0];
        for (int n = threadIdx.x; n <= nh; n += NT) {
            ip[n] = g.in_ptr[h0 + n] - ib;
            op[n] = g.out_ptr[h0 + n] - ob;
        }
        const int ni = g.in_ptr[h0 + nh] - ib, no = g.out_ptr[h0 + nh] - ob;
        for (int k = threadIdx.x; k < ni; k += NT) {
            ie[k] = g.in_eid[ib + k] - s0;
            inb[k] = g.in_nbr[ib + k] - h0;
        }
        for (int k = threadIdx.x; k < no; k += NT) {
            oe[k] = g.out_eid[ob + k] - s0;
            onb[k] = g.out_nbr[ob + k] - h0;
        }
    }
    for (int j = threadIdx.x; j < ns; j += NT) {
        const int sg = g.src[s0 + j];
        sl[j] = sg < 0 ? -1 : sg - h0;
        dl[j] = sg < 0 ? -1 : g.dst[s0 + j] - h0;
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
            for (int r = 0; r < RP; ++r) acc[r] = isq ? 0.0f : b1[d0 + r];
#pragma unroll
            for (int c = 0; c < LDH / 4; ++c)
                fma_piece(acc, W1 + d0 * 2 * C + (isq ? C : 0), 2 * C, c,
                          *reinterpret_cast<const float4 *>(Hsrc + n * LDH + 4 * c), std::integral_constant<int, RP>{});
#pragma unroll
            for (int r = 0; r < RP; ++r) PQ[n * 2 * D + row0 + r] = acc[r];
        }
    };
    auto keep_rows = [&](const float *Hsrc, int t) {
        if (H_all)
            for (int i = threadIdx.x; i < nh * LDH; i += NT) H_all[((int64_t)t * g.n_hits + h0) * LDH + i] = Hsrc[i];
    };

    // input network (k_input): rows of tanh(Win x + bin) per wavefront
    for (int n = lane; n < nh; n += 64) {
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            const int d = wv * RW + r;
            float acc = bin[d];
#pragma unroll
            for (int k = 0; k < F; ++k) acc = fmaf(Win[d * F + k], H[n * LDH + D + k], acc);
            H[n * LDH + d] = tanh_f(acc);
        }
    }
    __syncthreads();
    keep_rows(H, 0);
    pq_rows(H);
    __syncthreads();

    for (int t = 0;; ++t) {
        const bool last = (t == T);
        // edge pass (k_edge) with set t: one segment per lane of the workgroup
        for (int j = threadIdx.x; j < ns; j += NT) {
            const int s = sl[j], d = dl[j];
            float acc = b2[0];
#pragma unroll
            for (int v = 0; v < D / 4; ++v) {
                float4 z;
                if (s >= 0) {
                    const float4 a = reinterpret_cast<const float4 *>(PQ + s * 2 * D)[v];
                    const float4 b = reinterpret_cast<const float4 *>(PQ + d * 2 * D + D)[v];
                    z = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
                } else {
                    z = make_float4(b1[4 * v], b1[4 * v + 1], b1[4 * v + 2], b1[4 * v + 3]);
                }
                acc = fmaf(W2[4 * v], tanh_f(z.x), acc);
                acc = fmaf(W2[4 * v + 1], tanh_f(z.y), acc);
                acc = fmaf(W2[4 * v + 2], tanh_f(z.z), acc);
                acc = fmaf(W2[4 * v + 3], tanh_f(z.w), acc);
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
        stage_edge(t + 1);      // set t has had its last reader; set t + 1 is first read after two more barriers
        // node pass (k_node) with set t.  Step 1: the segment sums mi, mo of every hit (local CSR, ascending segment id)
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
            for (int r = 0; r < RW; ++r) acc[r] = b3[d0 + r];
#pragma unroll 1
            for (int part = 0; part < 3; ++part) {
                const float *mrow = part == 2 ? H + n * LDH : Mb + n * 2 * LDH + part * LDH;
#pragma unroll
                for (int c = 0; c < LDH / 4; ++c)
                    fma_piece(acc, W3 + d0 * 3 * C + part * C, 3 * C, c, *reinterpret_cast<const float4 *>(mrow + 4 * c),
                              std::integral_constant<int, RW>{});
            }
#pragma unroll
            for (int r = 0; r < RW; ++r) qb[n * D + d0 + r] = tanh_f(acc[r]);
        }
        for (int i = threadIdx.x; i < nh * (LDH - D); i += NT) {   // shortcut: X again behind the new columns
            const int n = i / (LDH - D), k = D + i % (LDH - D);
            Hn[n * LDH + k] = H[n * LDH + k];
        }
        __syncthreads();
        for (int n = lane; n < nh; n += 64) {                // second layer: rows per wavefront
            const int d0 = wv * RW;
            float acc[RW];
#pragma unroll
            for (int r = 0; r < RW; ++r) acc[r] = b4[d0 + r];
#pragma unroll
            for (int c = 0; c < D / 4; ++c) {
                const float4 v = *reinterpret_cast<const float4 *>(qb + n * D + 4 * c);
                const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < RW; ++r) acc[r] = fmaf(W4[(d0 + r) * D + 4 * c + j], vv[j], acc[r]);
            }
#pragma unroll
            for (int r = 0; r < RW; ++r) Hn[n * LDH + d0 + r] = tanh_f(acc[r]);
        }
        __syncthreads();
        if (t + 1 < T) stage_node(t + 1);                    // first read after the barrier below
        keep_rows(Hn, t + 1);
        pq_rows(Hn);                                         // P / Q for edge set t + 1
        __syncthreads();
        float *tmp = H; H = Hn; Hn = tmp;
    }
}

// ---------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------
// One pass's weight gradient: out[index(l, k)] = sum over the graph's hits of L[n][l] * R[n][k], R taken in 4-float
// pieces (index < 0: a padding column), then the NB plain sums of L's first columns (the bias, + bias_add[l] if
// given).  One thread per element group, hits ascending: the same sums as Outer4 of k_event_bwd, stored, not added.
template <int NL, int NR4, int NB, typename Index>
__device__ __forceinline__ void outer_store(int nh, const float *L, int ls, const float *R, int rs, float *out,
                                            Index index, int bias0, const float *bias_add)
{
    for (int r = threadIdx.x; r < NL * NR4 + NB; r += kBlock) {
        if (r < NL * NR4) {
            const float *l = L + r / NR4, *rr = R + 4 * (r % NR4);
            float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            for (int n = 0; n < nh; ++n) {
                const float lv = l[n * ls];
                const float4 rv = *reinterpret_cast<const float4 *>(rr + n * rs);
                a.x = fmaf(lv, rv.x, a.x); a.y = fmaf(lv, rv.y, a.y);
                a.z = fmaf(lv, rv.z, a.z); a.w = fmaf(lv, rv.w, a.w);
            }
            const float v[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int o = index(r / NR4, 4 * (r % NR4) + j);
                if (o >= 0) out[o] = v[j];
            }
        } else {
            const int b = r - NL * NR4;
            float a = 0.0f;
            for (int n = 0; n < nh; ++n) a += L[n * ls + b];
            out[bias0 + b] = bias_add ? a + bias_add[b] : a;
        }
    }
}

template <int F, int D>
__global__ __launch_bounds__(kBlock) void k_iter_event_bwd(
    gnn_graph_t g, gnn_iter_params_t p, const int32_t *__restrict__ hit_ptr, const int32_t *__restrict__ seg_ptr,
    const float *__restrict__ e_all, const float *__restrict__ H_all, const float *__restrict__ grad_out,
    float *__restrict__ rep, int cap_h, int cap_s)
{
    using B = EvBwd<F, D>;
    constexpr int C = B::C, LDH = B::LDH, NT = kBlock, NW = NT / 64, NS = D + 2;
    extern __shared__ __attribute__((aligned(16))) float ib_lds[];
    __shared__ float red[NW * NS];      // the wavefronts' per-segment sums of one edge pass
    __shared__ float padv[D];           // the padded segments' share of that pass's gb1
    const int s4 = (cap_s + 3) & ~3;
    float *Hc = ib_lds, *Hp = Hc + cap_h * LDH, *gH = Hp + cap_h * LDH, *gHp = gH + cap_h * LDH,
          *gmio = gHp + cap_h * LDH, *Mr = gmio + cap_h * 2 * LDH, *PQ = Mr + cap_h * 3 * LDH, *fa = PQ + cap_h * 2 * D,
          *qb = fa + cap_h * 2 * D, *ec = qb + cap_h * D, *gu = ec + s4, *wl = gu + s4;
    int32_t *ip = reinterpret_cast<int32_t *>(wl + B::w_total), *op = ip + cap_h + 1, *ie = op + cap_h + 1,
            *inb = ie + cap_s, *oe = inb + cap_s, *onb = oe + cap_s, *sl = onb + cap_s, *dl = sl + cap_s;
    const int tid = threadIdx.x;
    const int h0 = hit_ptr[blockIdx.x], nh = hit_ptr[blockIdx.x + 1] - h0;
    const int s0 = seg_ptr[blockIdx.x], ns = seg_ptr[blockIdx.x + 1] - s0;
    const int64_t N = g.n_hits, E = g.n_segments;
    const int T = p.n_iters;
    const IterLayout lay(F, D, T);
    rep += (int64_t)blockIdx.x * lay.stride();          // this graph's row

    auto stage_edge = [&](int t) {
        const gnn_iter_set_t s = t < T ? p.edge[t] : p.out;
        const float *__restrict__ w1 = s.Wa, *__restrict__ bb1 = s.ba, *__restrict__ w2 = s.Wb;
        for (int i = tid; i < D * 2 * LDH; i += NT) {
            const int d = i / (2 * LDH), blk = (i / LDH) % 2, k = i % LDH;
            wl[B::oW1 + i] = k < C ? w1[d * 2 * C + blk * C + k] : 0.0f;
        }
        for (int i = tid; i < D; i += NT) {
            wl[B::ob1 + i] = bb1[i];
            wl[B::oW2 + i] = w2[i];
        }
    };
    auto stage_node = [&](int t) {
        const gnn_iter_set_t s = p.node[t];
        const float *__restrict__ w3 = s.Wa, *__restrict__ bb3 = s.ba, *__restrict__ w4 = s.Wb;
        for (int i = tid; i < D * 3 * LDH; i += NT) {
            const int d = i / (3 * LDH), blk = (i / LDH) % 3, k = i % LDH;
            wl[B::oW3 + i] = k < C ? w3[d * 3 * C + blk * C + k] : 0.0f;
        }
        for (int i = tid; i < D * D; i += NT) wl[B::oW4 + i] = w4[i];
        for (int i = tid; i < D; i += NT) wl[B::ob3 + i] = bb3[i];
    };
    const float *W1 = wl + B::oW1, *b1 = wl + B::ob1, *W2 = wl + B::oW2, *W3 = wl + B::oW3, *b3 = wl + B::ob3,
                *W4 = wl + B::oW4;
    stage_edge(T);                                      // the last pass is output_network's
    const EvIds ids = {ip, op, ie, inb, oe, onb, sl, dl};       // the graph's index arrays as LOCAL ids
    if (nh > 0) ev_local_lists<NT>(g, h0, nh, s0, ids);
    ev_local_ends<NT>(g, h0, s0, ns, ids);
    for (int i = tid; i < nh * LDH; i += NT) {
        gH[i] = gHp[i] = 0.0f;                  // (padding columns stay zero: nothing writes them)
        gmio[2 * i] = gmio[2 * i + 1] = 0.0f;
        Hc[i] = H_all[((int64_t)T * N + h0) * LDH + i];
    }
    for (int j = tid; j < ns; j += NT) ec[j] = e_all[(int64_t)T * E + s0 + j];
    __syncthreads();

    for (int t = T;; --t) {
        float *slot_e = rep + lay.edge_slot(t);
        // P/Q rows of H_t (kb_pq) with edge set t: one (hit, row) per thread
        for (int i = tid; i < nh * 2 * D; i += NT) {
            const int n = i / (2 * D), r = i % (2 * D), d = r % D;
            const bool isq = r >= D;
            float acc = isq ? 0.0f : b1[d];
            const float4 *w = reinterpret_cast<const float4 *>(W1 + d * 2 * LDH + (isq ? LDH : 0));
            const float4 *h = reinterpret_cast<const float4 *>(Hc + n * LDH);
#pragma unroll
            for (int c = 0; c < LDH / 4; ++c) {      // (padding columns add 0 * 0: the sums are unchanged)
                const float4 a = w[c], b = h[c];
                acc = fmaf(a.x, b.x, acc); acc = fmaf(a.y, b.y, acc);
                acc = fmaf(a.z, b.z, acc); acc = fmaf(a.w, b.w, acc);
            }
            PQ[n * 2 * D + r] = acc;
        }
        __syncthreads();
        // edge pass t (k_edge_bwd): gu per segment, this thread's sums for gW2 / gb2 / the padded share of gb1
        {
            float sW2[D], sb2 = 0.0f, spad = 0.0f;
#pragma unroll
            for (int i = 0; i < D; ++i) sW2[i] = 0.0f;
            for (int j = tid; j < ns; j += NT) {
                const int s = sl[j], d = dl[j];
                const float ev = ec[j];
                float gej = 0.0f;
                if (t == T) {
                    gej = grad_out[s0 + j];
                } else if (s >= 0) {
#pragma unroll
                    for (int c = 0; c < C; ++c) gej = fmaf(gmio[d * 2 * LDH + c], Hc[s * LDH + c], gej);
#pragma unroll
                    for (int c = 0; c < C; ++c) gej = fmaf(gmio[s * 2 * LDH + LDH + c], Hc[d * LDH + c], gej);
                }
                const float guv = gej * ev * (1.0f - ev);
                if (s >= 0) {
#pragma unroll
                    for (int i = 0; i < D; ++i)
                        sW2[i] = fmaf(guv, tanh_f(PQ[s * 2 * D + i] + PQ[d * 2 * D + D + i]), sW2[i]);
                } else {
#pragma unroll
                    for (int i = 0; i < D; ++i) sW2[i] = fmaf(guv, tanh_f(b1[i]), sW2[i]);
                    spad += guv;
                }
                sb2 += guv;
                gu[j] = guv;
            }
            // a fixed butterfly inside the wavefront, then the wavefronts in order
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                float x = i < D ? sW2[i < D ? i : 0] : i == D ? sb2 : spad;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
                if ((tid & 63) == 0) red[(tid >> 6) * NS + i] = x;
            }
        }
        __syncthreads();
        if (tid <= D) {                                 // gW2, gb2 of pass t
            float x = 0.0f;
#pragma unroll
            for (int w = 0; w < NW; ++w) x += red[w * NS + tid];
            slot_e[tid < D ? lay.oW2 + tid : lay.ob2] = x;
        } else if (tid < 2 * D + 1) {
            const int i = tid - D - 1;
            float x = 0.0f;
#pragma unroll
            for (int w = 0; w < NW; ++w) x += red[w * NS + D + 1];
            const float a = tanh_f(b1[i]);
            padv[i] = x != 0.0f ? x * W2[i] * (1.0f - a * a) : 0.0f;
        }
        // k_pq_bwd: gP = sum_out gz, gQ = sum_in gz, one (hit, P|Q, 4 hidden units) per thread -> fa = [gP | gQ]
        for (int i = tid; i < nh * 2 * (D / 4); i += NT) {
            const int n = i / (2 * (D / 4)), part = (i / (D / 4)) & 1, v = i % (D / 4);
            const float4 own = *reinterpret_cast<const float4 *>(PQ + n * 2 * D + part * D + 4 * v);
            const float4 w2 = *reinterpret_cast<const float4 *>(W2 + 4 * v);
            const int32_t *el = part ? ie : oe, *nl = part ? inb : onb;
            float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            for (int k = part ? ip[n] : op[n], k1 = part ? ip[n + 1] : op[n + 1]; k < k1; ++k) {
                const float gk = gu[el[k]];
                // out-walk: P[n] + Q[end hit];  in-walk: P[start hit] + Q[n]
                const float4 o = *reinterpret_cast<const float4 *>(PQ + nl[k] * 2 * D + (part ? 0 : D) + 4 * v);
                const float ax = tanh_f(own.x + o.x), ay = tanh_f(own.y + o.y), az = tanh_f(own.z + o.z),
                            aw = tanh_f(own.w + o.w);
                acc.x += gk * w2.x * (1.0f - ax * ax);
                acc.y += gk * w2.y * (1.0f - ay * ay);
                acc.z += gk * w2.z * (1.0f - az * az);
                acc.w += gk * w2.w * (1.0f - aw * aw);
            }
            *reinterpret_cast<float4 *>(fa + n * 2 * D + part * D + 4 * v) = acc;
        }
        __syncthreads();
        for (int i = tid; i < nh * C; i += NT) {            // gH += W1a^T gP + W1b^T gQ
            const int n = i / C, k = i % C;
            float acc = 0.0f;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                acc = fmaf(W1[d * 2 * LDH + k], fa[n * 2 * D + d], acc);
                acc = fmaf(W1[d * 2 * LDH + LDH + k], fa[n * 2 * D + D + d], acc);
            }
            gH[n * LDH + k] += acc;
        }
        // gW1, gb1 of pass t: [gP | gQ] (x) H_t
        outer_store<2 * D, LDH / 4, D>(nh, fa, 2 * D, Hc, LDH, slot_e,
                                       [](int l, int kk) { return kk < C ? (l % D) * 2 * C + (l / D) * C + kk : -1; },
                                       lay.ob1, padv);
        __syncthreads();
        if (t == 0) break;
        // node pass t-1 -> t (k_node_bwd) with node set t-1: H_{t-1}, e_{t-1} in; Hc = H_t holds the pass's outputs.
        // Edge set t-1 comes in with it: set t had its last reader before the barrier above.
        float *slot_n = rep + lay.node_slot(t - 1);
        stage_node(t - 1);
        stage_edge(t - 1);
        for (int i = tid; i < nh * LDH; i += NT) Hp[i] = H_all[((int64_t)(t - 1) * N + h0) * LDH + i];
        for (int j = tid; j < ns; j += NT) ec[j] = e_all[(int64_t)(t - 1) * E + s0 + j];
        __syncthreads();
        // M = [mi | mo | h], rows padded to LDH: one (hit, part, 4-float piece) per thread
        for (int i = tid; i < nh * 3 * (LDH / 4); i += NT) {
            const int n = i / (3 * (LDH / 4)), part = (i / (LDH / 4)) % 3, c = i % (LDH / 4);
            float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (part == 2) {
                m = *reinterpret_cast<const float4 *>(Hp + n * LDH + 4 * c);
            } else {
                const int32_t *el = part ? oe : ie, *nl = part ? onb : inb;
                for (int k = part ? op[n] : ip[n], k1 = part ? op[n + 1] : ip[n + 1]; k < k1; ++k) {
                    const float w = ec[el[k]];
                    const float4 a = *reinterpret_cast<const float4 *>(Hp + nl[k] * LDH + 4 * c);
                    m.x = fmaf(w, a.x, m.x);
                    m.y = fmaf(w, a.y, m.y);
                    m.z = fmaf(w, a.z, m.z);
                    m.w = fmaf(w, a.w, m.w);
                }
            }
            *reinterpret_cast<float4 *>(Mr + n * 3 * LDH + part * LDH + 4 * c) = m;
        }
        __syncthreads();
        for (int i = tid; i < nh * D; i += NT) {             // q and gr
            const int n = i / D, d = i % D;
            float acc = b3[d];
            const float4 *w = reinterpret_cast<const float4 *>(W3 + d * 3 * LDH);
            const float4 *mrow = reinterpret_cast<const float4 *>(Mr + n * 3 * LDH);
#pragma unroll
            for (int c = 0; c < 3 * LDH / 4; ++c) {
                const float4 a = w[c], b = mrow[c];
                acc = fmaf(a.x, b.x, acc); acc = fmaf(a.y, b.y, acc);
                acc = fmaf(a.z, b.z, acc); acc = fmaf(a.w, b.w, acc);
            }
            qb[i] = tanh_f(acc);
            const float hn = Hc[n * LDH + d];
            fa[n * 2 * D + d] = gH[n * LDH + d] * (1.0f - hn * hn);
        }
        __syncthreads();
        for (int i = tid; i < nh * D; i += NT) {             // gp
            const int n = i / D, k = i % D;
            float acc = 0.0f;
#pragma unroll
            for (int d = 0; d < D; ++d) acc = fmaf(W4[d * D + k], fa[n * 2 * D + d], acc);
            fa[n * 2 * D + D + k] = acc * (1.0f - qb[i] * qb[i]);
        }
        __syncthreads();
        for (int i = tid; i < nh * 3 * C; i += NT) {         // gM -> gmi | gmo | gH_prev (self part)
            const int n = i / (3 * C), k = i % (3 * C);
            float acc = 0.0f;
#pragma unroll
            for (int d = 0; d < D; ++d) acc = fmaf(W3[d * 3 * LDH + (k / C) * LDH + k % C], fa[n * 2 * D + D + d], acc);
            if (k < C) gmio[n * 2 * LDH + k] = acc;
            else if (k < 2 * C) gmio[n * 2 * LDH + LDH + (k - C)] = acc;
            else gHp[n * LDH + (k - 2 * C)] = acc;
        }
        // gW3, gb3 = gp (x) [mi | mo | h];  gW4, gb4 = gr (x) q   (node set t-1)
        outer_store<D, 3 * LDH / 4, D>(nh, fa + D, 2 * D, Mr, 3 * LDH, slot_n,
                                       [](int l, int kk) { return kk % LDH < C ? l * 3 * C + (kk / LDH) * C + kk % LDH : -1; },
                                       lay.ob3, nullptr);
        outer_store<D, D / 4, D>(nh, fa, 2 * D, qb, D, slot_n, [&](int l, int kk) { return lay.oW4 + l * D + kk; }, lay.ob4,
                                 nullptr);
        __syncthreads();
        for (int i = tid; i < nh * (LDH / 4); i += NT) {     // k_agg_bwd_n, 4 columns per thread
            const int n = i / (LDH / 4), c = i % (LDH / 4);
            float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            for (int k = op[n]; k < op[n + 1]; ++k) {
                const float w = ec[oe[k]];
                const float4 a = *reinterpret_cast<const float4 *>(gmio + onb[k] * 2 * LDH + 4 * c);
                acc.x = fmaf(w, a.x, acc.x); acc.y = fmaf(w, a.y, acc.y);
                acc.z = fmaf(w, a.z, acc.z); acc.w = fmaf(w, a.w, acc.w);
            }
            for (int k = ip[n]; k < ip[n + 1]; ++k) {
                const float w = ec[ie[k]];
                const float4 a = *reinterpret_cast<const float4 *>(gmio + inb[k] * 2 * LDH + LDH + 4 * c);
                acc.x = fmaf(w, a.x, acc.x); acc.y = fmaf(w, a.y, acc.y);
                acc.z = fmaf(w, a.z, acc.z); acc.w = fmaf(w, a.w, acc.w);
            }
            float4 *dst = reinterpret_cast<float4 *>(gHp + n * LDH + 4 * c);
            const float4 old = *dst;
            *dst = make_float4(old.x + acc.x, old.y + acc.y, old.z + acc.z, old.w + acc.w);
        }
        __syncthreads();
        float *tmp = gH; gH = gHp; gHp = tmp;
        tmp = Hc; Hc = Hp; Hp = tmp;          // H_{t-1} is the next pass's H_t; ec already holds e_{t-1}
    }
    // input network (k_input_bwd): Hc = H_0
    for (int i = tid; i < nh * D; i += NT) {
        const int n = i / D, d = i % D;
        const float h = Hc[n * LDH + d];
        fa[n * 2 * D + d] = gH[n * LDH + d] * (1.0f - h * h);
    }
    __syncthreads();
    outer_store<D, (LDH - D) / 4, D>(nh, fa, 2 * D, Hc + D, LDH, rep, [](int l, int kk) { return kk < F ? l * F + kk : -1; },
                                     D * F, nullptr);
}

// out[j] = the rows' element j added in row order.  Shared weights (cell 14, SegmentClassifier2): out is the
// ten-tensor layout, and an element of the one edge / node network is its slots added in pass order, each slot
// over the rows in row order.
__global__ __launch_bounds__(kBlock) void k_iter_fold(const float *__restrict__ rep, int64_t rows, int64_t stride,
                                                      float *__restrict__ out, int n_out, IterLayout lay, int shared)
{
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n_out) return;
    int first = j, step = 0, slots = 1, extra = -1;
    if (shared && j >= lay.nin) {
        if (j < lay.nin + lay.n1) {
            first = j, step = lay.n1, slots = lay.T, extra = lay.edge_slot(lay.T) + (j - lay.nin);
        } else {
            first = lay.node_slot(0) + (j - lay.nin - lay.n1), step = lay.n3, slots = lay.T;
        }
    }
    float acc = 0.0f;
    for (int t = 0; t < slots; ++t)
        for (int64_t r = 0; r < rows; ++r) acc += rep[r * stride + first + (int64_t)t * step];
    if (extra >= 0)
        for (int64_t r = 0; r < rows; ++r) acc += rep[r * stride + extra];
    out[j] = acc;
}

template <int F, int D>
int run_iter_forward(const gnn_graph_t *g, const gnn_iter_params_t *p, const int32_t *hit_ptr, const int32_t *seg_ptr,
                     int64_t n_graphs, int cap_h, int cap_s, float *e_out, float *e_all, float *H_all, hipStream_t s)
{
    using L = ItFwd<F, D>;
    if (n_graphs <= 0) return 0;
    static DevOnce attr_done;     // dynamic LDS above 64 KB must be opted into, once per device
    if (attr_done.need())
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_iter_event<F, D>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)kIterLdsMax);
    const size_t lds = ev_fwd_lds_bytes(F, D, cap_h, cap_s, L::w_total);
    GNN_LAUNCH_SH("k_iter_event", (k_iter_event<F, D>), (unsigned)n_graphs, L::NT, lds, s, *g, *p, hit_ptr, seg_ptr, e_out,
                  cap_h, cap_s, e_all, H_all);
    return 0;
}

int fold(const float *rep, int64_t rows, const IterLayout &lay, int shared, float *out, hipStream_t s)
{
    const int n_out = shared ? lay.shared_floats() : lay.stride();
    GNN_LAUNCH("k_iter_fold", k_iter_fold, (unsigned)((n_out + kBlock - 1) / kBlock), kBlock, s, rep, rows,
               (int64_t)lay.stride(), out, n_out, lay, shared);
    return 0;
}

template <int F, int D>
int run_iter_backward(const gnn_graph_t *g, const gnn_iter_params_t *p, const int32_t *hit_ptr, const int32_t *seg_ptr,
                      int64_t n_graphs, int cap_h, int cap_s, const float *e_all, const float *H_all,
                      const float *grad_out, float *grads_flat, char *ws, hipStream_t s)
{
    float *rep = reinterpret_cast<float *>(ws);
    if (n_graphs > 0) {
        static DevOnce attr_done;
        if (attr_done.need())
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_iter_event_bwd<F, D>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)kIterLdsMax);
        const size_t lds = EvBwd<F, D>::lds_bytes(cap_h, cap_s);
        GNN_LAUNCH_SH("k_iter_event_bwd", (k_iter_event_bwd<F, D>), (unsigned)n_graphs, kBlock, lds, s, *g, *p, hit_ptr,
                      seg_ptr, e_all, H_all, grad_out, rep, cap_h, cap_s);
    }
    return fold(rep, n_graphs, IterLayout(F, D, p->n_iters), p->shared, grads_flat, s);
}

// ---- the input network's backward on its own (models that run the passes module by module) ------------------
constexpr int kInChunk = 1024;      // hits per workgroup

__global__ __launch_bounds__(kBlock) void k_iter_input_bwd(const float *__restrict__ X, const float *__restrict__ H0,
                                                           int ldh, const float *__restrict__ gH0, int ldg,
                                                           int64_t n_hits, int F, int D, float *__restrict__ partial)
{
    const int64_t n0 = (int64_t)blockIdx.x * kInChunk, n1 = n0 + kInChunk < n_hits ? n0 + kInChunk : n_hits;
    float *row = partial + (int64_t)blockIdx.x * (D * F + D);
    for (int r = threadIdx.x; r < D * F + D; r += kBlock) {
        const bool bias = r >= D * F;
        const int d = bias ? r - D * F : r / F, k = bias ? 0 : r % F;
        float acc = 0.0f;
        for (int64_t n = n0; n < n1; ++n) {
            const float h = H0[n * ldh + d];
            const float gz = gH0[n * ldg + d] * (1.0f - h * h);
            acc = bias ? acc + gz : fmaf(gz, X[n * F + k], acc);
        }
        row[r] = acc;
    }
}

int check_params(const char *who, const gnn_iter_params_t *p)
{
    if (!p) return fail(GNN_ERR_BADARG, "%s: params missing", who);
    if (p->n_iters < 0 || p->n_iters > GNN_ITER_MAX)
        return fail(GNN_ERR_BADARG, "%s: n_iters must be in [0, %d], got %d", who, GNN_ITER_MAX, p->n_iters);
    if (!IterShapes::has(p->F, p->D))
        return fail(GNN_ERR_UNSUPPORTED, "%s: no per-iteration kernel for input_dim=%d hidden_dim=%d", who, p->F, p->D);
    auto whole = [](const gnn_iter_set_t &s) { return s.Wa && s.ba && s.Wb && s.bb; };
    auto same = [](const gnn_iter_set_t &a, const gnn_iter_set_t &b) {
        return a.Wa == b.Wa && a.ba == b.ba && a.Wb == b.Wb && a.bb == b.bb;
    };
    if (!p->Win || !p->bin || !whole(p->out)) return fail(GNN_ERR_BADARG, "%s: a weight tensor is missing", who);
    for (int t = 0; t < p->n_iters; ++t) {
        if (!whole(p->edge[t]) || !whole(p->node[t]))
            return fail(GNN_ERR_BADARG, "%s: a weight tensor of iteration %d is missing", who, t);
        if (p->shared && (!same(p->edge[t], p->out) || !same(p->node[t], p->node[0])))
            return fail(GNN_ERR_BADARG, "%s: shared = 1 but iteration %d has tensors of its own", who, t);
    }
    return 0;
}

int check_batch(const char *who, const gnn_graph_t *g, const int32_t *hit_ptr, const int32_t *seg_ptr, int64_t n_graphs,
                int32_t max_hits, int32_t max_segments)
{
    if (!g || n_graphs < 0 || max_hits < 0 || max_segments < 0 || g->n_hits < 0 || g->n_segments < 0)
        return fail(GNN_ERR_BADARG, "%s: bad argument", who);
    if (n_graphs > 0 && (!hit_ptr || !seg_ptr)) return fail(GNN_ERR_BADARG, "%s: graph offsets missing", who);
    if (g->n_hits > 0 && (!g->X || !g->in_ptr || !g->out_ptr)) return fail(GNN_ERR_BADARG, "%s: hit arrays missing", who);
    if (g->n_segments > 0 && (!g->src || !g->dst || !g->in_eid || !g->in_nbr || !g->out_eid || !g->out_nbr))
        return fail(GNN_ERR_BADARG, "%s: segment arrays missing", who);
    return 0;
}

}  // namespace

using namespace gnn;

extern "C" {

int gnn_iter_events_supported(int32_t F, int32_t D, int64_t max_hits, int64_t max_segments, int32_t backward)
{
    if (max_hits < 0 || max_segments < 0 || max_hits >= (1 << 20) || max_segments >= (1 << 24)) return 0;
    return IterShapes::find<int>(F, D, 0, [&](auto sh) {
        return ev_fwd_lds_bytes(sh.F, sh.D, max_hits, max_segments, ItFwd<sh.F, sh.D>::w_total) <= kIterLdsMax &&
               (!backward || EvBwd<sh.F, sh.D>::lds_bytes(max_hits, max_segments) <= kIterLdsMax); });
}

int gnn_iter_forward_events(const gnn_graph_t *g, const gnn_iter_params_t *p, const int32_t *hit_ptr,
                            const int32_t *seg_ptr, int64_t n_graphs, int32_t max_hits, int32_t max_segments,
                            float *e_out, float *e_all, float *H_all, void *stream)
{
    const char *who = "gnn_iter_forward_events";
    if (int rc = check_params(who, p)) return rc;
    if (int rc = check_batch(who, g, hit_ptr, seg_ptr, n_graphs, max_hits, max_segments)) return rc;
    // (an array of no elements may be NULL: a batch without segments has no e_all, one without hits no H_all)
    if ((e_all && !H_all && g->n_hits > 0) || (H_all && !e_all && g->n_segments > 0))
        return fail(GNN_ERR_BADARG, "%s: e_all and H_all come together or not at all", who);
    if (!e_out && !e_all && g->n_segments > 0) return fail(GNN_ERR_BADARG, "%s: no output asked for", who);
    if (!gnn_iter_events_supported(p->F, p->D, max_hits, max_segments, 0))
        return fail(GNN_ERR_UNSUPPORTED, "%s: graphs of up to %d hits / %d segments do not fit one workgroup's LDS at "
                    "input_dim=%d hidden_dim=%d", who, max_hits, max_segments, p->F, p->D);
    return IterShapes::find<int>(p->F, p->D, GNN_ERR_UNSUPPORTED, [&](auto sh) {      // (check_params: the shape is listed)
        return run_iter_forward<sh.F, sh.D>(g, p, hit_ptr, seg_ptr, n_graphs, max_hits, max_segments, e_out, e_all, H_all,
                                            static_cast<hipStream_t>(stream)); });
}

int64_t gnn_iter_grad_floats(int32_t F, int32_t D, int32_t n_iters, int32_t shared)
{
    if (!IterShapes::has(F, D) || n_iters < 0 || n_iters > GNN_ITER_MAX) return 0;
    const IterLayout lay(F, D, n_iters);
    return shared ? lay.shared_floats() : lay.stride();
}

size_t gnn_iter_backward_workspace_bytes(int64_t n_graphs, int32_t F, int32_t D, int32_t n_iters)
{
    if (!IterShapes::has(F, D) || n_iters < 0 || n_iters > GNN_ITER_MAX || n_graphs < 0) {
        fail(GNN_ERR_BADARG, "gnn_iter_backward_workspace_bytes: bad argument");
        return 0;
    }
    return (size_t)(n_graphs > 0 ? n_graphs : 1) * IterLayout(F, D, n_iters).stride() * sizeof(float) + 256;
}

int gnn_iter_backward_events(const gnn_graph_t *g, const gnn_iter_params_t *p, const int32_t *hit_ptr,
                             const int32_t *seg_ptr, int64_t n_graphs, int32_t max_hits, int32_t max_segments,
                             const float *e_all, const float *H_all, const float *grad_out, float *grads_flat,
                             void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "gnn_iter_backward_events";
    if (int rc = check_params(who, p)) return rc;
    if (int rc = check_batch(who, g, hit_ptr, seg_ptr, n_graphs, max_hits, max_segments)) return rc;
    if (!grads_flat) return fail(GNN_ERR_BADARG, "%s: grads_flat missing", who);
    if ((g->n_segments > 0 && (!e_all || !grad_out)) || (g->n_hits > 0 && !H_all))
        return fail(GNN_ERR_BADARG, "%s: the forward's saved tensors or grad_out missing", who);
    if (!gnn_iter_events_supported(p->F, p->D, max_hits, max_segments, 1))
        return fail(GNN_ERR_UNSUPPORTED, "%s: graphs of up to %d hits / %d segments do not fit the one-launch backward at "
                    "input_dim=%d hidden_dim=%d", who, max_hits, max_segments, p->F, p->D);
    if (int rc = check_workspace(workspace, workspace_bytes, gnn_iter_backward_workspace_bytes(n_graphs, p->F, p->D, p->n_iters)))
        return rc;
    return IterShapes::find<int>(p->F, p->D, GNN_ERR_UNSUPPORTED, [&](auto sh) {      // (check_params: the shape is listed)
        return run_iter_backward<sh.F, sh.D>(g, p, hit_ptr, seg_ptr, n_graphs, max_hits, max_segments, e_all, H_all,
                                             grad_out, grads_flat, align_ws(workspace), static_cast<hipStream_t>(stream)); });
}

size_t gnn_iter_input_bwd_workspace_bytes(int64_t n_hits, int32_t F, int32_t D)
{
    if (n_hits < 0 || F < 1 || D < 1) {
        fail(GNN_ERR_BADARG, "gnn_iter_input_bwd_workspace_bytes: bad argument");
        return 0;
    }
    const int64_t chunks = n_hits > 0 ? (n_hits + kInChunk - 1) / kInChunk : 1;
    return (size_t)chunks * (D * F + D) * sizeof(float) + 256;
}

int gnn_iter_input_bwd(const float *X, const float *H0, int32_t ldh, const float *gH0, int32_t ldg, int64_t n_hits,
                       int32_t F, int32_t D, float *grads_flat, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "gnn_iter_input_bwd";
    if (n_hits < 0 || F < 1 || D < 1 || !grads_flat || (n_hits > 0 && (!X || !H0 || !gH0)))
        return fail(GNN_ERR_BADARG, "%s: bad argument", who);
    if (ldh < D || ldg < D) return fail(GNN_ERR_BADARG, "%s: ldh and ldg must be at least hidden_dim", who);
    if (int rc = check_workspace(workspace, workspace_bytes, gnn_iter_input_bwd_workspace_bytes(n_hits, F, D))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *partial = reinterpret_cast<float *>(align_ws(workspace));
    const int64_t chunks = (n_hits + kInChunk - 1) / kInChunk;
    if (chunks > 0)
        GNN_LAUNCH("k_iter_input_bwd", k_iter_input_bwd, (unsigned)chunks, kBlock, s, X, H0, ldh, gH0, ldg, n_hits, F, D,
                   partial);
    IterLayout lay(F, D, 0);        // (its stride is not the row length here: rows of nin floats)
    GNN_LAUNCH("k_iter_fold", k_iter_fold, (unsigned)((lay.nin + kBlock - 1) / kBlock), kBlock, s, partial, chunks,
               (int64_t)lay.nin, grads_flat, lay.nin, lay, 0);
    return 0;
}

}  // extern "C"
