// event_passes.h - what the four kernels that run a whole small graph in one workgroup share: k_event (gnn_kernels.hip),
// k_event_bwd (backward.hip), k_iter_event and k_iter_event_bwd (iter_events.hip).  Here: the wavefronts per graph, the
// LDS byte counts the entry points answer with, the backward's weight-block offsets, and the copy of a graph's index
// arrays as local ids.  No function here contains a barrier.
//
// The stages per hit, per segment and per list entry are NOT here: each kernel keeps its own text of them, in the same
// order.  The register allocation of these kernels follows the inlining boundaries - a stage moved, statement for
// statement, into a function changes the resource usage of some instantiation - and only what compiles to the
// parent's resource usage at every shape is shared (profiles/event_passes_ab.txt has what was tried).
#pragma once
#include "common.h"

namespace gnn {

template <int D>
struct EvCfg {
    // wavefronts per graph: the output rows of every layer are dealt to them
    static constexpr int NWV = D >= 32 ? 16 : D >= 8 ? 8 : 4;
    static constexpr int NT = 64 * NWV;
};

// int32 words of a graph's local ids behind the floats: ip, op [cap_h + 1], ie, inb, oe, onb, sl, dl [cap_s]
constexpr int64_t ev_id_words(int64_t cap_h, int64_t cap_s) { return 2 * (cap_h + 1) + 6 * cap_s; }

// The forward's LDS: H, Hn (LDH per hit each), PQ (2 D), qb (D), Mb (2 LDH), es (segments, padded to 4), the family's
// block of `w_floats` weights, the local ids
inline size_t ev_fwd_lds_bytes(int F, int D, int64_t cap_h, int64_t cap_s, int w_floats)
{
    const int ldh = (F + D + 3) & ~3;
    return (size_t)(cap_h * (4 * ldh + 3 * D) + ((cap_s + 3) & ~(int64_t)3) + w_floats + ev_id_words(cap_h, cap_s)) *
           sizeof(float);
}

// The backward's LDS (kBlock threads per graph)
template <int F, int D>
struct EvBwd {
    static constexpr int C = F + D, LDH = (C + 3) & ~3;
    // one weight set in LDS: W1, b1, W2, W3, b3, W4; the rows of W1 / W3 are laid out like the feature rows
    // they multiply (blocks of C columns padded to LDH, zeros) so that products run on 4-float pieces
    static constexpr int oW1 = 0, ob1 = oW1 + D * 2 * LDH, oW2 = ob1 + D, oW3 = oW2 + D,
                         ob3 = oW3 + D * 3 * LDH, oW4 = ob3 + D, w_total = oW4 + D * D;
    static constexpr int per_hit = 9 * LDH + 5 * D;     // Hc Hp gH gHp (4) + gmio (2) + M (3) | PQ fa (2D each) qb
    static size_t lds_bytes(int64_t cap_h, int64_t cap_s)
    {
        const int64_t s4 = (cap_s + 3) & ~(int64_t)3;
        return (size_t)(cap_h * per_hit + 2 * s4 + w_total + ev_id_words(cap_h, cap_s) + 8) * sizeof(float);
    }
};

// where the local ids of the workgroup's graph - hits [h0, h0 + nh), segments [s0, s0 + ns) of the block-diagonal
// batch - go in LDS
struct EvIds {
    int32_t *ip, *op, *ie, *inb, *oe, *onb, *sl, *dl;
};

// The graph's two segment lists as LOCAL ids: the pull loops chase eid -> score and nbr -> feature row per list entry,
// and from global memory every hop is a dependent round trip.  One coalesced pass instead.  (A graph of no hits is not
// to come here: in_ptr[h0] may lie behind the arrays.)
template <int NT>
__device__ __forceinline__ void ev_local_lists(const gnn_graph_t &g, int h0, int nh, int s0, const EvIds &m)
{
    const int ib = g.in_ptr[h0], ob = g.out_ptr[h0];
    for (int n = threadIdx.x; n <= nh; n += NT) {
        m.ip[n] = g.in_ptr[h0 + n] - ib;
        m.op[n] = g.out_ptr[h0 + n] - ob;
    }
    const int ni = g.in_ptr[h0 + nh] - ib, no = g.out_ptr[h0 + nh] - ob;
    for (int k = threadIdx.x; k < ni; k += NT) {
        m.ie[k] = g.in_eid[ib + k] - s0;
        m.inb[k] = g.in_nbr[ib + k] - h0;
    }
    for (int k = threadIdx.x; k < no; k += NT) {
        m.oe[k] = g.out_eid[ob + k] - s0;
        m.onb[k] = g.out_nbr[ob + k] - h0;
    }
}

// src / dst as local ids; a padded segment (src < 0) is -1 at both ends
template <int NT>
__device__ __forceinline__ void ev_local_ends(const gnn_graph_t &g, int h0, int s0, int ns, const EvIds &m)
{
    for (int j = threadIdx.x; j < ns; j += NT) {
        const int sg = g.src[s0 + j];
        m.sl[j] = sg < 0 ? -1 : sg - h0;
        m.dl[j] = sg < 0 ? -1 : g.dst[s0 + j] - h0;
    }
}

}  // namespace gnn
