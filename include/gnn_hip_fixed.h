/* gnn_hip_fixed.h - C ABI of the fixed-point forward of SegmentClassifier (third public header of libgnn_hip.so).
 *
 * The reference's stated goal is a segment classifier small enough for an FPGA (gnn/README.md).
 * gnn_segclf_forward of gnn_hip.h runs gnn/model.py:140-156 in float32; the entry point here runs the same dataflow as
 * an HLS design would: two's-complement words of a chosen width, exact integer sums, activations read from tables.
 * Nothing is rounded in an order-dependent way, so the results are defined bit for bit ("Fixed point").
 *
 *   format   W = total_bits, I = int_bits (sign included), Fb = W - I, lo = -2^(W-1), hi = 2^(W-1) - 1; a stored
 *            integer k in [lo, hi] means k * 2^-Fb
 *   requant  of an exact accumulator at scale 2^-2Fb: add 2^(Fb-1) when rounding = GNN_FX_RND and Fb > 0, shift
 *            right by Fb (arithmetic: floor), and where the result leaves [lo, hi] count one overflow of the stage
 *            and clip (GNN_FX_SAT) or keep the low W bits, sign-extended (GNN_FX_WRAP)
 *   lookup   of a stored k: T[clamp(((int64) k << s >> Fb) + 2^(tb-1), 0, 2^tb - 1)], s = tb - 3 for the tanh table
 *            (which spans [-4, 4)) and tb - 4 for the sigmoid table ([-8, 8)), tb = table_bits
 *
 * Every convention of gnn_hip.h holds (caller-allocated device memory, nn.Linear's [out, in] layout, asynchronous work
 * on `stream`, no hidden synchronisation or copy, 0 / negative return values with gnn_last_error(), padded segments
 * src = dst = -1, capturable in a HIP graph).  Hit rows are int32 [H'(D) | x(F) | 0-pad], gnn_h_stride(F, D) apart.
 * GNN_ABI_VERSION of gnn_hip.h covers this header too.
 */
#ifndef GNN_HIP_FIXED_H
#define GNN_HIP_FIXED_H

#include "gnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GNN_FX_TRN  0 /* rounding: truncate (floor)                     */
#define GNN_FX_RND  1 /* rounding: add half an output step, then floor  */
#define GNN_FX_WRAP 0 /* overflow: keep the low W bits                  */
#define GNN_FX_SAT  1 /* overflow: clip to [lo, hi]                     */

#define GNN_FX_STAGES 6 /* columns of `counts`: input z, edge z1, edge z2, aggregate mi / mo, node z3, node z4 */

typedef struct gnn_fx_format {
    int32_t total_bits; /* W, 4 .. 24                     */
    int32_t int_bits;   /* I, 2 .. W, sign included       */
    int32_t rounding;   /* GNN_FX_TRN / GNN_FX_RND        */
    int32_t overflow;   /* GNN_FX_WRAP / GNN_FX_SAT       */
    int32_t table_bits; /* tb, 4 .. 12                    */
} gnn_fx_format_t;

/* The ten effective weight tensors of gnn_params_t (W * mask, gnn/model.py:28-33), quantised by the caller to stored
 * integers of the format: device pointers, shapes of the reference state_dict. */
typedef struct gnn_fx_params {
    const int32_t *Win, *bin; /* input_network.0           [D,F]  [D]   gnn/model.py:132-134 */
    const int32_t *W1, *b1;   /* edge_network.network.0    [D,2C] [D]   gnn/model.py:45-46   */
    const int32_t *W2, *b2;   /* edge_network.network.2    [1,D]  [1]   gnn/model.py:48      */
    const int32_t *W3, *b3;   /* node_network.network.0    [D,3C] [D]   gnn/model.py:94-95   */
    const int32_t *W4, *b4;   /* node_network.network.2    [D,D]  [D]   gnn/model.py:97      */
    int32_t F, D;
} gnn_fx_params_t;

/* The two activation tables, 2^table_bits stored integers each (device pointers): nn.Tanh of gnn/model.py:47,96,98,134
 * sampled on [-4, 4) and nn.Sigmoid of gnn/model.py:49 on [-8, 8).  The kernels evaluate neither function. */
typedef struct gnn_fx_tables {
    const int32_t *tanh_table, *sigmoid_table;
} gnn_fx_tables_t;

/* 1 if gnn_fx_forward has kernels for this (input_dim, hidden_dim) - the shapes of gnn_shape_supported
 * (gnn/model.py:130-138 at any width the reference trains) - and the format is one it runs. */
int gnn_fx_supported(int32_t F, int32_t D, int32_t total_bits, int32_t int_bits, int32_t table_bits);

/* Bytes of workspace gnn_fx_forward needs: two tables of hit rows H (gnn/model.py:146,154), the sums mi | mo of one
 * node pass (gnn/model.py:118-119), the per-hit halves of the edge network's first layer as int64 and one pass's
 * scores (gnn/model.py:150).  0: bad arguments; the message is in gnn_last_error. */
size_t gnn_fx_workspace_bytes(int64_t n_hits, int64_t n_segments, int32_t F, int32_t D);

/* SegmentClassifier.forward (gnn/model.py:140-156) in fixed point.  g->X is float32 and quantised here
 * (clip(rint(X * 2^Fb)), NaN -> 0); all six segment lists of `g` are required.  Per pass t = 0 .. n_iters: the edge
 * network (gnn/model.py:69-81) scores every segment, padded ones included; for t < n_iters the node network
 * (gnn/model.py:113-125) sums e_j * H[other end] over each hit's in and out lists, exactly, requantises the sums and
 * updates the hit (gnn/model.py:149-154).
 * Written: e_raw [n_segments] int32, the stored integers of the last edge pass; e_float [n_segments] = e_raw * 2^-Fb
 * (exact); counts [(n_iters + 1) * GNN_FX_STAGES] int64, the overflows of every stage per pass (zeroed here; row
 * n_iters has the edge columns only); e_trace [(n_iters + 1), n_segments] and H_trace [(n_iters + 1), n_hits, C] int32,
 * every pass's scores and hit rows, or NULL.  An array of no elements may be NULL.
 * The sums are exact as long as every hit's in and out list is shorter than 2^(65 - 2 W) entries: the caller's to
 * check.  GNN_ERR_BADARG names the argument; GNN_ERR_UNSUPPORTED: gnn_fx_supported says no. */
int gnn_fx_forward(const gnn_graph_t *g, const gnn_fx_params_t *p, const gnn_fx_format_t *fmt,
                   const gnn_fx_tables_t *tables, int32_t n_iters, int32_t *e_raw, float *e_float, int64_t *counts,
                   int32_t *e_trace, int32_t *H_trace, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GNN_HIP_FIXED_H */
