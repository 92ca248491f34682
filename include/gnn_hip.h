/* gnn_hip.h - C ABI of libgnn_hip.so: the SegmentClassifier message-passing forward
 * of jmduarte/gnn-fpga (gnn/model.py) as hand-written HIP kernels for gfx950 (MI355X).
 *
 * The reference has no native boundary: its "FFI" for this path is the set of ATen calls
 * in gnn/model.py.  Each entry point below names the reference interface it replaces.
 * A maintainer binds it with ctypes; no C++ or torch types cross.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into caller-owned memory (e.g. tensor.data_ptr());
 *     the library never allocates, frees or retains caller buffers;
 *   - workspaces and output buffers need NOT be initialised by the caller: a call clears what it
 *     counts in or adds up, and writes EVERY element of every output it documents - padded
 *     segments' scores, rows of empty graphs or events, list tails and the 0-pad of a hit-feature
 *     row included - unless an exception is listed at the entry point (there is one: the columns
 *     of gnn_gcn_forward's H_all past a layer's own width are unspecified);
 *   - a call writes nothing outside the workspace bytes its *_workspace_bytes function asked for
 *     and the documented extent of its outputs;
 *   - buffers documented as "ADDED into", "ORed into" or "zero them first" (gnn_grads_t, grad_H of
 *     gnn_edge_bwd, the counters of gnn_segment_metrics_update, the lists of
 *     gnn_gcn_compress_fill) are inputs as well: the caller initialises those;
 *     (tests/test_gpu_uninitialised.py runs every entry point on poisoned, guarded buffers)
 *   - Alignment.  An array - input, output, weight, gradient, kept training tensor, table column - must
 *     start at a multiple of its ELEMENT size (4 bytes for float32 / int32, 8 for float64 / int64) and
 *     nothing more: a window of a larger array (X of graphs j .. j1 of a dataset, a gradient or a
 *     parameter inside one flat buffer) is as good as an allocation of its own, at every entry point.
 *     Several kernels move such arrays 16 bytes per lane (hit rows H / H_all / Q_all / grad rows, the
 *     biases b1, b3, b4 at D >= 32); gfx950 serves a 16-byte global load or store at any 4-byte address and
 *     the results are bit-identical wherever the array starts; only gnn_segment_metrics_update picks
 *     between a 16-byte and a 4-byte loop by address.  Rows keep their documented stride (ldh floats).
 *     A workspace needs no alignment of its own: every entry point rounds the pointer up to 256
 *     bytes itself and every *_workspace_bytes value includes that slack (gnn_gcn_backward and
 *     gnn_bce_loss use theirs as floats from the first byte: 4 bytes).  That is read from the code;
 *     the tests move workspaces in steps of 4 bytes.  The one exception are the arrays of gnn_plan_t
 *     / gnn_plan_out_t, which the fused kernels stream in pieces of 16 bytes and more: give each an
 *     allocation of its own (hipMalloc / a torch tensor: 256 bytes and up), as the shipped binding does.
 *     (tests/test_gpu_offset_arrays.py runs every entry point with its arrays - inputs, and the
 *     outputs, kept tensors, gradient buffers and workspaces the shipped binding allocates - 4, 8 and
 *     12 bytes past the 16-byte grid and with a different offset for every array of a call, between
 *     guard bands; the segment lists of gnn_graph_t, the hit_ptr / seg_ptr of the one-launch entry
 *     points and seg_ptr / tw_src / tw_dst of gnn_segclf_forward_train_plan - int32 arrays read one
 *     element at a time - stay where the binding's other modules put them)
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     all work is asynchronous on it, no implicit synchronisation;
 *   - return value 0 = success; negative = -(hipError_t) or one of GNN_ERR_*;
 *     gnn_last_error() returns a thread-local message for the last failing call;
 *   - matrices are row-major float32; weights use torch's nn.Linear layout [out, in];
 *   - F = input_dim, D = hidden_dim, C = D + F; hit-feature rows H[n] = [H'(D) | X(F) | 0-pad]
 *     with row stride ldh = gnn_h_stride(F, D) floats (C rounded up to a multiple of 4);
 *   - a padded segment has src = dst = -1 (the all-zero Ri/Ro column of
 *     gnn/trainSegmentClassifier.py:83-93): it scores sigmoid(W2 tanh(b1) + b2) and
 *     contributes nothing to any hit.
 */
#ifndef GNN_HIP_H
#define GNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNN_ABI_VERSION 7

#define GNN_ERR_UNSUPPORTED (-10001) /* (F, D) has no kernel instantiation            */
#define GNN_ERR_BADARG      (-10002) /* null pointer, negative size, bad stride ...   */
#define GNN_ERR_WORKSPACE   (-10003) /* workspace smaller than gnn_forward_workspace_bytes */

/* Effective weights (mask already applied: W*mask, gnn/model.py:28-33), device pointers.
 * Shapes follow the reference state_dict. */
typedef struct gnn_params {
    const float *Win, *bin; /* input_network.0           [D,F]  [D]   gnn/model.py:132-134 */
    const float *W1, *b1;   /* edge_network.network.0    [D,2C] [D]   gnn/model.py:45-46   */
    const float *W2, *b2;   /* edge_network.network.2    [1,D]  [1]   gnn/model.py:48      */
    const float *W3, *b3;   /* node_network.network.0    [D,3C] [D]   gnn/model.py:94-95   */
    const float *W4, *b4;   /* node_network.network.2    [D,D]  [D]   gnn/model.py:97      */
    int32_t F, D;
    int32_t flags;          /* GNN_FLAG_* (fused pipeline only)                                */
} gnn_params_t;

/* The caller asserts max(|P'|, |Q'|) <= 60 for every hit, with P' = 2 log2(e) (W1[:, :C] H + b1),
 * Q' = 2 log2(e) W1[:, C:] H.  Since |H'| <= 1 (tanh) a sufficient condition is
 *   2 log2(e) * max_i ( sum_{k<D} |W1[i,k]| + sum_{k<F} |W1[i,D+k]| max|X[:,k]| + |b1[i]| ) <= 60
 * (same for the columns C..2C without the bias); gnn_exp_product_bound computes the left side.
 * With the flag set the fused kernels publish 2^P', 2^Q' and form 2^(P'+Q') by multiplication
 * (one transcendental less per hidden unit and segment); without it they use the exact path. */
#define GNN_FLAG_EXP_PRODUCT 1

/* hidden_dim 32 / 64 only (ignored elsewhere): run the hit update (gnn/model.py:120-125, and the
 * per-hit halves of the next edge / node layers) on the matrix cores with bf16 operands and fp32
 * accumulation (v_mfma_f32_16x16x32_bf16).  Weights are rounded to bf16 once per forward,
 * activations per use; the per-hit gather records travel as bf16, everything per segment is
 * computed in fp32.  NOT within the 1e-5 parity bound of the fp32 path: scores move by ~1e-3
 * (tests state the bound). */
#define GNN_FLAG_BF16_MLP 2

/* One block-diagonal batch of hit graphs in index form (replaces the dense Ri/Ro of
 * gnn/graph.py:28-35).  CSR arrays list, per hit, the segments ending (in_*) / starting
 * (out_*) there in ascending segment id, and the hit at the other end of each. */
typedef struct gnn_graph {
    const float *X;                            /* [n_hits, F]                              */
    const int32_t *src, *dst;                  /* [n_segments]  start / end hit, -1 = pad  */
    const int32_t *in_ptr, *in_eid, *in_nbr;   /* [n_hits+1], [n_valid], [n_valid] (=src[in_eid])  */
    const int32_t *out_ptr, *out_eid, *out_nbr;/* [n_hits+1], [n_valid], [n_valid] (=dst[out_eid]) */
    int64_t n_hits, n_segments;
} gnn_graph_t;

/* Gradient outputs, same shapes as gnn_params_t; the caller zero-initialises them and the
 * backward ADDS into them (device pointers). */
typedef struct gnn_grads {
    float *Win, *bin, *W1, *b1, *W2, *b2, *W3, *b3, *W4, *b4;
} gnn_grads_t;

/* Execution plan of the fused pipeline (built once per batch by the host; see
 * gnn-fpga_amd/plan.py).  Hits are renumbered by (graph, topological level), cut into tiles of
 * <= tile_hits hits (one workgroup each), degree-sorted inside a tile and padded to 16-hit
 * slices; n_pad = padded hit count, NULL hit id = n_pad.  Neighbour lists are SELL-16: entry k
 * of hit i of slice s at off[s] + 16*k + i, padded with the NULL entry.  A tile / chunk whose
 * neighbour id windows fit the LDS budget (gnn_plan_limits) runs in LDS mode (mode = 1): its
 * list / endpoint entries are window-relative and NULL = window size; otherwise entries are
 * absolute padded ids.  Scores stay per segment in the caller's segment order.
 *   tile  descriptor, 8 ints: slice_begin, slice_end, in_lo, in_cnt, out_lo, out_cnt, mode, sched_base
 *   chunk descriptor, 8 ints: seg_begin, seg_end, src_lo, src_cnt, dst_lo, dst_cnt, mode, 0 */
typedef struct gnn_plan {
    const float *X;                      /* [n_pad+1+64, F] renumbered features; dummy, NULL and the 64
                                            tail rows (window DMA overrun) are zero */
    const int32_t *src, *dst;            /* [n_segments] endpoints (window-relative or absolute)   */
    const int32_t *in_off, *in_nbr;      /* [n_pad/16+1], [in_off[last]]  segments ending at a hit -> start hit */
    const int32_t *out_off, *out_nbr;    /* [n_pad/16+1], [out_off[last]] segments starting at a hit -> end hit */
    const int32_t *tiles, *chunks;       /* [n_tiles*8], [n_chunks*8] descriptors                  */
    /* 16-bit packed copy of the lists (window-relative entries, steps padded to 8 per slice,
     * word p of hit i of slice s = steps 2p | 2p+1 << 16 at off16[s] + 16*p + i) */
    const int32_t *in_off16, *in_nbr16, *out_off16, *out_nbr16;
    /* per-phase wave schedules of the phase-split kernel: sched[tile[7] + 16*round + wave] = slice
     * id (or -1) that wavefront `wave` of the tile's workgroup takes in `round` */
    const int32_t *sched_a, *sched_b;
    const int32_t *sd16;                 /* [n_segments] LDS-mode chunks: dst_rel << 16 | src_rel   */
    int64_t n_pad, n_segments, n_tiles, n_chunks;
    int64_t iter_lds_records;            /* max over LDS-mode tiles of in_cnt + out_cnt + 2        */
    int64_t edge_lds_rows;               /* max over LDS-mode chunks of src_cnt + dst_cnt + 2      */
    int64_t n_lds_tiles;                 /* number of tiles with mode = 1                          */
    int64_t iter_lds_in, iter_lds_out;   /* max in_cnt / out_cnt over LDS-mode tiles               */
    int64_t tile_hits_max;               /* largest tile, in (padded) hits                         */
    int64_t max_list_steps;              /* longest SELL list of any slice, in steps               */
} gnn_plan_t;

int gnn_abi_version(void);
const char *gnn_last_error(void);

/* 1 if kernels exist for this (input_dim, hidden_dim), else 0. */
int gnn_shape_supported(int32_t F, int32_t D);
/* Row stride (floats) of H for this shape; 0 if unsupported. */
int32_t gnn_h_stride(int32_t F, int32_t D);

/* input_network + skip concat: H[n] = [tanh(Win X[n] + bin) | X[n]].
 * Replaces gnn/model.py:144,146 (nn.Linear + Tanh + torch.cat). */
int gnn_input_fwd(const float *X, const float *Win, const float *bin, float *H,
                  int64_t n_hits, int32_t F, int32_t D, int32_t ldh, void *stream);

/* EdgeNetwork.forward: e[j] = sigmoid(W2 tanh(W1 [H[src j] | H[dst j]] + b1) + b2).
 * Replaces gnn/model.py:69-81 (two bmm gathers, cat, MaskedLinear, Tanh, MaskedLinear, Sigmoid).
 * pq_ws: scratch of n_hits * 2 * D floats (per-hit halves of the first layer). */
int gnn_edge_fwd(const float *H, int32_t ldh, const int32_t *src, const int32_t *dst,
                 const float *W1, const float *b1, const float *W2, const float *b2,
                 float *e, float *pq_ws, int64_t n_hits, int64_t n_segments,
                 int32_t F, int32_t D, void *stream);

/* NodeNetwork.forward + the following skip concat:
 *   mi[n] = sum_{j: dst j = n} e[j] H[src j],  mo[n] = sum_{j: src j = n} e[j] H[dst j],
 *   Hnext[n] = [tanh(W4 tanh(W3 [mi|mo|H[n]] + b3) + b4) | X[n]]   (X[n] = H[n][D:D+F]).
 * Replaces gnn/model.py:113-125 (four bmm, two broadcast multiplies, cat, 2x MaskedLinear+Tanh)
 * and :154.  Sums run in ascending segment id (fixed order: bit-reproducible).
 * Only X, in_*, out_* and n_hits of `g` are read.  Hnext must not alias H.  Of every row of Hnext the first
 * gnn_h_stride(F, D) floats are written (the 0-pad is H's); floats past them, where ldh is larger, are not touched. */
int gnn_node_fwd(const float *H, int32_t ldh, const float *e, const gnn_graph_t *g,
                 const float *W3, const float *b3, const float *W4, const float *b4,
                 float *Hnext, int32_t F, int32_t D, void *stream);

/* Bytes of device scratch gnn_segclf_forward needs for this problem. */
size_t gnn_forward_workspace_bytes(int64_t n_hits, int64_t n_segments, int32_t F, int32_t D);

/* SegmentClassifier.forward (gnn/model.py:140-156): input network, n_iters x (edge pass,
 * node pass), final edge pass.  e_out [n_segments] receives the scores.
 * Optional traces for parity tests (NULL to skip): e_trace [(n_iters+1), n_segments],
 * H_trace [(n_iters+1), n_hits, C] (unpadded rows). */
int gnn_segclf_forward(const gnn_graph_t *g, const gnn_params_t *p, int32_t n_iters,
                       float *e_out, float *e_trace, float *H_trace,
                       void *workspace, size_t workspace_bytes, void *stream);

/* Small events (the reference's muon graphs, gnn/prepareMuonGraphs.py: tens of hits): the same
 * forward in ONE launch, one workgroup per graph of the block-diagonal batch, hit features and
 * scores resident in LDS across all iterations (no workspace).  hit_ptr / seg_ptr [n_graphs+1]
 * are device arrays of the graphs' first hit / segment; every segment in
 * [seg_ptr[i], seg_ptr[i+1]) must join hits in [hit_ptr[i], hit_ptr[i+1]) (or be padded,
 * src = dst = -1); max_hits / max_segments bound the graph sizes.  Bit-identical to
 * gnn_segclf_forward.  gnn_events_supported: 1 if graphs of that size fit one workgroup.
 * A never-seen event needs nothing prepared (gnn/Inference.ipynb cell 3: one graph in, scores out): with
 * all six list pointers of `g` NULL the kernel builds the lists itself, in LDS, from (src, dst) - the lists
 * gnn_csr_build makes, so the scores are the same bits -, and with n_graphs == 1 hit_ptr / seg_ptr may be
 * NULL (the graph is [0, n_hits) x [0, n_segments)).  (gnn_segclf_forward only; the training entry points
 * below take caller-built lists and offsets.) */
int gnn_events_supported(int32_t F, int32_t D, int64_t max_hits, int64_t max_segments);
int gnn_segclf_forward_events(const gnn_graph_t *g, const gnn_params_t *p, const int32_t *hit_ptr,
                              const int32_t *seg_ptr, int64_t n_graphs, int32_t max_hits,
                              int32_t max_segments, int32_t n_iters, float *e_out, void *stream);

/* Training forward: like gnn_segclf_forward but keeps what the backward needs - the scores of
 * every edge pass e_all [(n_iters+1), n_segments] (the last row is the model output), the hit
 * features of every iteration H_all [(n_iters+1), n_hits, ldh] (padded rows) and, optionally, the
 * hidden layer of every node pass Q_all [n_iters, n_hits, hidden_dim] (NULL: not kept; the backward
 * then rebuilds it with a second walk over both segment lists). */
int gnn_segclf_forward_train(const gnn_graph_t *g, const gnn_params_t *p, int32_t n_iters,
                             float *e_all, float *H_all, float *Q_all, void *workspace,
                             size_t workspace_bytes, void *stream);

/* The same for a batch of small graphs in one launch (gnn_segclf_forward_events that also keeps
 * e_all / H_all; bit-identical to gnn_segclf_forward_train). */
int gnn_segclf_forward_train_events(const gnn_graph_t *g, const gnn_params_t *p, const int32_t *hit_ptr,
                                    const int32_t *seg_ptr, int64_t n_graphs, int32_t max_hits,
                                    int32_t max_segments, int32_t n_iters, float *e_all, float *H_all,
                                    void *stream);

/* Gradient of a scalar loss w.r.t. the ten parameter tensors, given grad_out [n_segments] =
 * dLoss/d(scores) and the tensors saved by gnn_segclf_forward_train.  Replaces autograd through
 * gnn/model.py:140-156 as triggered by loss.backward() in gnn/estimator.py:58.  Adds into
 * `grads` (zero them first).  Workspace size from gnn_backward_workspace_bytes. */
size_t gnn_backward_workspace_bytes(int64_t n_hits, int64_t n_segments, int32_t F, int32_t D);

/* The reference's loss, nn.BCELoss()(scores, targets) (gnn/trainSegmentClassifier.py:164,
 * gnn/estimator.py:57), value and gradient in one pass over the scores:
 *   loss_out[0] = scale * sum_j -( y_j max(log e_j, -100) + (1 - y_j) max(log(1 - e_j), -100) )
 *   grad_e[j]   = scale * (e_j - y_j) / max(e_j (1 - e_j), 1e-12)        (NULL to skip)
 * scale = 1/n for the reference's "mean" reduction (n counts padded segments too, like the
 * reference's mean over B x E_max), 1 for "sum".  Same clamps as torch; deterministic (fixed
 * summation order).  workspace: GNN_BCE_WORKSPACE_BYTES of device scratch. */
#define GNN_BCE_WORKSPACE_BYTES 4096
int gnn_bce_loss(const float *e, const float *y, int64_t n, float scale, float *loss_out,
                 float *grad_e, void *workspace, void *stream);
int gnn_segclf_backward(const gnn_graph_t *g, const gnn_params_t *p, int32_t n_iters,
                        const float *e_all, const float *H_all, const float *Q_all /* or NULL */,
                        const float *grad_out, const gnn_grads_t *grads, void *workspace,
                        size_t workspace_bytes, void *stream);

/* NodeClassifier (gnn/MPNN_HitClassifier.ipynb cells 20-21, the reference's hit classifier): the trunk of
 * gnn_segclf_forward - input network, n_iters x (edge pass, node pass) - then the output network
 *   y[n] = sigmoid(Wo [H'_T[n] | X[n]] + bo),   Wo [1, C] (H' columns first, then X), bo [1]
 * in place of the final edge pass (the last node pass's kernel scores its hits; with n_iters = 0 the
 * input network's does).  Wo, bo, gWo, gbo are separate device pointers: gnn_params_t / gnn_grads_t
 * are the trunk's ten tensors.  Workspace: gnn_forward_workspace_bytes for both forwards,
 * gnn_backward_workspace_bytes for the backward.
 * gnn_nodeclf_forward replaces NodeClassifier.forward (cell 21): y_out [n_hits]; H_trace (NULL to
 * skip) [(n_iters+1), n_hits, C] as in gnn_segclf_forward. */
int gnn_nodeclf_forward(const gnn_graph_t *g, const gnn_params_t *p, const float *Wo, const float *bo,
                        int32_t n_iters, float *y_out, float *H_trace, void *workspace,
                        size_t workspace_bytes, void *stream);
/* Training forward of cell 21 (as run by gnn/estimator.py's training_step, cell 30): like
 * gnn_segclf_forward_train, with the n_iters trunk edge passes in e_all [n_iters, n_segments],
 * H_all [(n_iters+1), n_hits, ldh], Q_all [n_iters, n_hits, hidden_dim] (or NULL), y_out [n_hits]. */
int gnn_nodeclf_forward_train(const gnn_graph_t *g, const gnn_params_t *p, const float *Wo, const float *bo,
                              int32_t n_iters, float *e_all, float *H_all, float *Q_all, float *y_out,
                              void *workspace, size_t workspace_bytes, void *stream);
/* Backward of cell 21 for loss.backward() in gnn/estimator.py (cell 30): given grad_y [n_hits] =
 * dLoss/dy and the tensors saved by gnn_nodeclf_forward_train (y = its y_out), ADDS the gradients of
 * the ten trunk tensors into `grads` and of the output network into gWo [C], gbo [1] (zero them first).
 * dz = grad_y y (1 - y) seeds gH_T = dz Wo[:D]; every sum runs in a fixed order (bit-reproducible). */
int gnn_nodeclf_backward(const gnn_graph_t *g, const gnn_params_t *p, const float *Wo, const float *bo,
                         int32_t n_iters, const float *e_all, const float *H_all, const float *Q_all /* or NULL */,
                         const float *y, const float *grad_y, const gnn_grads_t *grads, float *gWo, float *gbo,
                         void *workspace, size_t workspace_bytes, void *stream);

/* The same gradients for a batch of SMALL graphs (gnn/prepareMuonGraphs.py sizes) in ONE launch:
 * one workgroup per graph keeps the graph's saved rows and every intermediate in LDS (counterpart
 * of gnn_segclf_forward_events; same layout contract for hit_ptr / seg_ptr).  Workspace:
 * gnn_backward_events_workspace_bytes.  gnn_events_backward_supported: 1 if graphs of that size
 * fit one workgroup for this (input_dim, hidden_dim). */
int gnn_events_backward_supported(int32_t F, int32_t D, int64_t max_hits, int64_t max_segments);
size_t gnn_backward_events_workspace_bytes(int64_t n_graphs, int32_t F, int32_t D);
int gnn_segclf_backward_events(const gnn_graph_t *g, const gnn_params_t *p, const int32_t *hit_ptr,
                               const int32_t *seg_ptr, int64_t n_graphs, int32_t max_hits,
                               int32_t max_segments, int32_t n_iters, const float *e_all,
                               const float *H_all, const float *grad_out, const gnn_grads_t *grads,
                               void *workspace, size_t workspace_bytes, void *stream);

/* SegmentClassifier.forward (gnn/model.py:140-156) on a planned batch: the fast path.
 * One fused kernel per message-passing iteration (edge scores are recomputed at both
 * endpoints from per-hit partial products instead of being stored), one final edge kernel.
 * e_out [n_segments].  Workspace size from gnn_plan_workspace_bytes. */
size_t gnn_plan_workspace_bytes(int64_t n_pad, int64_t n_segments, int32_t F, int32_t D);
int gnn_segclf_forward_plan(const gnn_plan_t *plan, const gnn_params_t *p, int32_t n_iters,
                            float *e_out, void *workspace, size_t workspace_bytes, void *stream);
/* The TRAINING forward on a planned batch (ABI 4): the same tile kernels, keeping what the backward
 * (gnn_segclf_backward) needs - what gnn_segclf_forward_train keeps with the per-module kernels
 * (autograd for gnn/estimator.py:53,57-58).  The backward's batch must be the plan-space form of the
 * planned batch: hits numbered by the plan's padded ids (n_pad hits, dummies without segments),
 * segments sorted by end hit (stable), `seg_ptr` [n_pad + 1] = its CSR pointer over end hits
 * (in_ptr).  Written: e_all rows 0 .. n_iters-1 ([n_iters + 1, n_segments]; the scores of every pass
 * in THAT segment order, valid segments only - padded ones are never read by the backward's list
 * walks), H_all [(n_iters + 1), n_pad, ldh] (ldh = gnn_h_stride), Q_all [n_iters, n_pad, D] and the
 * final scores e_out [n_segments] in the PLAN's segment order (the caller's; NULL: not wanted).  Row
 * n_iters of e_all - the final scores in the backward's order - is written when tw_src / tw_dst
 * [n_segments] are given: that batch's segment endpoints as plan hit ids, -1 = padded (same bits as
 * e_out for the same segment); with NULL the row is the caller's to fill (a gather of e_out).  Shapes
 * on the general tile kernel only (hidden_dim <= 16 without the 16-lanes-per-hit route):
 * GNN_ERR_UNSUPPORTED otherwise.  Workspace as gnn_segclf_forward_plan. */
int gnn_segclf_forward_train_plan(const gnn_plan_t *plan, const gnn_params_t *p, int32_t n_iters,
                                  const int32_t *seg_ptr, const int32_t *tw_src, const int32_t *tw_dst,
                                  float *e_all, float *H_all, float *Q_all, float *e_out /* or NULL */,
                                  void *workspace, size_t workspace_bytes, void *stream);
/* 1 if the fused pipeline has kernels for this (input_dim, hidden_dim). */
int gnn_plan_shape_supported(int32_t F, int32_t D);
/* Plan-building limits for a shape: out4 = { tile_hits, iter_records, chunk_segments,
 * edge_records } - the tile / chunk sizes and the LDS window budgets (in records of 2D floats
 * for the iteration kernel, rows of D floats for the edge kernel). */
int gnn_plan_limits(int32_t F, int32_t D, int32_t *out4);
/* Which kernels gnn_segclf_forward_plan (training = 0) or gnn_segclf_forward_train_plan (training = 1) launches
 * for this plan, these flags and n_iters, decided by the very function the forward calls (choose_route in
 * csrc/sell_pipeline.hip).  Reads the plan's scalars, which of its pointers are NULL, p->F, p->D, p->flags and
 * the GNN_NO_ITER2 / GNN_NO_FUSE_FIRST / GNN_NO_WIDE_EXACT / GNN_WIDE_LOCKSTEP / GNN_WIDE_ROLES switches of the
 * environment; dereferences no device pointer and needs no GPU.  out [GNN_ROUTE_FIELDS]:
 *   GNN_ROUTE_REC         record form: 0 fp32 (general kernels), 1 bf16 rows (after k_pack16), 2 exact fp32 rows of
 *                         the 16-lanes-per-hit kernels (after k_pack32)
 *   GNN_ROUTE_INPUT       input stage: 0 none (no hits, or fused into the first k_iter2), 1 k_input4,
 *                         2 k_input4_bf, 3 k_input4_x
 *   GNN_ROUTE_FAMILY      the kernel of each of the n_iters iterations: 0 k_iter, 1 k_iter2, 2 k_iter_w, 3 k_iter_wx
 *   GNN_ROUTE_FUSE_FIRST  1: the first k_iter2 launch runs the input network too
 *   GNN_ROUTE_EDGE        final edge pass (n_segments > 0): 0 k_edge, 1 k_edge_w
 *   GNN_ROUTE_PACK        1: k_pack runs first
 *   GNN_ROUTE_ITER_LDS, GNN_ROUTE_ITER2_LDS, GNN_ROUTE_EDGE_LDS   dynamic LDS bytes of k_iter, k_iter2 (0: the
 *                         shape has none) and k_edge; GNN_ROUTE_CAP_A / _B: k_iter2's window buffers in records
 *   GNN_ROUTE_WIDE_WINDOW records per group of k_iter_w / k_iter_wx (0: another family)
 * (sizes beyond INT32_MAX are reported as INT32_MAX).  GNN_ERR_UNSUPPORTED: no fused kernels for (F, D), or
 * training = 1 for a shape without a fused training forward. */
enum {
    GNN_ROUTE_REC, GNN_ROUTE_INPUT, GNN_ROUTE_FAMILY, GNN_ROUTE_FUSE_FIRST, GNN_ROUTE_EDGE, GNN_ROUTE_PACK,
    GNN_ROUTE_ITER_LDS, GNN_ROUTE_ITER2_LDS, GNN_ROUTE_CAP_A, GNN_ROUTE_CAP_B, GNN_ROUTE_EDGE_LDS,
    GNN_ROUTE_WIDE_WINDOW, GNN_ROUTE_FIELDS
};
enum { GNN_REC_FP32, GNN_REC_BF16, GNN_REC_EXACT };
enum { GNN_INPUT_NONE, GNN_INPUT_K_INPUT4, GNN_INPUT_K_INPUT4_BF, GNN_INPUT_K_INPUT4_X };
enum { GNN_FAMILY_K_ITER, GNN_FAMILY_K_ITER2, GNN_FAMILY_K_ITER_W, GNN_FAMILY_K_ITER_WX };
enum { GNN_EDGE_K_EDGE, GNN_EDGE_K_EDGE_W };
int gnn_plan_route(const gnn_plan_t *plan, const gnn_params_t *p, int32_t n_iters, int32_t training, int32_t *out);

/* The reference's dense input contract -> index form, on the device: Ri, Ro [B, N, E] float32 with one
 * non-zero per real column and all-zero padded columns (gnn/graph.py:28-35,
 * gnn/trainSegmentClassifier.py:66-95) -> src, dst [B*E] int32 global hit ids b*N + n, -1 for a padded
 * column.  flags [1] (device): bit 0 = a column with more than one non-zero, bit 1 = a column set in
 * only one of Ri / Ro (such columns come out as -1).  Asynchronous on `stream`. */
int gnn_dense_to_index(const float *Ri, const float *Ro, int64_t B, int64_t N, int64_t E, int32_t *src,
                       int32_t *dst, int32_t *flags, void *stream);

/* ---- per-module backward ------------------------------------------------------------------------
 * The reference's sub-modules are ordinary autograd modules (model.edge_network(H, Ri, Ro),
 * model.node_network(H, e, Ri, Ro): gnn/model.py:69-81, 113-125; called on their own in
 * gnn/MPNN_Seg_ACTS_maskedlinear.ipynb cells 42, 46).  These two entry points are their backward:
 * H rows of ldh = gnn_h_stride(F, D) floats, gradient tensors as in gnn_segclf_backward (all ten
 * pointers valid, the backward ADDS into them; an edge backward touches W1, b1, W2, b2 only, a node
 * backward W3, b3, W4, b4 only).  Workspace: gnn_backward_workspace_bytes.
 *   gnn_edge_bwd: grad_e [n_segments] -> grad_H [n_hits, ldh] (caller-zeroed, ADDED into)
 *   gnn_node_bwd: Hnext = the forward's output [n_hits, ldh], grad_Hnext [n_hits, ldh] (first D
 *                 columns used) -> grad_H [n_hits, ldh] (written), grad_e [n_segments] (written) */
int gnn_edge_bwd(const float *H, int32_t ldh, const gnn_graph_t *g, const gnn_params_t *p, const float *e,
                 const float *grad_e, float *grad_H, const gnn_grads_t *grads, void *workspace,
                 size_t workspace_bytes, void *stream);
int gnn_node_bwd(const float *H, int32_t ldh, const float *e, const float *Hnext, const gnn_graph_t *g,
                 const gnn_params_t *p, const float *grad_Hnext, float *grad_H, float *grad_e,
                 const gnn_grads_t *grads, void *workspace, size_t workspace_bytes, void *stream);

/* ---- the plan, built on the GPU (csrc/plan_build.hip) -------------------------------------------
 * Index-form counterpart of the reference's per-batch host work (graph_from_sparse densifies,
 * merge_graphs zero-pads: gnn/graph.py:28-35, gnn/trainSegmentClassifier.py:66-111): the same
 * plan gnn-fpga_amd/plan.py specifies in numpy, array for array, in two calls around ONE host
 * read-back of the sizes:
 *   gnn_plan_build_sizes  levels, tiles, renumbering, sorted neighbour lists, windows, chunks ->
 *                         *sizes_out (DEVICE memory, written asynchronously on `stream`)
 *   gnn_plan_build_fill   fills the arrays the caller allocated from those sizes (a HOST copy of
 *                         the sizes is passed back in)
 * src / dst [n_segments] int32 (-1 = padded), hit_ptr [n_graphs+1] int64 on the DEVICE (graph
 * boundaries, non-decreasing); tile_hits / iter_records / chunk_segments / edge_records as
 * gnn_plan_limits gives them (after the caller's small-batch adjustments, plan.py).  sizes.status
 * != 0: this batch is outside the builder's static bounds (degree >= 65536, > n/16 + 1024 tiles,
 * ...) - build the plan with plan.py / plan_device.py instead; bit 64 of status: a segment end
 * outside [0, n_hits) or a segment with exactly one negative end (malformed batch: the kernels
 * skip such segments, the caller must raise).  n_hits, n_segments > 0.
 * The bits of sizes.status: */
#define GNN_PLAN_ST_DEGREE    1   /* a hit with >= 65536 segments in one direction                    */
#define GNN_PLAN_ST_TILES     2   /* more than n_hits / 16 + 1024 tiles                               */
#define GNN_PLAN_ST_PAD       4   /* more padded hits than the workspace holds                        */
#define GNN_PLAN_ST_CHUNKS    8   /* more marks or chunks than the workspace holds                    */
#define GNN_PLAN_ST_SLICES    16  /* (kept for the slice bound; no kernel sets it today)              */
#define GNN_PLAN_ST_I32       32  /* (kept for the int32 list bound; the caller checks the totals)    */
#define GNN_PLAN_ST_ENDPOINT  64  /* malformed endpoints (above): the caller must raise              */
#define GNN_PLAN_ST_FAST_MISS 128 /* gnn_plan_build_sizes_graphs: call gnn_plan_build_sizes instead   */
typedef struct gnn_plan_sizes {
    int64_t n_pad, n_tiles, n_slices, n_chunks;
    int64_t in_total, out_total;        /* entries of in_nbr / out_nbr before their 64 zero entries */
    int64_t in16_words, out16_words;    /* words of in_nbr16 / out_nbr16 before their 64 zero words */
    int64_t n_sched;                    /* entries of sched_a, sched_b                              */
    int64_t iter_lds_records, edge_lds_rows, n_lds_tiles, n_lds_chunks, iter_lds_in, iter_lds_out;
    int64_t tile_hits_max, max_list_steps, n_valid, max_level, status;
    int64_t list_mode;                  /* ABI 5, graph-local form: 1 = neighbour lists built per tile in LDS, 0 = by scattered
                                           pairs and a sort per list (segments of a tile's lists not contiguous, hub hits) */
} gnn_plan_sizes_t;

typedef struct gnn_plan_out {           /* device arrays gnn_plan_build_fill writes (sizes: gnn_plan_t) */
    float *X;                           /* [(n_pad + 1 + 64) * F]                                     */
    float *x_absmax;                    /* [F] per-feature max |X| (gnn_exp_product_bound)            */
    int32_t *src, *dst, *sd16;          /* [n_segments]                                               */
    int32_t *in_off, *in_nbr;           /* [n_slices + 1], [in_total + 64]                            */
    int32_t *out_off, *out_nbr;         /* [n_slices + 1], [out_total + 64]                           */
    int32_t *in_off16, *in_nbr16;       /* [n_slices + 1], [in16_words + 64]                          */
    int32_t *out_off16, *out_nbr16;     /* [n_slices + 1], [out16_words + 64]                         */
    int32_t *tiles, *chunks;            /* [8 n_tiles], [8 n_chunks]                                  */
    int32_t *sched_a, *sched_b;         /* [n_sched]                                                  */
    int32_t *perm;                      /* [n_pad] new id -> caller's hit id, -1 = padding            */
    int32_t *src_abs, *dst_abs, *level; /* optional (NULL): renumbered endpoints [n_segments], levels [n_hits] */
} gnn_plan_out_t;

size_t gnn_plan_build_workspace_bytes(int64_t n_hits, int64_t n_segments, int32_t chunk_segments);
int gnn_plan_build_sizes(const int32_t *src, const int32_t *dst, const int64_t *hit_ptr, int64_t n_hits,
                         int64_t n_segments, int64_t n_graphs, int32_t tile_hits, int32_t iter_records,
                         int32_t chunk_segments, int32_t edge_records, void *workspace,
                         size_t workspace_bytes, gnn_plan_sizes_t *sizes_out, void *stream);
/* ABI 5: the same stage 1 for a batch whose graphs are laid out one after the other, as merge_graphs' block-diagonal
 * batches are (gnn/trainSegmentClassifier.py:66-95): seg_ptr [n_graphs+1] int64 on the DEVICE, graph g owns segments
 * [seg_ptr[g], seg_ptr[g+1]) and they join hits of [hit_ptr[g], hit_ptr[g+1]) only; max_graph_hits /
 * max_graph_segments = the largest graph (host values).  Degrees, levels, renumbered endpoints and both neighbour
 * lists are then built by one workgroup per graph in LDS instead of device-wide sweeps and sorts (same arrays, entry
 * for entry).  The kernels CHECK the layout they were told: status bit 128 = it does not hold for this batch (an end
 * outside its graph's hit range, ranges that do not tile [0, n_hits) / [0, n_segments), a level above 64, a hit with
 * more than 1024 segments in one direction, a graph of more than 16384 hits whose level / degree / id bits exceed a 32-bit sort key) - call gnn_plan_build_sizes instead.  max_graph_hits > 19456:
 * GNN_ERR_UNSUPPORTED. */
#define GNN_PLAN_GRAPH_CAP_HITS 19456   /* the largest graph of the graph-local form: its tables live in 152 KB of LDS */
int gnn_plan_build_sizes_graphs(const int32_t *src, const int32_t *dst, const int64_t *hit_ptr, const int64_t *seg_ptr,
                                int64_t max_graph_hits, int64_t max_graph_segments, int64_t n_hits,
                                int64_t n_segments, int64_t n_graphs, int32_t tile_hits, int32_t iter_records,
                                int32_t chunk_segments, int32_t edge_records, void *workspace,
                                size_t workspace_bytes, gnn_plan_sizes_t *sizes_out, void *stream);
int gnn_plan_build_fill(const float *X, int32_t F, const int32_t *src, const int32_t *dst, int64_t n_hits,
                        int64_t n_segments, int32_t chunk_segments, const gnn_plan_sizes_t *sizes,
                        void *workspace, size_t workspace_bytes, const gnn_plan_out_t *out, void *stream);

/* ---- the two segment lists, built on the GPU (csrc/csr_build.hip; ABI 4) --------------------------
 * What gnn_graph_t's in_ptr / in_eid / in_nbr and out_ptr / out_eid / out_nbr hold, from the index form: for every
 * hit the ids of the segments that end (start) there, ASCENDING - the reference's on-disk order, `Ri.nonzero()` /
 * `Ro.nonzero()` row-major (gnn/graph.py:20-26), and the order its bmm against Ri / Ro sums in
 * (gnn/model.py:114-119).  Replaces two stable sorts and a read-back per never-seen batch.
 * src / dst [n_segments] int32 (-1 / -1 = padded segment, left out of both lists).  Written: in_ptr, out_ptr
 * [n_hits + 1]; in_eid, in_nbr, out_eid, out_nbr [n_segments] - the first in_ptr[n_hits] (= out_ptr[n_hits]) entries
 * are the lists, the rest is -1; status [1] (device): bit 0 = a segment with an end outside [0, n_hits) or with
 * exactly one negative end (skipped like a padded one; the caller must raise).  The arrays are the same in every
 * run (no dependence on the order atomics arrive in).  Asynchronous on `stream`; no host synchronisation. */
size_t gnn_csr_build_workspace_bytes(int64_t n_hits, int64_t n_segments);
int gnn_csr_build(const int32_t *src, const int32_t *dst, int64_t n_hits, int64_t n_segments, int32_t *in_ptr,
                  int32_t *in_eid, int32_t *in_nbr, int32_t *out_ptr, int32_t *out_eid, int32_t *out_nbr,
                  int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/* ---- segment graphs from detector hits, built on the GPU (csrc/graph_build.hip; ABI 6) ----------------------------
 * Replaces the reference's per-event host graph construction: split_phi_sectors (gnn/prepareGraphs.py:87-106) and one
 * construct_graph per sector (gnn/graph.py:37-142, with construct_segments / select_segments :43-93), as
 * process_event calls them (gnn/prepareGraphs.py:136-170).  gnn-fpga_amd/graph_build.py is the numpy specification;
 * the segments selected are the reference's, bit for bit, for float32 hit columns.  Two calls around ONE host
 * read-back, as the plan builder's:
 *   gnn_graph_build_sizes  sectors, (graph, layer) grouping in frame order, kept-pair counts -> *sizes_out, hit_ptr,
 *                          seg_ptr (DEVICE memory, written asynchronously on `stream`)
 *   gnn_graph_build_fill   X, src, dst, y, hit_index into arrays the caller allocated from a HOST copy of the sizes
 *                          (the same workspace, not touched in between)
 * Inputs (DEVICE): r, phi, z float32 [n_hits], layer int32 [n_hits], event_ptr int64 [n_events + 1] (event e owns
 * rows [event_ptr[e], event_ptr[e+1])), particle_id int64 [n_hits] or NULL (then y is not written).  layer_pairs
 * is a HOST array [n_pairs][2] of (l1, l2) in [0, n_layers), at most 128 pairs.  Graph g = event * n_phi_sectors +
 * sector: its hits in frame order, rows hit_ptr[g] .. hit_ptr[g+1] of X [n_hits_out, 3] (r, centred phi, z, each
 * float32(float64(v) / scale)) and of hit_index (input row, int64); its segments seg_ptr[g] .. seg_ptr[g+1] of src
 * (start hit), dst (end hit) int32 in batch numbering and y = (particle_id[start] == particle_id[end]), ordered
 * pair by pair, then by start hit, then by end hit in frame order.  A pair is kept when |phi_slope| <
 * (l1 < 5 ? phi_slope_max : phi_slope_outer_max) and |z0| < z0_max (float32 thresholds).  sizes.status (0 = fine):
 * bit 1 a layer outside [0, n_layers), bit 2 more than 2^31 - 1 segments, bit 4 event_ptr not non-decreasing from 0
 * to n_hits; gnn_graph_build_fill refuses flagged sizes.  GNN_ERR_BADARG: null or negative arguments, a layer_pairs
 * entry out of range, n_phi_sectors < 1; GNN_ERR_UNSUPPORTED: > 128 pairs or sizes beyond int32 indices.  The
 * output is the same in every run (no order decided by atomics). */
typedef struct gnn_graph_build_sizes {
    int64_t n_graphs, n_hits, n_segments;       /* graphs = n_events * n_phi_sectors; hits kept (in a sector)      */
    int64_t n_rows, n_tasks;                    /* (start hit, pair) rows and workgroup tasks of the pair kernels   */
    int64_t max_graph_hits, max_graph_segments, status;
} gnn_graph_build_sizes_t;

size_t gnn_graph_build_workspace_bytes(int64_t n_hits, int64_t n_events, const int32_t *layer_pairs, int32_t n_pairs,
                                       int32_t n_layers, int32_t n_phi_sectors);
int gnn_graph_build_sizes(const float *r, const float *phi, const float *z, const int32_t *layer, int64_t n_hits,
                          const int64_t *event_ptr, int64_t n_events, const int32_t *layer_pairs, int32_t n_pairs,
                          int32_t n_layers, int32_t n_phi_sectors, float phi_slope_max, float phi_slope_outer_max,
                          float z0_max, void *workspace, size_t workspace_bytes, gnn_graph_build_sizes_t *sizes_out,
                          int64_t *hit_ptr, int64_t *seg_ptr, void *stream);
int gnn_graph_build_fill(const int64_t *particle_id, int64_t n_hits, int64_t n_events, const int32_t *layer_pairs,
                         int32_t n_pairs, int32_t n_layers, int32_t n_phi_sectors, float phi_slope_max,
                         float phi_slope_outer_max, float z0_max, double scale_r, double scale_phi, double scale_z,
                         const gnn_graph_build_sizes_t *sizes, void *workspace, size_t workspace_bytes, float *X,
                         int32_t *src, int32_t *dst, float *y, int64_t *hit_index, void *stream);

/* ---- the hit classifier's track samples from detector hits, built on the GPU (csrc/hit_samples.hip; ABI 7) ---------
 * Replaces the sample preparation of gnn/MPNN_HitClassifier.ipynb on the host in pandas: the deduplication of
 * select_hits (cell 5), select_signal_hits (cells 5 and 10), the signal keys (cell 11), the constants and arrays of
 * cells 12 and 14 and the per-sample loop of cell 15 with calc_eta / calc_dphi / calc_eta_phi_distance (cell 9).
 * gnn-fpga_amd/hit_samples.py is the numpy specification.  Two calls around ONE host read-back of the sizes:
 *   gnn_hit_samples_sizes  deduplication, event and track selection, sample numbering, kept hits grouped per
 *                          (event, layer) in frame order -> *sizes_out (DEVICE memory, written asynchronously)
 *   gnn_hit_samples_fill   X, y, hit_index, src, dst, keys into arrays the caller allocated from a HOST copy of the
 *                          sizes (the same workspace, not touched in between)
 * Inputs (DEVICE): r, phi, z float32 [n_hits], layer int32 [n_hits] (barrel layers already renumbered),
 * particle_id int64 [n_hits], event_ptr int64 [n_events + 1] (event e owns rows [event_ptr[e], event_ptr[e+1])).
 * L = n_det_layers <= 64, K = n_layer_hits <= 16 (GNN_ERR_BADARG otherwise).  Per (event, particle, layer) the hit of
 * smallest r is kept (the first row on ties); an event is dropped when a layer present in it has <= K kept hits; a
 * sample is an (event, particle) whose kept hits cover all L layers, numbered in ascending (event, particle_id).
 * Sample s owns hits [s L K, (s + 1) L K) of X [., 4] (r, phi - phi of its layer-0 hit wrapped to [-pi, pi], z, each
 * float32(float64(v) / scale), then the label on layers < n_seed_layers, 0 elsewhere), y (float32 label: the
 * candidate's particle is the sample's) and hit_index (input row, int64), layer-major, on each layer the K hits
 * nearest its own hit by d = sqrt(deta^2 + dphi^2) (float32, the track hit's eta in float64) in ascending d, the
 * first in frame order on equal d; segments [s K^2 (L-1), ...) of src (inner hit) and dst (outer hit) int32 in batch
 * numbering, every adjacent-layer pair in np.where order; keys [n_samples][2] int64 (event, particle_id).
 * sizes.status (0 = fine): bit 1 a layer outside [0, L), bit 2 more than 2^31 - 1 sample hits or segments, bit 4
 * event_ptr not non-decreasing from 0 to n_hits, bit 8 a non-finite r, phi or z; gnn_hit_samples_fill refuses
 * flagged sizes.  The output is the same in every run (no order decided by atomics). */
typedef struct gnn_hit_samples_sizes {
    int64_t n_samples, n_hits, n_segments;      /* samples; sample hits n_samples L K; segments n_samples K^2 (L-1) */
    int64_t n_kept, n_groups, n_tasks, status;  /* kept hits; (event, particle) pairs; fill work items             */
} gnn_hit_samples_sizes_t;

size_t gnn_hit_samples_workspace_bytes(int64_t n_hits, int64_t n_events, int32_t n_det_layers, int32_t n_layer_hits);
int gnn_hit_samples_sizes(const float *r, const float *phi, const float *z, const int32_t *layer,
                          const int64_t *particle_id, int64_t n_hits, const int64_t *event_ptr, int64_t n_events,
                          int32_t n_det_layers, int32_t n_layer_hits, void *workspace, size_t workspace_bytes,
                          gnn_hit_samples_sizes_t *sizes_out, void *stream);
int gnn_hit_samples_fill(const float *r, const float *phi, const float *z, const int64_t *particle_id, int64_t n_hits,
                         int64_t n_events, int32_t n_det_layers, int32_t n_layer_hits, int32_t n_seed_layers,
                         double scale_r, double scale_phi, double scale_z, const gnn_hit_samples_sizes_t *sizes,
                         void *workspace, size_t workspace_bytes, float *X, float *y, int64_t *hit_index,
                         int32_t *src, int32_t *dst, int64_t *keys, void *stream);

/* ---- muon trigger graphs from EMTF hits, built on the GPU (csrc/muon_graph.hip; ABI 7) ------------------------------
 * Replaces the reference's host graph preparation of the endcap muon trigger: gnn/prepareMuonGraphs.py main from the
 * tree.pandas.df reads (:171-173) through save_graphs (:263) - the LUT layer (:49-92, :175-176), the cross-frame and
 * truth filters (:178-192), the per-source deduplication and the mixing of PU into muon entries by ordinal (:193-232),
 * the layer pairs from Python set order (:234-246), pt / eta (:254) - and gnn/Muon_graph.py construct_graph with its
 * segment selection (:60-162).  gnn-fpga_amd/muon_graph.py is the numpy specification; the output is bit-identical.
 *   gnn_muon_graph_sizes   checks, deduplication, ordinals, graph composition, kept-segment counts -> *sizes_out,
 *                          hit_ptr, seg_ptr [n_entries + 1] (the first n_graphs + 1 used; DEVICE memory, written
 *                          asynchronously on `stream`)
 *   gnn_muon_graph_fill    the graphs into arrays the caller allocated from a HOST copy of the sizes (the same
 *                          workspace, not touched in between)
 *   gnn_muon_graph_padded  no read-back at all: graph slot e = entry e owns hits [42 e, 42 e + 42) and segments
 *                          [441 e, 441 e + 441) (21 chambers per source survive the deduplication; the pairs form a
 *                          bipartite graph over <= 42 hits); unused hits are X = 0 rows with hit_source = hit_row = -1,
 *                          unused segments src = dst = -1 with y = 0; outputs sized n_entries; *status (DEVICE int32)
 *                          receives the status word
 * Inputs (DEVICE): per source (muon, PU) the ten hit_features columns of :169-170 and event_ptr [n_entries + 1]
 * (entry e owns rows [event_ptr[e], event_ptr[e+1]), the subentry is the position in the entry); vp_pt, vp_eta
 * float32 [n_vp] the flat vp rows.  Graph g (flat: ascending entry over the entries that have rows, including graphs
 * with no layer pair) owns rows hit_ptr[g] .. hit_ptr[g+1] of X [., 11] (float32(column) for the ten features, then
 * the LUT layer times sign(z), +0 for z = +-0), hit_source (0 = PU, 1 = muon) and hit_row (int64, the row in its source), in the
 * reference's frame order; segments seg_ptr[g] .. seg_ptr[g+1] of src (l1 hit), dst (l2 hit) int32 in batch numbering
 * and y = 1 iff both hits are muon rows, pair by pair, l1 hit by l1 hit, then by l2 hit; entry = entry_start + e,
 * pt / eta = vp row e (NaN where e >= n_vp), flags bit 1 a graph (padded: the slot holds one), bit 2 written (the
 * reference saves a file: at least one layer pair), bit 4 vp row missing; graph_hits, graph_segments per graph.
 * status (0 = fine): bit 1 a type, station or ring outside [0, 5), bit 2 a non-finite z, bit 4 an event_ptr not
 * non-decreasing from 0 to n_rows (or an entry of 2^31 rows or more); gnn_muon_graph_fill refuses flagged sizes.
 * GNN_ERR_BADARG: null pointers, n_entries < 1; GNN_ERR_UNSUPPORTED: more than (2^31 - 1) / 441 entries.  The output
 * is the same in every run (no order decided by atomics). */
typedef struct gnn_emtf_hits {
    const float *z, *theta, *phi, *r;           /* vh_sim_z, vh_sim_theta, vh_sim_phi, vh_sim_r [n_rows]           */
    const int32_t *bend, *tp1, *tp2, *station, *ring, *type;   /* vh_bend, vh_sim_tp1, vh_sim_tp2, vh_station, ... */
    const int64_t *event_ptr;                   /* [n_entries + 1]                                                  */
    int64_t n_rows;
} gnn_emtf_hits_t;

typedef struct gnn_muon_graph_sizes {
    int64_t n_graphs, n_hits, n_segments, max_graph_hits, max_graph_segments, status;
} gnn_muon_graph_sizes_t;

typedef struct gnn_muon_graph_out {             /* DEVICE arrays: [n_hits] / [n_segments] / [n_graphs]              */
    float *X;
    int32_t *src, *dst;
    float *y;
    int32_t *hit_source;
    int64_t *hit_row, *entry;
    float *pt, *eta;
    int32_t *flags, *graph_hits, *graph_segments;
} gnn_muon_graph_out_t;

size_t gnn_muon_graph_workspace_bytes(int64_t n_entries);
int gnn_muon_graph_sizes(const gnn_emtf_hits_t *muon, const gnn_emtf_hits_t *pu, int64_t n_entries, int32_t muon_only,
                         void *workspace, size_t workspace_bytes, gnn_muon_graph_sizes_t *sizes_out, int64_t *hit_ptr,
                         int64_t *seg_ptr, void *stream);
int gnn_muon_graph_fill(const gnn_emtf_hits_t *muon, const gnn_emtf_hits_t *pu, int64_t n_entries, int32_t muon_only,
                        const float *vp_pt, const float *vp_eta, int64_t n_vp, int64_t entry_start,
                        const gnn_muon_graph_sizes_t *sizes, void *workspace, size_t workspace_bytes,
                        const gnn_muon_graph_out_t *out, void *stream);
int gnn_muon_graph_padded(const gnn_emtf_hits_t *muon, const gnn_emtf_hits_t *pu, int64_t n_entries, int32_t muon_only,
                          const float *vp_pt, const float *vp_eta, int64_t n_vp, int64_t entry_start, void *workspace,
                          size_t workspace_bytes, const gnn_muon_graph_out_t *out, int32_t *status, void *stream);

/* ---- ACTS full-event graphs from cluster hits, built on the GPU (csrc/event_graphs.hip; ABI 7) ----------------------
 * Replaces the host graph preparation of gnn/MPNN_Seg_ACTS_fullEvents.ipynb: select_hits (cell 5: barrel selection,
 * layer renumbering, deduplication in pandas), calc_dphi (cell 7), construct_graph (cell 8: three dense N x N masks,
 * two dense N x E matrices, an int64 matmul for the labels) and the dataset loop with its occupancy filter (cells
 * 16-18).  gnn-fpga_amd/event_graphs.py is the numpy specification; the output is bit-identical.  Two calls around
 * ONE host read-back of the sizes:
 *   gnn_event_graphs_workspace_bytes  device scratch both calls need (cells 5 and 8 allocate theirs in numpy)
 *   gnn_event_graphs_sizes  cell 5, the window test of cell 8 counted per start hit, the filter of cells 17-18 ->
 *                           *sizes_out, hit_ptr, seg_ptr [n_events + 1] and event_index [n_events] (the first
 *                           n_graphs (+ 1) used; DEVICE memory, written asynchronously on `stream`)
 *   gnn_event_graphs_fill   cell 8's X, edge list and labels (and merge_samples' float32 cast, cell 24) into arrays
 *                           the caller allocated from a HOST copy of the sizes (the same workspace, not touched in
 *                           between; the same cuts)
 * Inputs (DEVICE): r, phi, z float32 [n_rows], volid, layid int32 [n_rows], barcode int64 [n_rows], event_ptr int64
 * [n_events + 1] (event e owns rows [event_ptr[e], event_ptr[e+1])).  Rows whose volid is not 8, 13 or 17 are
 * dropped; layer = int8(layid / 2 - 1 + 4 * volume) in float64, truncated toward zero (negative layers are legal);
 * per (event, barcode, layer) the hit of smallest r is kept (the first row on ties); an event's hits are ordered by
 * (barcode, layer), both signed.  For start hit i in that order, then end hit j in that order with layer[j] -
 * layer[i] == 1, float32: dphi = phi[i] - phi[j], minus f32(2 pi) if > f32(pi), then plus f32(2 pi) if < -f32(pi);
 * kept when |dphi| < dphi_max and |z[j] - z[i]| < dz_max.  An event is a graph when it has a kept hit and
 * n_hits > n_nodes_min, n_hits < n_nodes_max, n_segments < n_edges_max (pass -1 / INT64_MAX for no test).  Graph g
 * (event event_index[g], ascending) owns rows hit_ptr[g] .. hit_ptr[g+1] of X [., 3] (float32(float64(v) / scale)
 * of r, phi, z), hit_index (int64, the input row) and layer (int32), and segments seg_ptr[g] .. seg_ptr[g+1] of src
 * (start hit), dst (end hit) int32 in batch numbering and y = 1 iff both hits share a barcode.
 * sizes.status (0 = fine): bit 1 a barrel row whose layer is outside int8, bit 2 more than 2^31 - 1 tested segments,
 * bit 4 event_ptr not non-decreasing from 0 to n_rows, bit 8 a non-finite r, phi or z; gnn_event_graphs_fill refuses
 * flagged sizes.  GNN_ERR_BADARG: null pointers, n_rows < 0, n_events < 1, a NaN cut, a zero or NaN scale;
 * GNN_ERR_UNSUPPORTED: 2^31 - 1 rows or events, or more.  The output is the same in every run (no order decided by
 * atomics). */
typedef struct gnn_event_graphs_sizes {
    int64_t n_graphs, n_hits, n_segments;       /* kept events; their hits; their segments                          */
    int64_t n_kept, n_tasks, n_tested, status;  /* hits after deduplication; pair work items; segments counted      */
} gnn_event_graphs_sizes_t;

size_t gnn_event_graphs_workspace_bytes(int64_t n_rows, int64_t n_events);
int gnn_event_graphs_sizes(const float *r, const float *phi, const float *z, const int32_t *volid, const int32_t *layid,
                           const int64_t *barcode, int64_t n_rows, const int64_t *event_ptr, int64_t n_events,
                           float dphi_max, float dz_max, int64_t n_nodes_min, int64_t n_nodes_max, int64_t n_edges_max,
                           void *workspace, size_t workspace_bytes, gnn_event_graphs_sizes_t *sizes_out,
                           int64_t *hit_ptr, int64_t *seg_ptr, int64_t *event_index, void *stream);
int gnn_event_graphs_fill(const float *r, const float *phi, const float *z, const int64_t *barcode, int64_t n_rows,
                          int64_t n_events, float dphi_max, float dz_max, double scale_r, double scale_phi,
                          double scale_z, const gnn_event_graphs_sizes_t *sizes, void *workspace,
                          size_t workspace_bytes, float *X, int32_t *src, int32_t *dst, float *y, int64_t *hit_index,
                          int32_t *layer, void *stream);

/* ---- TrackML barrel hits selected from raw event tables on the GPU (csrc/select_hits.hip; ABI 7) ---------------------
 * Replaces select_hits of gnn/prepareGraphs.py:53-85, which runs on the host in pandas: the barrel (volume, layer)
 * pairs mapped to layers 0 .. 9 (:55-62), pt and its cut (:64-67), truth merged with the kept particles (:68-69), r
 * and phi (:71-72), hits merged with truth (:74-76), the optional "hits every layer" filter (:77-80) and the
 * deduplication by groupby(['particle_id', 'layer']).r.idxmin() (:82-84).  gnn-fpga_amd/select_hits.py is the numpy
 * specification; the output is bit-identical (phi as given; without it, atan2f(y, x)).  Two calls around ONE host
 * read-back of the sizes:
 *   gnn_select_hits_workspace_bytes  device scratch both calls need
 *   gnn_select_hits_sizes  everything but the gather -> *sizes_out and event_ptr_out [n_events + 1] (DEVICE memory,
 *                          written asynchronously on `stream`)
 *   gnn_select_hits_fill   the selected hits' columns into arrays of n_kept entries the caller allocated from a HOST
 *                          copy of the sizes (the same workspace, not touched in between; the same no_missing_hits)
 * Inputs (DEVICE, but barrel_layers): hits hit_id int64, x, y, z float32, volume_id, layer_id int32 [n_hits]; truth
 * hit_id, particle_id int64 [n_truth]; particles particle_id int64, px, py float32 [n_particles]; one event_ptr int64
 * [n_events + 1] per table (event e owns rows [ptr[e], ptr[e+1]) of it); barrel_layers HOST int32 [n_layers, 2],
 * n_layers <= GNN_SELECT_HITS_MAX_LAYERS; phi float32 [n_hits] or NULL.
 * layer = the first k with barrel_layers[k] == (volume_id, layer_id), other rows are dropped; float32, every operation
 * rounded on its own: pt = sqrt(px px + py py), a particle is kept when pt > pt_min (strictly), r = sqrt(x x + y y);
 * a hit survives when its hit_id has a truth row in its own event whose particle_id is a kept particle of its own
 * event (ids compared as int64); with no_missing_hits a particle is kept only if its hits cover n_layers distinct
 * layers; per (event, particle_id, layer) the hit of smallest r is kept, the lowest row on equal r.  Output: within an
 * event by particle_id ascending (signed), then layer; event e owns entries event_ptr_out[e] .. event_ptr_out[e+1].
 * sizes.status (0 = fine): bit 4 an event_ptr not non-decreasing from 0 to its table's rows, bit 8 a non-finite x or
 * y, bit 16 a hit_id twice in an event's hits or truth rows or a particle_id twice in an event's particles;
 * gnn_select_hits_fill refuses flagged sizes.  GNN_ERR_BADARG: null pointers, negative sizes, n_events < 1, n_layers
 * outside 1 .. 64, a NaN pt_min; GNN_ERR_UNSUPPORTED: 2^31 - 1 rows or events, or more.  The output is the same in
 * every run (no order decided by atomics). */
#define GNN_SELECT_HITS_MAX_LAYERS 64

typedef struct gnn_select_hits_sizes {
    int64_t n_kept, status;                     /* selected hits; the status word                                   */
} gnn_select_hits_sizes_t;

size_t gnn_select_hits_workspace_bytes(int64_t n_hits, int64_t n_truth, int64_t n_particles, int64_t n_events);
int gnn_select_hits_sizes(const int64_t *hit_id, const float *x, const float *y, const int32_t *volume_id,
                          const int32_t *layer_id, int64_t n_hits, const int64_t *hit_event_ptr,
                          const int64_t *truth_hit_id, const int64_t *truth_particle_id, int64_t n_truth,
                          const int64_t *truth_event_ptr, const int64_t *particle_id, const float *px, const float *py,
                          int64_t n_particles, const int64_t *particle_event_ptr, int64_t n_events,
                          const int32_t *barrel_layers, int32_t n_layers, float pt_min, int32_t no_missing_hits,
                          void *workspace, size_t workspace_bytes, gnn_select_hits_sizes_t *sizes_out,
                          int64_t *event_ptr_out, void *stream);
int gnn_select_hits_fill(const int64_t *hit_id, const float *x, const float *y, const float *z, const float *phi,
                         int64_t n_hits, int64_t n_truth, int64_t n_particles, int64_t n_events,
                         int32_t no_missing_hits, const gnn_select_hits_sizes_t *sizes, void *workspace,
                         size_t workspace_bytes, float *r_out, float *phi_out, float *z_out, int32_t *layer_out,
                         int64_t *particle_id_out, int64_t *hit_id_out, int64_t *row_out, void *stream);

/* ---- scoring a classifier: confusion counts, score histograms (csrc/metrics.hip; ABI 7) ----------------------------
 * Stands in for the evaluation cells of the reference's notebooks (gnn/MPNN_Seg_ACTS*.ipynb, makeROC and the
 * per-sample cells), which flatten Estimator.predict's scores (gnn/estimator.py:137-146) and call sklearn.metrics
 * accuracy_score / precision_score / recall_score on `pred > thresh` and roc_curve on the scores, on the host.
 * gnn-fpga_amd/metrics.py (segment_metrics_numpy) is the specification of every counter.
 *   gnn_metrics_bins(key_shift): histogram bins per class, (0x3F800000 >> key_shift) + 1, for key_shift in [10, 23]
 *     (8192 .. 1 bins per octave); 0 otherwise.  A score's bin is its float32 bit pattern (sign cleared) >> key_shift.
 *   gnn_metrics_workspace_bytes: device scratch the update needs (0 in this version; pass what it returns).
 *   gnn_segment_metrics_update: ONE pass over e [n] scores, y [n] labels (float32) and, unless NULL, src [n] int32
 *     (src < 0 = padded segment, skipped).  Class c = 0 for y == 0, 1 for y == 1.  ADDS (int64, device, caller-owned,
 *     so calls stream over batches) into counts [T + 1][2] (row 0: segments per class, row 1 + k: segments with
 *     e > thresholds[k]) and hist [2][gnn_metrics_bins(key_shift)].  thresholds: HOST array of T <= 16 floats.
 *     With seg_ptr [n_graphs + 1] (device int64; graph g = segments [seg_ptr[g], seg_ptr[g+1]), non-decreasing),
 *     per_graph [n_graphs][T + 1][2] is WRITTEN with the same counts graph by graph; both NULL or both given.
 *     status [1] (device int32) is ORed with: 1 a score NaN, inf or outside [0, 1]; 2 a label not exactly 0 or 1;
 *     4 a threshold not finite (such segments are counted nowhere; the caller reads the word and raises).
 *     Integer atomics only: the counters are the same in every run.  Asynchronous on `stream`, no read-back. */
int64_t gnn_metrics_bins(int32_t key_shift);
size_t gnn_metrics_workspace_bytes(int64_t n, int32_t n_thresholds, int32_t key_shift, int64_t n_graphs);
int gnn_segment_metrics_update(const float *e, const float *y, const int32_t *src, int64_t n, const float *thresholds,
                               int32_t n_thresholds, int32_t key_shift, int64_t *counts, int64_t *hist,
                               const int64_t *seg_ptr, int64_t n_graphs, int64_t *per_graph, int32_t *status,
                               void *workspace, size_t workspace_bytes, void *stream);

/* ---- track candidates from scored segments, and their matching to particles (csrc/track_build.hip; ABI 7) ------------
 * The reference has no counterpart: it ends at one score per segment (Estimator.predict, gnn/estimator.py:137-146) and
 * its notebooks draw the scored segments (the draw_sample(..., alpha_labels=True) cells); gnn/Graph_dev.ipynb says
 * that multi-track finding was not tried.  These entry points follow on from there: hits -> tracks -> track-level
 * efficiency and fake rate, on the device.  gnn-fpga_amd/tracks.py (build_tracks_numpy, match_tracks_numpy) is the
 * specification of every array; all results are integers, the same in every run (labels are minima and maxima,
 * integer atomics only, stable sorts).
 * A batch: src, dst int32 [n_segments] (src < 0: padded segment, skipped), scores float32 [n_segments], hit_ptr int64
 * [n_graphs + 1] non-decreasing from 0 to n_hits (graph g owns hits [hit_ptr[g], hit_ptr[g+1])); all DEVICE memory.
 * Segment j is a CANDIDATE when src[j] >= 0, src[j] != dst[j], both ends inside [0, n_hits) and scores[j] > threshold
 * (strictly; never for NaN).  KEPT: GNN_TRACKS_COMPONENTS every candidate; GNN_TRACKS_BEST the candidates that are both
 * the best outgoing candidate of their src and the best incoming candidate of their dst (largest score, -0 = +0, ties
 * to the smallest segment id).  A hit's root is the smallest hit of its component over the kept segments (undirected);
 * components of at least min_hits hits are the tracks, numbered in ascending order of root.
 *   gnn_track_build_workspace_bytes  device scratch of labels + lists (0: a size negative or >= 2^31)
 *   gnn_track_build_labels  gnn/estimator.py:137-146's scores -> root [n_hits] int32, track_of_hit [n_hits] int32
 *                           (-1: no track) and sizes_out [4] int64 = {n_tracks, hits in tracks, kept segments, status};
 *                           asynchronous on `stream`, nothing read back.  status bits: 1 a NaN score on a segment with
 *                           src >= 0, 2 a kept segment whose hits lie in different graphs, 4 an endpoint outside
 *                           [0, n_hits) (such a segment is no candidate).
 *   gnn_track_build_lists   from a HOST copy of sizes_out (the same workspace, not touched in between): track_ptr
 *                           [n_tracks + 1], track_hits [hits in tracks] (a track's hits in ascending hit id),
 *                           track_graph [n_tracks] (the graph of the root), graph_track_ptr [n_graphs + 1] (graph g
 *                           owns tracks [ptr[g], ptr[g+1])); all int32.
 *   gnn_track_match_workspace_bytes  device scratch of gnn_track_match (0: bad sizes)
 *   gnn_track_match         what the draw_sample cells leave to the eye: particle_id int64 [n_hits] (ids <= 0: no
 *                           particle; a particle is a (graph, id) pair) -> per track majority_particle int64 (most
 *                           hits in the track, ties to the smallest id, 0: noise only), majority_hits, particle_hits
 *                           (that particle's hits in its graph), matched (2 majority_hits > track size and
 *                           2 majority_hits > particle_hits), int32 each, and counts [4] int64 WRITTEN with {tracks,
 *                           matched tracks, particles with >= min_hits hits, those of them that are the majority of a
 *                           matched track}.
 * GNN_ERR_BADARG names the argument: sizes negative or >= 2^31, a threshold that is not finite, an unknown mode,
 * min_hits < 1, n_tracks / n_track_hits that cannot be this workspace's, a missing pointer; a null or short workspace
 * is GNN_ERR_WORKSPACE. */
#define GNN_TRACKS_COMPONENTS 0
#define GNN_TRACKS_BEST 1
size_t gnn_track_build_workspace_bytes(int64_t n_hits, int64_t n_segments);
int gnn_track_build_labels(const int32_t *src, const int32_t *dst, const float *scores, int64_t n_segments,
                           int64_t n_hits, const int64_t *hit_ptr, int64_t n_graphs, float threshold, int32_t mode,
                           int32_t min_hits, void *workspace, size_t workspace_bytes, int32_t *root,
                           int32_t *track_of_hit, int64_t *sizes_out, void *stream);
int gnn_track_build_lists(const int32_t *track_of_hit, int64_t n_hits, const int64_t *hit_ptr, int64_t n_graphs,
                          int64_t n_tracks, int64_t n_track_hits, void *workspace, size_t workspace_bytes,
                          int32_t *track_ptr, int32_t *track_hits, int32_t *track_graph, int32_t *graph_track_ptr,
                          void *stream);
size_t gnn_track_match_workspace_bytes(int64_t n_hits, int64_t n_tracks);
int gnn_track_match(const int32_t *track_of_hit, const int64_t *particle_id, int64_t n_hits, const int64_t *hit_ptr,
                    int64_t n_graphs, const int32_t *track_ptr, int64_t n_tracks, int32_t min_hits, void *workspace,
                    size_t workspace_bytes, int64_t *majority_particle, int32_t *majority_hits, int32_t *particle_hits,
                    int32_t *matched, int64_t *counts, void *stream);

/* ---- the fit of track candidates: curvature, impact parameter, z0, chi2 per track (csrc/track_fit.hip; ABI 7) --------
 * The reference has no counterpart: it ends at segment scores, and a track candidate of gnn_track_build_lists is a
 * list of hit ids.  gnn-fpga_amd/tracks.py fit_tracks_numpy is the specification and the kernel restates it operation
 * for operation in float64 without contraction: every output equals it bit for bit.
 * Track t owns track_hits[track_ptr[t] .. track_ptr[t+1]) (int32, as gnn_track_build_lists writes them), visited in
 * that order; x, y, z double [n_hits] in mm, in the batch's hit order; all DEVICE memory.  Per hit r2 = x x + y y,
 * r = sqrt(r2); every sum runs over the track's hits in list order from 0.0.
 *   moments [n_tracks, 13]  the sums of x, y, z, r2, x x, x y, y y, x r2, y r2, r2 r2, r, r z, z z
 *   params  [n_tracks, 8]   rho, c, s, d, chi2_circle - Karimaki's non-iterative circle fit (NIM A305 (1991) 187),
 *                           unweighted: curvature, the direction (cos, sin) at the point of closest approach (d s, -d c),
 *                           oriented from the hit of smallest r2 to the one of largest, the signed distance of closest
 *                           approach; rho > 0 bends clockwise - and cot, z0, chi2_line of the straight line
 *                           z = z0 + cot r (gnn/graph.py's z0 variable, not the arc-length fit of a helix)
 *   n_fit   [n_tracks]      int32, the track's number of hits
 *   status  [n_tracks]      int32, 0 = fitted; bit 1 fewer than 3 hits (moments only, params NaN); 2 more than max_hits
 *                           hits (not visited, all NaN); 4 a coordinate that is not finite (all NaN); 8 a degenerate
 *                           circle (its five parameters NaN); 16 a degenerate line (its three NaN); 32 a hit id outside
 *                           [0, n_hits), not read, or a track_ptr pair that leaves track_hits (all NaN).  8 and 16 are
 *                           decided only where 1, 2, 4 and 32 are clear.
 * max_hits is part of the definition: one lane owns one track, and the components of 10 k hits that
 * GNN_TRACKS_COMPONENTS can make are not tracks.  Asynchronous on `stream`, caller-allocated outputs, no workspace,
 * nothing read back; n_tracks == 0 returns 0 without a launch.  GNN_ERR_BADARG names the argument: sizes negative or
 * >= 2^31, max_hits < 3, a missing pointer with a non-zero size. */
int gnn_track_fit(const int32_t *track_ptr, const int32_t *track_hits, int64_t n_tracks, int64_t n_track_hits,
                  const double *x, const double *y, const double *z, int64_t n_hits, int32_t max_hits, double *moments,
                  double *params, int32_t *n_fit, int32_t *status, void *stream);

/* ---- graph-convolution classifiers (csrc/gcn.hip; ABI 7) ------------------------------------------------------------
 * Stand in for GraphConv / GraphConvSelfInt (gnn/GCN_Seg_Toy2D.ipynb cell 20, gnn/GCN_Toy2D.ipynb cell 11),
 * GCNBinaryClassifier (Seg cell 21, Toy2D cell 13) and GCRNBinaryClassifier (Toy2D cell 14), which multiply a dense
 * [B, N, N] adjacency into the node features once per layer (torch.matmul(a, x)).  gnn-fpga_amd/gcn.py holds the
 * modules; exact fp32 throughout.
 *   gnn_gcn_adj_t: the compressed adjacency of B graphs of N nodes.  row_cnt [B][N] entries of row i, row_idx /
 *     row_val [B][N][W] their column indices (ascending) and values; col_* the same for the transposed matrix (the
 *     entries of column j, ascending row index).  W >= 1 is one width for the whole tensor.  Nothing assumes A = A^T.
 *   gnn_gcn_net_t: the model.  dims [n_dims] = hidden_dims (n_dims - 1 graph-convolution layers, at most
 *     GNN_GCN_MAX_LAYERS); layer l takes cin = dims[l] (+ F with `residual`, GCRN's [h | x]) to dims[l + 1].
 *     GraphConvSelfInt: Wn [dout][cin] and bn [dout] = node_mod, Wg [dout][cin] = neighbor_mod.  GraphConv: Wn NULL,
 *     bn and Wg = linear's bias and weight.  Wf [dims[0]][F], bf: feature_extractor; Wc [dims[last]], bc [1]:
 *     classifier.  off_*: where each gradient starts in the flat grads [n_params] the backward writes.
 *   gnn_gcn_supported(N, F, max_width, list_width): 1 if the kernels take the shape; 0 otherwise, and gnn_last_error
 *     names the limit (the forward keeps two [N][max_width + F] row buffers in the 160 KB of LDS, and x beside them
 *     when it fits; the backward two [N][max_width] row buffers and x).
 *   gnn_gcn_compress_count: row_cnt, col_cnt [B][N] and info [2] (device int32: the widest list; status, bit 0 = a
 *     non-finite entry) from the dense fp32 a [B][N][N]; every entry with a != 0 counts.  The caller reads info back
 *     (the ONE read-back of a compression), sizes the lists (zero-filled) and calls gnn_gcn_compress_fill.
 *   gnn_gcn_forward: ONE launch, one workgroup per graph: out [B][N] logits from x [B][N][F].  H_all (NULL for
 *     inference) [B][n_dims][N][max_width] receives the post-ReLU h of every layer, which the backward reads:
 *     columns [0, dims[l]) of layer l are written, the columns past a layer's own width are UNSPECIFIED (never
 *     written, never read by gnn_gcn_backward).
 *   gnn_gcn_backward: ONE launch, one workgroup per graph (per-graph partial sums into the workspace, A^T gz pulled
 *     over the column lists, no float atomics) and ONE fixed-order reduction launch: grads [n_params] is WRITTEN, the
 *     same bits in every run.  grad_out [B][N] is the gradient of the logits.  No gradient for x or a.
 *   Everything is asynchronous on `stream`; no call reads anything back. */
#define GNN_GCN_MAX_LAYERS 16
typedef struct {
    const int32_t *row_cnt, *row_idx;
    const float *row_val;
    const int32_t *col_cnt, *col_idx;
    const float *col_val;
    int64_t B;
    int32_t N, W;
} gnn_gcn_adj_t;
typedef struct {
    const float *Wf, *bf, *Wc, *bc;
    const float *Wn[GNN_GCN_MAX_LAYERS], *bn[GNN_GCN_MAX_LAYERS], *Wg[GNN_GCN_MAX_LAYERS];
    int32_t dims[GNN_GCN_MAX_LAYERS + 1];
    int32_t off_n[GNN_GCN_MAX_LAYERS], off_b[GNN_GCN_MAX_LAYERS], off_g[GNN_GCN_MAX_LAYERS];
    int32_t off_f, off_bf, off_c, off_bc, n_params;
    int32_t n_dims, F, residual, max_width;
} gnn_gcn_net_t;
int gnn_gcn_supported(int32_t N, int32_t F, int32_t max_width, int32_t list_width);
int gnn_gcn_compress_count(const float *a, int64_t B, int32_t N, int32_t *row_cnt, int32_t *col_cnt, int32_t *info,
                           void *stream);
int gnn_gcn_compress_fill(const float *a, int64_t B, int32_t N, int32_t W, int32_t *row_idx, float *row_val,
                          int32_t *col_idx, float *col_val, void *stream);
int gnn_gcn_forward(const gnn_gcn_adj_t *adj, const gnn_gcn_net_t *net, const float *x, float *out, float *H_all,
                    void *stream);
size_t gnn_gcn_backward_workspace_bytes(int64_t B, int32_t n_params);
int gnn_gcn_backward(const gnn_gcn_adj_t *adj, const gnn_gcn_net_t *net, const float *x, const float *H_all,
                     const float *grad_out, float *grads, void *workspace, size_t workspace_bytes, void *stream);

/* ---- the toy notebooks' graphs, built into compressed adjacencies (csrc/toy_graphs.hip; ABI 7) ----------------------
 * Stand in for the data cells of gnn/GCN_Seg_Toy2D.ipynb (cells 10-17 and 24: cell 12 is a Python triple loop over
 * events x segments x segments into a dense fp64 [E, S, S] array) and gnn/GCN_Toy2D.ipynb (cells 8 and 17 with cell
 * 4's calc_adjacency, norm_adjacency and kwnorm_adjacency: three dense fp64 [E, N, N] arrays).  Both builders take an
 * event's n_layers x n_tracks hits - hit_x [E][L T] positions, layer-major and sorted within a layer, hit_y int32
 * [E][L T] the sort index (track label) - and write gnn_gcn_adj_t's lists directly: ONE launch each, no dense tensor,
 * nothing read back.  The list contract is gnn_gcn_compress_fill's: an entry is listed if and only if its fp32 value
 * is != 0, indices ascend, lists are zero-padded, one width W for the whole tensor.  gnn-fpga_amd/synth.py
 * (toy_segment_graphs_from_hits, toy_hit_graphs_from_hits) is the specification of every array.  All DEVICE memory.
 *   gnn_toy_graphs_list_width(kind, L, T, norm): W = min(2 T, nodes), one more with GNN_TOY_NORM_KW's diagonal; 0 when
 *     the kernels do not take the shape (gnn_last_error names the limit: L >= 2, 1 <= T <= 16, at most 4096 segments
 *     S = T^2 (L - 1) or hits N = L T per event).
 *   gnn_toy_segment_graphs: det_r float32 [L]; two_sigma2 = float32(2 sigma^2).  Segment (l, a, b) = hit a of layer l
 *     to hit b of layer l + 1 has index (l T + a) T + b.  X [E][S][5] = (x0, x1, r0, r1, slope), y [E][S] = the two
 *     hits share a label, row_cnt [E][S], row_idx / row_val [E][S][W]: the segments that end where this one starts or
 *     start where it ends, weighted exp(-(slope_j - slope_i)^2 / two_sigma2) in fp32.  The matrix is symmetric bit for
 *     bit: the column lists are the row lists.
 *   gnn_toy_hit_graphs: hit_x and det_r fp64; r_norm float32 [L] = det_r / det_r[L - 1]; norm_table fp64 [2 T + 2]
 *     indexed by a count: GNN_TOY_NORM_ROW {0, 1/1, 1/2, ...}, GNN_TOY_NORM_KW {0, 1/sqrt(1), 1/sqrt(2), ...}, made on
 *     the host (NULL for GNN_TOY_NORM_NONE).  X [E][N][3] = (x, r_norm, label == target on the first seed_size
 *     layers), y0 [E][N] = label == target, the row lists and, computed entry by entry and never mirrored, the column
 *     lists of calc_adjacency's matrix under `norm`; a hit whose column of the binary matrix is empty (the notebook's
 *     1 / 0) gets a zero row and counts into n_isolated (device int64, WRITTEN; the one atomic counter).
 * GNN_ERR_BADARG names the argument: an unknown kind or norm, n_events negative or 2^31 and more, two_sigma2 not
 * positive and finite, a missing pointer; GNN_ERR_UNSUPPORTED names the shape limit. */
#define GNN_TOY_SEGMENTS 0
#define GNN_TOY_HITS 1
#define GNN_TOY_NORM_NONE 0
#define GNN_TOY_NORM_ROW 1
#define GNN_TOY_NORM_KW 2
int32_t gnn_toy_graphs_list_width(int32_t kind, int32_t n_layers, int32_t n_tracks, int32_t norm);
int gnn_toy_segment_graphs(const float *hit_x, const int32_t *hit_y, const float *det_r, int64_t n_events,
                           int32_t n_layers, int32_t n_tracks, float two_sigma2, float *X, float *y, int32_t *row_cnt,
                           int32_t *row_idx, float *row_val, void *stream);
int gnn_toy_hit_graphs(const double *hit_x, const int32_t *hit_y, const double *det_r, const float *r_norm,
                       const double *norm_table, int64_t n_events, int32_t n_layers, int32_t n_tracks,
                       int32_t seed_size, int32_t norm, int32_t target, float *X, float *y0, int32_t *row_cnt,
                       int32_t *row_idx, float *row_val, int32_t *col_cnt, int32_t *col_idx, float *col_val,
                       int64_t *n_isolated, void *stream);

/* ---- choosing the graph builder's arguments: all-pair histograms and a layer census (ABI 7) ------------------------
 * gnn-fpga_amd/cut_study.py is the numpy specification of both.  All arrays are DEVICE memory except layer_pairs
 * (HOST, as gnn_graph_build_sizes takes it); both calls are asynchronous on `stream` and read nothing back.
 *   gnn_cut_study (csrc/graph_build.hip) replaces the all-pairs loops of gnn/GraphConstructionDev.ipynb cell 20 and
 *     gnn/GraphConstructionDev_mu200.ipynb cell 18 and the histograms of their cells 21-25: for every graph (event x
 *     phi sector, split and re-centred exactly as gnn_graph_build_sizes does), every (l1, l2) of layer_pairs and every
 *     (l1 hit, l2 hit) it computes phi_slope and z0 with the float32 operations of gnn/graph.py:57-62 (the builder's
 *     own pair arithmetic) and counts the pair in counts [n_pairs][2][n_slope_edges + 1][n_z0_edges + 1] (int64,
 *     WRITTEN: zeroed first; axis 1: 0 = the particle ids differ, 1 = they are equal, the builder's y).  The bin of a
 *     value is the number of edges <= |value| (np.searchsorted(edges, |v|, side="right")); NaN goes to the last bin,
 *     so a pair with r2 == r1 sits in the last bin of both axes.  The edges are float32, strictly increasing and free
 *     of NaN (the caller's duty: they are not checked here; the last may be +inf).  A pair with a layer that has no
 *     hit in the graph adds nothing (gnn/graph.py:82-89).  *status (int64, WRITTEN) holds gnn_graph_build_sizes'
 *     status bits 1 and 4.  GNN_ERR_BADARG as gnn_graph_build_sizes, and fewer than one edge on an axis;
 *     GNN_ERR_UNSUPPORTED: more than 4096 cells (n_slope_edges + 1) * (n_z0_edges + 1) (the per-workgroup table lives
 *     in LDS), 2^25 hits or more, and gnn_graph_build_sizes' limits.  Only integers are summed: every run gives the
 *     same bits.  gnn_cut_study_workspace_bytes returns 0 for arguments gnn_cut_study refuses.
 *   gnn_layer_census (csrc/layer_census.hip) replaces gnn/GraphConstructionDev.ipynb cells 16-17 and 37-41 (group the
 *     hits by (evtid, barcode), sort each group by r, count which layer follows which): table [n_layers][n_layers]
 *     (int64, WRITTEN: zeroed first), entry [a][b] = how often a hit of layer b directly follows a hit of layer a among
 *     the hits of one (event, particle_id) ordered by r; equal r is ordered by input row.  has_skip != 0 leaves out
 *     the hits whose particle_id is skip_particle_id.  *status (int64, WRITTEN): bit 1 a layer outside [0, n_layers),
 *     bit 4 a malformed event_ptr, bit 8 a NaN r; the table of a flagged call means nothing.  GNN_ERR_UNSUPPORTED:
 *     more than 4096 layers, 2^31 hits or more. */
size_t gnn_cut_study_workspace_bytes(int64_t n_hits, int64_t n_events, const int32_t *layer_pairs, int32_t n_pairs,
                                     int32_t n_layers, int32_t n_phi_sectors, int32_t n_slope_edges, int32_t n_z0_edges);
int gnn_cut_study(const float *r, const float *phi, const float *z, const int32_t *layer, const int64_t *particle_id,
                  int64_t n_hits, const int64_t *event_ptr, int64_t n_events, const int32_t *layer_pairs, int32_t n_pairs,
                  int32_t n_layers, int32_t n_phi_sectors, const float *phi_slope_edges, int32_t n_slope_edges,
                  const float *z0_edges, int32_t n_z0_edges, void *workspace, size_t workspace_bytes, int64_t *counts,
                  int64_t *status, void *stream);
size_t gnn_layer_census_workspace_bytes(int64_t n_hits, int64_t n_events, int32_t n_layers);
int gnn_layer_census(const float *r, const int32_t *layer, const int64_t *particle_id, int64_t n_hits,
                     const int64_t *event_ptr, int64_t n_events, int32_t n_layers, int32_t has_skip,
                     int64_t skip_particle_id, void *workspace, size_t workspace_bytes, int64_t *table, int64_t *status,
                     void *stream);

/* bound_out (device, 1 float) = the left side of the GNN_FLAG_EXP_PRODUCT condition;
 * x_absmax (device, [F]) = per-feature max |X|.  Asynchronous on `stream`. */
int gnn_exp_product_bound(const gnn_params_t *p, const float *x_absmax, float *bound_out,
                          void *stream);

/* Per-kernel timing with HIP events on the launch stream (bench.py's roofline leg).
 * gnn_profile_begin(capacity) arms recording of up to `capacity` kernel launches;
 * gnn_profile_end synchronises the recorded events and returns the number of records,
 * filling names[i] (static strings) and ms[i] for i < min(count, capacity_out). */
int gnn_profile_begin(int32_t capacity);
int gnn_profile_end(const char **names, float *ms, int32_t capacity_out);

#ifdef __cplusplus
}
#endif
#endif /* GNN_HIP_H */
