/* gnn_hip_iter.h - C ABI of the per-iteration segment classifier (second public header of libgnn_hip.so).
 *
 * The toy notebook gnn/MPNN_Seg_Toy2D.ipynb, cell 14, defines two classifiers.  `SegmentClassifier2` shares one
 * edge network and one node network across its iterations: that is gnn_segclf_* of gnn_hip.h.  `SegmentClassifier`
 * gives every iteration its own edge_networks[i] and node_networks[i] and scores with a separate output_network:
 *
 *     H = [tanh(Win X + bin) | X]                                          (cell 14, input_network + shortcut)
 *     for i in 0 .. n_iters-1:
 *         e = edge_networks[i](H);  H = [node_networks[i](H, e) | X]       (cell 14, SegmentClassifier.forward)
 *     return output_network(H)
 *
 * The entry points here run that forward and its backward for a block-diagonal batch of SMALL graphs (the notebook's
 * events: 40 hits, 144 segments) in one launch each, one workgroup per graph, with a different weight set per pass.
 * Every convention of gnn_hip.h holds (caller-allocated device memory, float32 row-major, nn.Linear's [out, in]
 * layout, asynchronous work on `stream`, no hidden synchronisation or copy, 0 / negative return values with
 * gnn_last_error(), padded segments src = dst = -1, rows H[n] = [H'(D) | X(F) | 0-pad] gnn_h_stride(F, D) apart,
 * capturable in a HIP graph).  GNN_ABI_VERSION of gnn_hip.h covers this header too.
 */
#ifndef GNN_HIP_ITER_H
#define GNN_HIP_ITER_H

#include "gnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GNN_ITER_MAX 16 /* most iterations one call takes (the notebook trains 10, cell 17) */

/* One network's four tensors, device pointers (cell 14: EdgeNetwork.network / NodeNetwork.network, layers 0 and 2). */
typedef struct gnn_iter_set {
    const float *Wa, *ba; /* .network.0  edge: [D,2C] [D]   node: [D,3C] [D] */
    const float *Wb, *bb; /* .network.2  edge: [1,D]  [1]   node: [D,D]  [D] */
} gnn_iter_set_t;

/* The weights of one model (cell 14, SegmentClassifier.__init__), passed BY VALUE to the kernels (about 1 KB of
 * kernel arguments: nothing is uploaded per call).  Entries [n_iters, GNN_ITER_MAX) of edge / node are not read.
 * shared = 1 restates SegmentClassifier2 (cell 14): every edge[i] and `out` must be the SAME four tensors and every
 * node[i] the same four; the backward then sums the passes' gradients into the ten-tensor layout of gnn_grads_t. */
typedef struct gnn_iter_params {
    const float *Win, *bin;            /* input_network.0                  [D,F] [D] */
    gnn_iter_set_t edge[GNN_ITER_MAX]; /* edge_networks.i.network.{0,2}              */
    gnn_iter_set_t node[GNN_ITER_MAX]; /* node_networks.i.network.{0,2}              */
    gnn_iter_set_t out;                /* output_network.network.{0,2}               */
    int32_t F, D, n_iters;
    int32_t shared;
} gnn_iter_params_t;

/* 1 if graphs of at most max_hits hits and max_segments segments fit one workgroup's LDS at this (F, D) - the
 * forward (cell 14, SegmentClassifier.forward), and with backward != 0 also the backward (what loss.backward() of
 * the notebook's Estimator, cell 20, runs through the same cell). */
int gnn_iter_events_supported(int32_t F, int32_t D, int64_t max_hits, int64_t max_segments, int32_t backward);

/* SegmentClassifier.forward (cell 14) for a batch of small graphs in one launch.  hit_ptr / seg_ptr [n_graphs+1]
 * and the six lists of `g` as gnn_segclf_forward_train_events takes them (all required).  e_out [n_segments]: the
 * output network's scores, or NULL; e_all [(n_iters+1), n_segments] and H_all [(n_iters+1), n_hits, ldh]: every
 * pass's scores and hit rows for the backward, or both NULL (inference); an array of no elements (no segments, no
 * hits) may be NULL.  Sums run in list order; the arithmetic per
 * row is that of gnn_input_fwd / gnn_edge_fwd / gnn_node_fwd. */
int gnn_iter_forward_events(const gnn_graph_t *g, const gnn_iter_params_t *p, const int32_t *hit_ptr,
                            const int32_t *seg_ptr, int64_t n_graphs, int32_t max_hits, int32_t max_segments,
                            float *e_out, float *e_all, float *H_all, void *stream);

/* Number of floats of the flat gradient: state_dict order of cell 14's SegmentClassifier - input_network,
 * edge_networks.0 .. n_iters-1, node_networks.0 .. n_iters-1, output_network - or, shared, of SegmentClassifier2
 * (the ten tensors of gnn_grads_t).  0: bad arguments. */
int64_t gnn_iter_grad_floats(int32_t F, int32_t D, int32_t n_iters, int32_t shared);

/* Backward of cell 14's SegmentClassifier.forward for loss.backward() (cell 20 through gnn/estimator.py): given
 * grad_out [n_segments] = dLoss/d(scores) and e_all / H_all of gnn_iter_forward_events, WRITES every gradient into
 * grads_flat [gnn_iter_grad_floats] (no need to zero it).  One workgroup per graph writes its own row of partial
 * gradients, one slot per pass, into the workspace; a second kernel adds the rows in graph order (and, shared, the
 * passes in pass order): bit-reproducible from run to run.  Workspace: gnn_iter_backward_workspace_bytes. */
size_t gnn_iter_backward_workspace_bytes(int64_t n_graphs, int32_t F, int32_t D, int32_t n_iters);
int gnn_iter_backward_events(const gnn_graph_t *g, const gnn_iter_params_t *p, const int32_t *hit_ptr,
                             const int32_t *seg_ptr, int64_t n_graphs, int32_t max_hits, int32_t max_segments,
                             const float *e_all, const float *H_all, const float *grad_out, float *grads_flat,
                             void *workspace, size_t workspace_bytes, void *stream);

/* Backward of the input network alone (cell 14: input_network = Linear + Tanh, then the shortcut), for models that
 * run the passes module by module: given H0 [n_hits, ldh] = [tanh(Win X + bin) | X | 0] and gH0 [n_hits, ldg] =
 * dLoss/dH0 (first D columns used), WRITES gWin [D,F] then gbin [D] into grads_flat [D*F + D].  Chunks of hits are
 * summed in hit order, the chunks in chunk order.  Workspace: gnn_iter_input_bwd_workspace_bytes. */
size_t gnn_iter_input_bwd_workspace_bytes(int64_t n_hits, int32_t F, int32_t D);
int gnn_iter_input_bwd(const float *X, const float *H0, int32_t ldh, const float *gH0, int32_t ldg, int64_t n_hits,
                       int32_t F, int32_t D, float *grads_flat, void *workspace, size_t workspace_bytes,
                       void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GNN_HIP_ITER_H */
