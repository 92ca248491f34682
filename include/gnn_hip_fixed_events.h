/* gnn_hip_fixed_events.h - C ABI of the one-launch fixed-point forward for batches of SMALL graphs (fourth public
 * header of libgnn_hip.so).
 *
 * gnn_fx_forward of gnn_hip_fixed.h runs SegmentClassifier.forward (gnn/model.py:140-156) in fixed point with one
 * kernel per reference module: 15 launches at three iterations, whatever the size of the batch.  The reference's
 * target is a trigger on small muon graphs (about 20 hits and 70 segments); the entry point here runs a whole
 * block-diagonal batch of such graphs in ONE launch, one workgroup per graph, everything the graph needs resident in
 * LDS.  The arithmetic is that of gnn_hip_fixed.h, unchanged (format, requant, lookup; DESIGN.md, "Fixed point"):
 * integers only, so the results equal gnn_fx_forward's bit for bit.  A workgroup owns a graph, so this entry point can
 * also say how many overflows EACH graph had - for a trigger one wrapped word spoils an event.
 *
 * Every convention of gnn_hip.h and gnn_hip_fixed.h holds (caller-allocated device memory, asynchronous work on
 * `stream`, no hidden synchronisation or copy, 0 / negative return values with gnn_last_error(), padded segments
 * src = dst = -1, capturable in a HIP graph).  GNN_ABI_VERSION of gnn_hip.h covers this header too.
 */
#ifndef GNN_HIP_FIXED_EVENTS_H
#define GNN_HIP_FIXED_EVENTS_H

#include "gnn_hip_fixed.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of LDS one workgroup of gnn_fxev_forward needs for graphs of at most max_hits hits and max_segments segments:
 * the ten weight tensors (gnn/model.py:132-134,45-48,94-97), both tables of 2^table_bits entries, two tables of hit
 * rows H (gnn/model.py:146,154), the sums mi | mo (gnn/model.py:118-119), the per-hit halves of the edge network's
 * first layer as int64, one score per segment (gnn/model.py:150) and the graph's index arrays as local ids.
 * 0: no kernel for (F, D), table_bits outside 4..12, or a size outside [0, 2^31). */
size_t gnn_fxev_lds_bytes(int32_t F, int32_t D, int32_t table_bits, int64_t max_hits, int64_t max_segments);

/* 1 if gnn_fxev_forward runs graphs of that size at (input_dim, hidden_dim) = (F, D) - the shapes of
 * gnn_shape_supported (gnn/model.py:130-138) - that is, if gnn_fxev_lds_bytes is non-zero and within a workgroup's
 * 160 KB.  The wide shapes answer yes for tiny graphs only. */
int gnn_fxev_supported(int32_t F, int32_t D, int32_t table_bits, int64_t max_hits, int64_t max_segments);

/* SegmentClassifier.forward (gnn/model.py:140-156) in fixed point for a block-diagonal batch of small graphs, in one
 * kernel launch (plus the memset of `counts`); no workspace.  hit_ptr / seg_ptr [n_graphs + 1] and the six lists of
 * `g` as gnn_iter_forward_events takes them (all required); max_hits / max_segments bound every graph.  Per pass
 * t = 0 .. n_iters (any n_iters >= 0) the edge network (gnn/model.py:69-81) scores every segment, padded ones
 * included, and for t < n_iters the node network (gnn/model.py:113-125) updates the hits, as gnn_fx_forward does.
 * Written, every element: e_raw [n_segments] int32, e_float [n_segments] = e_raw * 2^-Fb, counts [(n_iters + 1) *
 * GNN_FX_STAGES] int64 - all as gnn_fx_forward writes them, the same bits; graph_overflows [n_graphs] int64 or NULL,
 * the overflows of graph i over all passes and stages (0 for a graph of no hits and no segments; they add up to the
 * sum of `counts`); e_trace [(n_iters + 1), n_segments] and H_trace [(n_iters + 1), n_hits, C] int32 or NULL, as in
 * gnn_fx_forward.  An array of no elements may be NULL.
 * The exactness bound of gnn_fx_forward (every list shorter than 2^(65 - 2 W) >= 131 072 entries) always holds: a
 * graph that fits a workgroup's LDS has fewer than 7 000 segments.
 * GNN_ERR_BADARG names the argument; GNN_ERR_UNSUPPORTED: gnn_fx_supported or gnn_fxev_supported says no (the
 * message gives the LDS bytes needed and the limit).  Nothing is launched in either case. */
int gnn_fxev_forward(const gnn_graph_t *g, const gnn_fx_params_t *p, const gnn_fx_format_t *fmt,
                     const gnn_fx_tables_t *tables, const int32_t *hit_ptr, const int32_t *seg_ptr, int64_t n_graphs,
                     int32_t max_hits, int32_t max_segments, int32_t n_iters, int32_t *e_raw, float *e_float,
                     int64_t *counts, int64_t *graph_overflows, int32_t *e_trace, int32_t *H_trace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GNN_HIP_FIXED_EVENTS_H */
