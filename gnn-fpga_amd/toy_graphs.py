"""The toy notebooks' graphs on the device, built straight into the compressed adjacency of gcn.py (csrc/toy_graphs.hip).

gnn/GCN_Seg_Toy2D.ipynb builds its inputs with a Python triple loop over events x 225 x 225 segment pairs (cell 12) into
a dense fp64 [32768, 225, 225] array; gnn/GCN_Toy2D.ipynb builds three dense fp64 [65536, 40, 40] intermediates and
normalises them event by event (cells 4 and 17).  A row of either matrix has at most 2 T entries (T tracks per event).
Here one launch per builder writes X, the labels and a `SparseAdjacency` from an event's n_layers x n_tracks hits: no
dense tensor, and nothing is read back - the list width is known before the launch.

    tracks [E, T, L] --sort_toy_tracks--> hit_x, hit_y [E, L T] --build_toy_segment_graphs--> X, y, adj [E, S, S]
                                                                --build_toy_hit_graphs------> X, y0, adj [E, N, N]

`synth.toy_segment_graphs_from_hits` and `synth.toy_hit_graphs_from_hits` are the numpy specification of every array.
There is no CPU path: CPU tensors raise, and so does a shape the kernels do not take (the message names the limit).
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib, synth
from .gcn import SparseAdjacency

ToySegmentGraphs = namedtuple("ToySegmentGraphs", ["X", "y", "adj"])
ToyHitGraphs = namedtuple("ToyHitGraphs", ["X", "y0", "adj", "n_isolated"])


def sort_toy_tracks(tracks):
    """generate_data's sort (Seg cell 3, Toy2D cell 4): tracks [E, T, L] positions on the device -> (hit_x, hit_y)
    [E, L * T], layer-major and sorted within each layer; hit_y int64 is the sort index, the track a hit belongs to.
    Equal positions keep the lower track first, which is what numpy's argsort gives for arrays this small."""
    if not torch.is_tensor(tracks) or not tracks.is_cuda:
        raise _lib.GnnHipError("sort_toy_tracks needs a tensor on a ROCm device; there is no CPU path")
    if tracks.dim() != 3 or not tracks.dtype.is_floating_point:
        raise _lib.GnnHipError("sort_toy_tracks takes floating-point [n_events, n_tracks, n_layers] positions, got %s %s"
                               % (tracks.dtype, tuple(tracks.shape)))
    E = tracks.shape[0]
    x, order = torch.sort(tracks.transpose(1, 2), dim=-1, stable=True)
    return x.reshape(E, -1).contiguous(), order.reshape(E, -1).contiguous()


def _det_r(det_r):
    det = np.asarray(det_r, dtype=np.float64)
    if det.ndim != 1 or det.shape[0] < 2:
        raise ValueError("det_r must list at least 2 detector layers, got shape %s" % (det.shape,))
    if not np.isfinite(det).all() or not (np.diff(det.astype(np.float32)) > 0).all():
        raise ValueError("det_r must be finite and strictly increasing (in float32 too), got %s" % (det.tolist(),))
    return det


def _hits(who, hit_x, hit_y, L, dtypes, check):
    """The validated (hit_x, hit_y int32, T) of a builder."""
    for name, t in (("hit_x", hit_x), ("hit_y", hit_y)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise _lib.GnnHipError("%s: %s must be a tensor on a ROCm device; there is no CPU path" % (who, name))
    if hit_x.dtype not in dtypes:
        raise TypeError("%s: hit_x must be %s, got %s" % (who, " or ".join(str(d) for d in dtypes), hit_x.dtype))
    if hit_y.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
        raise TypeError("%s: hit_y must be an integer tensor, got %s" % (who, hit_y.dtype))
    if hit_x.dim() != 2 or hit_y.shape != hit_x.shape or hit_x.shape[1] == 0 or hit_x.shape[1] % L:
        raise ValueError("%s: hit_x and hit_y must both be [n_events, n_layers * n_tracks] with n_layers = %d, got %s "
                         "and %s" % (who, L, tuple(hit_x.shape), tuple(hit_y.shape)))
    if hit_x.device != hit_y.device:
        raise _lib.GnnHipError("%s: hit_x is on %s and hit_y on %s" % (who, hit_x.device, hit_y.device))
    if hit_x.requires_grad:
        raise _lib.GnnHipError("%s: hit_x requires grad: the builders have no gradient" % who)
    if check and not bool(torch.isfinite(hit_x).all()):
        raise ValueError("%s: hit_x has a non-finite entry (NaN or Inf)" % who)
    return hit_x.detach().contiguous(), hit_y.to(torch.int32).contiguous(), hit_x.shape[1] // L


def build_toy_segment_graphs(hit_x, hit_y, det_r=synth.TOY_DET_R, sigma=0.01, check=True):
    """The segment graphs of gnn/GCN_Seg_Toy2D.ipynb, cells 10-17 and 24, on the device: hit_x float32 [E, L * T]
    positions sorted within each layer (layer-major), hit_y integer [E, L * T] track labels, as `sort_toy_tracks` or
    the notebook's generate_data (cell 3) gives them.

    Returns ToySegmentGraphs(X [E, S, 5] fp32 = (x0, x1, r0, r1, slope), y [E, S] fp32, adj) with S = T^2 (L - 1)
    segments in the order `synth.toy_segment_graphs_from_hits` documents (cell 10's np.triu(...).nonzero()) and `adj`
    a SparseAdjacency [E, S, S] of width min(2 T, S): cell 12's adjacency times cell 17's Gaussian kernel of the slope
    difference, in float32.  The matrix is symmetric bit for bit, so adj.col_* ARE adj.row_* (the same tensors).
    Entries whose kernel value underflows to 0.0 are not listed (the counts may be smaller than the width).

    One launch, no dense tensor.  `check` tests hit_x for NaN / Inf first, the one value read back; check=False reads
    nothing back.  X, y and the slope equal the specification bit for bit; a kernel value differs from numpy's by the
    two exp implementations only."""
    who = "build_toy_segment_graphs"
    det = _det_r(det_r)
    sigma = float(sigma)
    if not (sigma > 0.0 and np.isfinite(sigma)):
        raise ValueError("%s: sigma must be positive and finite, got %r" % (who, sigma))
    two_sigma2 = float(np.float32(2 * sigma ** 2))
    if not (two_sigma2 > 0.0 and np.isfinite(two_sigma2)):
        raise ValueError("%s: 2 sigma^2 = %r is not a positive finite float32" % (who, two_sigma2))
    L = det.shape[0]
    x, y, T = _hits(who, hit_x, hit_y, L, (torch.float32,), check)
    W = _lib.toy_list_width(_lib.GNN_TOY_SEGMENTS, L, T)
    _lib.gcn_require(T * T * (L - 1), 5, 1, W)
    r = torch.from_numpy(det.astype(np.float32)).to(x.device)
    X, ys, cnt, idx, val = _lib.toy_segment_graphs(x, y, r, L, T, two_sigma2)
    return ToySegmentGraphs(X, ys, SparseAdjacency(cnt, idx, val, cnt, idx, val))


def build_toy_hit_graphs(hit_x, hit_y, det_r=synth.TOY_DET_R, seed_size=3, norm="row", target=0, check=True):
    """The hit graphs of gnn/GCN_Toy2D.ipynb, cells 8 and 17 with cell 4's calc_adjacency, norm_adjacency and
    kwnorm_adjacency, on the device: hit_x float64 [E, L * T] (float32 is widened exactly) and hit_y as for
    `build_toy_segment_graphs`.

    Returns ToyHitGraphs(X [E, N, 3] fp32 = (x, r / r_max, the target-track flag on the first seed_size layers),
    y0 [E, N] fp32 = the hit is on track `target`, adj, n_isolated) with N = L * T and `adj` a SparseAdjacency
    [E, N, N] of width min(2 T, N) (one more for "kw"'s diagonal): hits of adjacent layers whose connecting line
    enters and leaves inside (0, 1), with `norm` = None (binary), "row" (norm_adjacency; NOT symmetric) or "kw"
    (kwnorm_adjacency).  All fp64 arithmetic is the cell's, entry by entry - a[i, j] and a[j, i] round differently and
    neither is mirrored - and every array equals `synth.toy_hit_graphs_from_hits` bit for bit.

    n_isolated is a device int64 [1]: the hits no line reaches (an empty column of the binary matrix), which get a
    zero row under "row" where the notebook writes NaN.  It is not read back.  One launch, no dense tensor; `check` as
    for `build_toy_segment_graphs`."""
    who = "build_toy_hit_graphs"
    if norm not in (None, "row", "kw"):
        raise ValueError("%s: norm must be None, 'row' or 'kw', got %r" % (who, norm))
    det = _det_r(det_r)
    L = det.shape[0]
    x, y, T = _hits(who, hit_x, hit_y, L, (torch.float64, torch.float32), check)
    W = _lib.toy_list_width(_lib.GNN_TOY_HITS, L, T, norm)
    _lib.gcn_require(L * T, 3, 1, W)
    seed_size, target = int(seed_size), int(target)
    if not -2 ** 31 <= target < 2 ** 31:
        raise ValueError("%s: target %d is no int32 track label" % (who, target))
    seed_size = min(max(seed_size, 0), L)
    dev = x.device
    c = np.arange(1, 2 * T + 2, dtype=np.float64)
    table = None
    if norm == "row":
        table = np.concatenate([[0.0], 1.0 / c])
    elif norm == "kw":
        table = np.concatenate([[0.0], 1.0 / np.sqrt(c)])
    if table is not None:
        table = torch.from_numpy(table).to(dev)
    r = torch.from_numpy(det).to(dev)
    r_norm = torch.from_numpy((det / det.max()).astype(np.float32)).to(dev)
    X, y0, rc, ri, rv, cc, ci, cv, n_iso = _lib.toy_hit_graphs(x.double(), y, r, r_norm, table, L, T, seed_size, norm,
                                                               target)
    return ToyHitGraphs(X, y0, SparseAdjacency(rc, ri, rv, cc, ci, cv), n_iso)
