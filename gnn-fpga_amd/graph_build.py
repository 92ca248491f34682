"""Track-segment graphs from detector hits: the reference's graph construction on the GPU.

Replaces, per event, gnn/prepareGraphs.py:136-170 (`process_event`): the phi-sector split
(`split_phi_sectors`, :87-106) followed by one `construct_graph` per sector (gnn/graph.py:37-142),
which pairs every hit of layer l1 with every hit of layer l2 in pandas and keeps the pairs that pass
the phi-slope and z0 cuts.  `build_graphs` returns the graphs of all events and sectors as one
HitGraphBatch, event-major and sector-minor.

What it computes, exactly as the reference does for float32 hit columns (TrackML's r, phi and z):

* sectors: edges np.linspace(-pi, pi, S + 1); a hit is in sector i when edge_i < phi < edge_i+1,
  compared in float64 (a hit exactly on an edge belongs to no sector and is dropped); its phi is
  re-centred in float32: (phi - f32(edge_i)) - f32(width / 2);
* pairs, for every (l1, l2) of `layer_pairs` in order, l1 hits in frame order, for each of them the l2
  hits in frame order, all float32 and in this order of operations:
  dphi = phi2 - phi1, minus f32(2 pi) if > f32(pi), then plus f32(2 pi) if < -f32(pi);
  phi_slope = dphi / (r2 - r1); z0 = z1 - (r1 * (z2 - z1)) / (r2 - r1);
  kept when |phi_slope| < f32(phi_slope_max if l1 < 5 else phi_slope_outer_max) and |z0| < f32(z0_max)
  (the cut is chosen by the pair's first layer: gnn/graph.py:65); r2 == r1 is never kept;
* X = float32(float64([r, phi_centred, z]) / feature_scale), feature_scale = (1000, pi / S, 1000)
  (gnn/prepareGraphs.py:149-150); src = start hit, dst = end hit, within the batch; y = float32(pid1 == pid2).

Differences from the reference: a sector with no layer pair that has hits on both of its layers gives a
graph without segments (the reference raises from pd.concat([])); `no_missing_hits` and `max_tracks`
(an unseeded shuffle) are not provided; thresholds are Python floats rounded to float32, as the
reference's command-line values are.

CUDA tensors run csrc/graph_build.hip (two calls around one read-back of the sizes); numpy arrays or CPU
tensors run `build_graphs_numpy`, the specification, and give a CPU batch.
"""
import numpy as np
import torch

from .hitgraph import HitGraphBatch

FEATURES = ("r", "phi", "z")
INNER_LAYERS = 5          # gnn/graph.py:65: pairs whose first layer is below this take phi_slope_max
GB_STATUS_LAYER = 1       # csrc/graph_build.hip: a layer outside [0, n_layers)
GB_STATUS_INT32 = 2       # more than 2^31 - 1 segments
GB_STATUS_EVENTS = 4      # event_ptr not 0 .. n_hits, non-decreasing
_STATUS_WORDS = ((GB_STATUS_LAYER, "layer outside [0, n_layers)"), (GB_STATUS_INT32, "more than 2^31 - 1 segments"),
                 (GB_STATUS_EVENTS, "malformed event_ptr"))

_PI32 = np.float32(np.pi)             # numpy rounds np.pi and 2 np.pi to float32 against float32 data
_TWO_PI32 = np.float32(2 * np.pi)


def wrap_dphi32(d):
    """The references' phi wrap (calc_dphi) on a float32 difference: minus f32(2 pi) where > f32(pi), then plus
    f32(2 pi) where < -f32(pi).  The one numpy statement of csrc/builder_common.h's wrap_dphi."""
    d = np.asarray(d)
    assert d.dtype == np.float32
    d = np.where(d > _PI32, d - _TWO_PI32, d)
    return np.where(d < -_PI32, d + _TWO_PI32, d)


def sector_edges(n_phi_sectors):
    """gnn/prepareGraphs.py:88-89: the float64 sector edges and the half width the hits are centred by."""
    return np.linspace(-np.pi, np.pi, n_phi_sectors + 1), 2 * np.pi / n_phi_sectors / 2


def _host(a, what=None):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.asarray(a)


def _raise_builder_status(builder, words, status):
    """ValueError for a non-zero status word of a builder: `words` is its ((bit, what it means), ...) table."""
    if status:
        raise ValueError("%s status %d (%s)" % (builder, status, ", ".join(w for b, w in words if status & b)))


def _check_on_device(dev, **columns):
    """Every column (None: not given) must be a tensor on r's device."""
    for name, t in columns.items():
        if t is not None and (not torch.is_tensor(t) or t.device != dev):
            raise ValueError("%s must be a tensor on %s like r" % (name, dev))


def _check_inputs(r, phi, z, layer, layer_pairs, particle_id, event_ptr, n_phi_sectors):
    """Host-side validation shared by both paths: returns (n_hits, pairs int32 [P, 2], event_ptr int64 or None)."""
    cols = (("r", r), ("phi", phi), ("z", z))
    for name, c in cols:
        if c.dtype in (np.float64, torch.float64):
            raise ValueError("%s is float64: the reference's cuts are float32 arithmetic on float32 columns; "
                             "convert explicitly if that is what you mean" % name)
        if c.dtype not in (np.float32, torch.float32):
            raise ValueError("%s must be float32, got %s" % (name, c.dtype))
        if len(c.shape) != 1:
            raise ValueError("%s must be one-dimensional" % name)
    n = int(r.shape[0])
    for name, c in cols[1:] + (("layer", layer),) + ((("particle_id", particle_id),) if particle_id is not None else ()):
        if len(c.shape) != 1 or int(c.shape[0]) != n:
            raise ValueError("%s has %s entries, r has %d" % (name, tuple(c.shape), n))
    if int(n_phi_sectors) != n_phi_sectors or n_phi_sectors < 1:
        raise ValueError("n_phi_sectors must be a positive integer")
    pairs = np.asarray(_host(layer_pairs, "layer_pairs"), dtype=np.int64).reshape(-1, 2) if len(layer_pairs) else \
        np.zeros((0, 2), np.int64)
    if pairs.size and pairs.min() < 0:
        raise ValueError("layer_pairs holds a negative layer")
    if pairs.size and pairs.max() >= 2 ** 31:
        raise ValueError("layer_pairs entry outside int32")
    ep = None
    if event_ptr is not None:
        ep = np.asarray(_host(event_ptr, "event_ptr"), dtype=np.int64).ravel()
        if ep.size < 2 or ep[0] != 0 or ep[-1] != n or np.any(np.diff(ep) < 0):
            raise ValueError("event_ptr must run non-decreasing from 0 to the number of hits (%d)" % n)
    if n >= 2 ** 31:
        raise ValueError("more than 2^31 - 1 hits")
    return n, pairs.astype(np.int32), ep


def build_graphs(r, phi, z, layer, layer_pairs, *, particle_id=None, event_ptr=None, n_phi_sectors=1,
                 phi_slope_max=0.001, phi_slope_outer_max=None, z0_max=200.0, feature_scale=None):
    """Segment graphs of every (event, sector) as one HitGraphBatch (see the module docstring).

    r, phi, z: float32 [n]; layer: integer [n]; layer_pairs: [P, 2] (l1, l2) in order; particle_id: integer
    [n] or None (then the batch has no y); event_ptr: [n_events + 1], event e owns rows event_ptr[e] ..
    event_ptr[e+1] (default: one event).  phi_slope_outer_max defaults to phi_slope_max; feature_scale to
    (1000, pi / n_phi_sectors, 1000).  The batch carries `hit_index` [n_hits] int64: the input row of each
    of its hits, where the batch lives.
    """
    n, pairs, ep = _check_inputs(r, phi, z, layer, layer_pairs, particle_id, event_ptr, n_phi_sectors)
    if phi_slope_outer_max is None:
        phi_slope_outer_max = phi_slope_max
    if feature_scale is None:
        feature_scale = (1000.0, np.pi / n_phi_sectors, 1000.0)
    feature_scale = tuple(float(s) for s in np.asarray(feature_scale, dtype=np.float64).ravel())
    if len(feature_scale) != 3:
        raise ValueError("feature_scale needs one value per feature %s" % (FEATURES,))
    cuts = (float(phi_slope_max), float(phi_slope_outer_max), float(z0_max))
    if ep is None:
        ep = np.array([0, n], dtype=np.int64)
    if torch.is_tensor(r) and r.is_cuda:
        return _build_device(r, phi, z, layer, pairs, particle_id, ep, int(n_phi_sectors), cuts, feature_scale)
    cols = [_host(c, k) for c, k in ((r, "r"), (phi, "phi"), (z, "z"), (layer, "layer"))]
    pid = None if particle_id is None else _host(particle_id, "particle_id")
    return build_graphs_numpy(*cols, pairs, pid, ep, int(n_phi_sectors), cuts, feature_scale)


def pair_values(rr, pp, zz, i, j):
    """gnn/graph.py:57-62 for the hit pairs (i[k], j[k]): (phi_slope, z0), float32, in the reference's order of
    operations.  The one numpy statement of csrc/builder_common.h's pair_slope_z0; r2 == r1 gives inf or NaN."""
    dphi = wrap_dphi32(pp[j] - pp[i])
    dz = zz[j] - zz[i]
    dr = rr[j] - rr[i]
    with np.errstate(divide="ignore", invalid="ignore"):
        slope = dphi / dr
        z0 = zz[i] - rr[i] * dz / dr
    assert dphi.dtype == slope.dtype == z0.dtype == np.float32
    return slope, z0


def _segments(rr, pp, zz, lay, pairs, cut_inner, cut_outer, z0_cut):
    """One graph's segments in the reference's order: (start positions, end positions)."""
    starts, ends = [], []
    for l1, l2 in pairs:
        a = np.flatnonzero(lay == l1)
        b = np.flatnonzero(lay == l2)
        if a.size == 0 or b.size == 0:          # gnn/graph.py:84-90: a layer without hits skips the pair
            continue
        i = np.repeat(a, b.size)                # the merge's order: left rows, then right rows, in frame order
        j = np.tile(b, a.size)
        slope, z0 = pair_values(rr, pp, zz, i, j)
        cut = cut_inner if l1 < INNER_LAYERS else cut_outer
        keep = (np.abs(slope) < cut) & (np.abs(z0) < z0_cut)
        starts.append(i[keep])
        ends.append(j[keep])
    if not starts:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(starts), np.concatenate(ends)


def build_graphs_numpy(r, phi, z, layer, pairs, particle_id, event_ptr, n_phi_sectors, cuts, feature_scale):
    """The specification (host arrays, validated by build_graphs): a CPU HitGraphBatch with hit_index."""
    r, phi, z = (np.asarray(c, dtype=np.float32) for c in (r, phi, z))
    layer = np.asarray(layer)
    if layer.size and layer.min() < 0:
        raise ValueError("negative layer id")
    edges, half = sector_edges(n_phi_sectors)
    half32 = np.float32(half)
    cut_inner, cut_outer, z0_cut = (np.float32(c) for c in cuts)
    scale = np.asarray(feature_scale, dtype=np.float64)
    Xs, srcs, dsts, ys, idx = [], [], [], [], []
    hit_ptr, seg_ptr = [0], [0]
    for e in range(event_ptr.shape[0] - 1):
        rows = np.arange(event_ptr[e], event_ptr[e + 1])
        ph64 = phi[rows].astype(np.float64)
        for s in range(n_phi_sectors):
            h = rows[(ph64 > edges[s]) & (ph64 < edges[s + 1])]
            cphi = (phi[h] - np.float32(edges[s])) - half32
            assert cphi.dtype == np.float32
            a, b = _segments(r[h], cphi, z[h], layer[h], pairs, cut_inner, cut_outer, z0_cut)
            X = (np.stack([r[h], cphi, z[h]], axis=1).astype(np.float64) / scale).astype(np.float32)
            Xs.append(X)
            srcs.append(a + hit_ptr[-1])
            dsts.append(b + hit_ptr[-1])
            if particle_id is not None:
                ys.append((particle_id[h][a] == particle_id[h][b]).astype(np.float32))
            idx.append(h)
            hit_ptr.append(hit_ptr[-1] + h.size)
            seg_ptr.append(seg_ptr[-1] + a.size)
    if seg_ptr[-1] >= 2 ** 31:
        raise ValueError("more than 2^31 - 1 segments")
    X = np.concatenate(Xs) if Xs else np.zeros((0, 3), np.float32)
    src = np.concatenate(srcs).astype(np.int32)
    dst = np.concatenate(dsts).astype(np.int32)
    y = np.concatenate(ys) if particle_id is not None else None
    batch = HitGraphBatch(X, src, dst, y=y, hit_ptr=hit_ptr, seg_ptr=seg_ptr, _checked=True)
    batch.hit_index = torch.from_numpy(np.concatenate(idx).astype(np.int64))
    return batch


def _build_device(r, phi, z, layer, pairs, particle_id, event_ptr, n_phi_sectors, cuts, feature_scale):
    from . import _lib
    _check_on_device(r.device, phi=phi, z=z, layer=layer, particle_id=particle_id)
    layer = layer.to(torch.int32).contiguous()
    n = int(r.shape[0])
    if n:
        lo, hi = torch.aminmax(layer)
        lo, hi = (int(v) for v in torch.stack([lo, hi]).tolist())
        if lo < 0:
            raise ValueError("negative layer id")
    else:
        hi = -1
    n_layers = max(hi, int(pairs.max()) if pairs.size else -1) + 1
    pid = None if particle_id is None else particle_id.to(torch.int64).contiguous()
    ep = torch.from_numpy(event_ptr).to(r.device)
    r, phi, z = (t.contiguous() for t in (r, phi, z))
    ws, sizes, hit_ptr, seg_ptr = _lib.graph_build_sizes(r, phi, z, layer, ep, pairs, n_layers, n_phi_sectors, cuts)
    _raise_builder_status("graph builder", _STATUS_WORDS, sizes.status)
    X, src, dst, y, hit_index = _lib.graph_build_fill(ws, sizes, pid, ep, pairs, n_layers, n_phi_sectors, cuts,
                                                      feature_scale, n)
    batch = HitGraphBatch._from_device_arrays(X, src, dst, y, hit_ptr, seg_ptr)
    batch.hit_index = hit_index
    return batch
