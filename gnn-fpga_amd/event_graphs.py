"""ACTS full-event graphs from cluster hits: the reference's full-event graph preparation on the GPU.

Replaces, in gnn/MPNN_Seg_ACTS_fullEvents.ipynb, `select_hits` (cell 5), `calc_dphi` (cell 7), `construct_graph`
(cell 8) and the dataset loop with its occupancy filter (cells 16-18), which run on the host: pandas for the
selection, three dense N x N masks, two dense N x E matrices and an int64 matmul against them for the labels.
`build_event_graphs` returns the kept events as one HitGraphBatch in event order; `EventGraphs.store()` hands the
same graphs to `batch_generator`, whose padded batches of 4 are the notebook's `merge_samples` batches (cells 24-25).
There are no phi sectors and no `layer_pairs` list: every pair of hits on adjacent layers is tested against a window.

What it computes, exactly as the reference does for float32 hit columns:

* barrel selection and layers (cell 5): rows whose volid is not 8, 13 or 17 are dropped; volume = 0, 1, 2 for those
  three; layer = int8(layid / 2 - 1 + 4 * volume), float64 arithmetic truncated toward zero ((8, 9) -> 3,
  (17, 1) -> 7, (8, 0) -> -1).  Negative layers are legal: a layer -1 hit starts segments to layer 0;
* deduplication: per (event, barcode, layer) the hit of smallest r is kept, the first input row on exactly equal r
  (idxmin); every distinct barcode is a particle, negative values and 0 included;
* hit order inside an event: ascending (barcode, layer), both signed - the order `hits.loc[groupby(...).r.idxmin()]`
  leaves.  It decides the rows of X and the order of the segments;
* segments (cell 8): for start hit i in that order, then end hit j in that order with layer[j] - layer[i] == 1, all
  float32 and in this order of operations: dphi = phi[i] - phi[j], minus f32(2 pi) if > f32(pi), then plus f32(2 pi)
  if < -f32(pi); kept when |dphi| < f32(dphi_max) and |z[j] - z[i]| < f32(dz_max) (NaN compares false); src = i,
  dst = j, positions within the batch: np.where order of the dense adjacency, start-hit-major;
* y = float32(barcode[i] == barcode[j]); X = float32(float64([r, phi, z]) / feature_scale) (the division is float64
  in cell 8, the float32 cast is merge_samples', cell 24);
* events (cells 16-18): an event without a kept hit gives no graph; with bounds given an event is kept when
  n_hits > n_nodes_min and n_hits < n_nodes_max and n_segments < n_edges_max (all strict; an absent bound is no
  test); graphs are numbered in event order among the kept ones and `event_index` says which events they are.

Differences from the reference: (1) cell 5 raises KeyError when an input has no hit in one of the three barrel
volumes (`get_group`): here the graphs are returned; (2) under pandas 2.3 `hits.loc[<DataFrame>]` does not run: the
fixtures take the `r` column of the idxmin result, which is the deduplication above; (3) a non-finite r, phi or z
(in any row), a malformed event_ptr, a layer outside int8 (the reference's cast is undefined there) and more than
2^31 - 1 hits or tested segments raise ValueError (the device builder flags them in its status word); (4) y is
float32, not bool; (5) thresholds are Python floats rounded to float32, which is what numpy 2 compares a float32
array against; (6) volid and layid are taken as int32, barcode as int64.

CUDA tensors run csrc/event_graphs.hip (two calls around one read-back of the sizes); numpy arrays or CPU tensors run
`build_event_graphs_numpy`, the specification, and give a CPU result.
"""
import numpy as np
import torch

from .graph_build import _check_on_device, _host, _raise_builder_status, wrap_dphi32
from .hitgraph import HitGraphBatch

BARREL_VOLUMES = (8, 13, 17)      # cell 5: vids
EG_STATUS_LAYER = 1               # csrc/event_graphs.hip: a barrel row whose layer is outside int8
EG_STATUS_INT32 = 2               # more than 2^31 - 1 tested segments
EG_STATUS_EVENTS = 4              # event_ptr not 0 .. n_rows, non-decreasing
EG_STATUS_FINITE = 8              # a non-finite r, phi or z
_STATUS_WORDS = ((EG_STATUS_LAYER, "layer outside int8"), (EG_STATUS_INT32, "more than 2^31 - 1 hits or segments"),
                 (EG_STATUS_EVENTS, "malformed event_ptr"), (EG_STATUS_FINITE, "a non-finite r, phi or z"))
NO_MIN, NO_MAX = -1, 2 ** 63 - 1  # what an absent bound is for the library: every count passes

_DENSE_HITS = 96                  # the specification tests events up to this size as one dense block


def _raise_status(st):
    _raise_builder_status("event graph builder", _STATUS_WORDS, st)


class EventGraphs:
    """The graphs of build_event_graphs, where the input lives.

    batch: HitGraphBatch of the kept events in event order (X [n_hits, 3], src / dst int32 in batch numbering, y
    float32, hit_ptr / seg_ptr per graph); event_index int64 [n_graphs]: the input event of each graph; hit_index
    int64 [n_hits]: the input row of each hit; layer int32 [n_hits]: its renumbered layer."""

    def __init__(self, batch, event_index, hit_index, layer):
        self.batch, self.event_index, self.hit_index, self.layer = batch, event_index, hit_index, layer

    def __len__(self):
        return self.batch.n_graphs

    def store(self):
        """A GraphStore of these graphs on the same device, made there: `batch_generator(store, n_samples,
        batch_size=4, layout="padded")` yields the notebook's batches (cells 24-25)."""
        from .batcher import GraphStore
        return GraphStore.from_batch(self.batch)


def _check_inputs(r, phi, z, volid, layid, barcode, event_ptr, dphi_max, dz_max, feature_scale, bounds):
    """Host-side validation shared by both paths: (n_rows, event_ptr int64, (dphi_max, dz_max), scale, bounds)."""
    for name, c in (("r", r), ("phi", phi), ("z", z)):
        if c.dtype in (np.float64, torch.float64):
            raise ValueError("%s is float64: the reference's cuts are float32 arithmetic on float32 columns; "
                             "convert explicitly if that is what you mean" % name)
        if c.dtype not in (np.float32, torch.float32):
            raise ValueError("%s must be float32, got %s" % (name, c.dtype))
        if len(c.shape) != 1:
            raise ValueError("%s must be one-dimensional" % name)
    n = int(r.shape[0])
    for name, c in (("volid", volid), ("layid", layid), ("barcode", barcode)):
        if c is None:
            raise ValueError("%s is required" % name)
        dt = c.dtype
        integer = (not dt.is_floating_point and dt not in (torch.bool, torch.complex64, torch.complex128)) \
            if torch.is_tensor(c) else np.issubdtype(dt, np.integer)
        if not integer:
            raise ValueError("%s must be an integer column, got %s" % (name, dt))
    for name, c in (("phi", phi), ("z", z), ("volid", volid), ("layid", layid), ("barcode", barcode)):
        if len(c.shape) != 1 or int(c.shape[0]) != n:
            raise ValueError("%s has %s entries, r has %d" % (name, tuple(c.shape), n))
    if n >= 2 ** 31 - 1:
        raise ValueError("more than 2^31 - 1 hits")
    if event_ptr is None:
        ep = np.array([0, n], dtype=np.int64)
    else:
        ep = _host(event_ptr, "event_ptr")
        if not np.issubdtype(ep.dtype, np.integer):
            raise ValueError("event_ptr must be integer")
        ep = ep.astype(np.int64).ravel()
        if ep.size < 2 or ep[0] != 0 or ep[-1] != n or np.any(np.diff(ep) < 0):
            raise ValueError("event_ptr must run non-decreasing from 0 to the number of hits (%d)" % n)
    cuts = (float(dphi_max), float(dz_max))
    if any(c != c for c in cuts):
        raise ValueError("dphi_max or dz_max is NaN")
    scale = tuple(float(s) for s in np.asarray(feature_scale, dtype=np.float64).ravel())
    if len(scale) != 3:
        raise ValueError("feature_scale needs one value per feature (r, phi, z)")
    if not all(s != 0.0 for s in scale):
        raise ValueError("a feature scale is zero or NaN")
    out = []
    for name, v, absent in (("n_nodes_min", bounds[0], NO_MIN), ("n_nodes_max", bounds[1], NO_MAX),
                            ("n_edges_max", bounds[2], NO_MAX)):
        if v is None:
            out.append(absent)
            continue
        if isinstance(v, bool) or int(v) != v:
            raise ValueError("%s must be an integer or None, got %r" % (name, v))
        out.append(min(max(int(v), NO_MIN), NO_MAX))       # counts are >= 0: below -1 and -1 are the same test
    return n, ep, cuts, scale, tuple(out)


def build_event_graphs(r, phi, z, volid, layid, barcode, event_ptr=None, *, dphi_max=np.pi / 4, dz_max=300.0,
                       feature_scale=(1000.0, np.pi, 1000.0), n_nodes_min=None, n_nodes_max=None, n_edges_max=None):
    """The full-event graphs of every kept event (see the module docstring) as EventGraphs.

    r, phi, z: float32 [n]; volid, layid: integer [n]; barcode: integer [n]; event_ptr: [n_events + 1], event e owns
    rows event_ptr[e] .. event_ptr[e+1] (default: one event).  n_nodes_min, n_nodes_max, n_edges_max: the occupancy
    filter of cells 17-18 (the notebook uses 50, 500, 1000), each an integer or None for no test."""
    n, ep, cuts, scale, bounds = _check_inputs(r, phi, z, volid, layid, barcode, event_ptr, dphi_max, dz_max,
                                               feature_scale, (n_nodes_min, n_nodes_max, n_edges_max))
    if torch.is_tensor(r) and r.is_cuda:
        return _build_device(r, phi, z, volid, layid, barcode, ep, cuts, scale, bounds)
    cols = [_host(c, k) for c, k in ((r, "r"), (phi, "phi"), (z, "z"), (volid, "volid"), (layid, "layid"),
                                     (barcode, "barcode"))]
    return build_event_graphs_numpy(*cols, ep, cuts[0], cuts[1], scale, *bounds)


def barrel_layers(volid, layid):
    """Cell 5's selection and renumbering: (selected bool [n], layer int64 [n], valid only where selected); a layer
    outside int8 on a selected row raises ValueError."""
    volid = np.asarray(volid).astype(np.int64)
    vol = np.full(volid.shape[0], -1, dtype=np.int64)
    for i, v in enumerate(BARREL_VOLUMES):
        vol[volid == v] = i
    sel = vol >= 0
    lay = np.trunc(np.asarray(layid).astype(np.float64) / 2 - 1 + 4 * vol)      # .astype(np.int8) truncates
    if np.any(sel & ((lay < -128) | (lay > 127))):
        _raise_status(EG_STATUS_LAYER)
    return sel, np.where(sel, lay, 0).astype(np.int64)


def _event_segments(phi, z, lay, dphi_cut, dz_cut):
    """One event's segments in np.where order of cell 8's adjacency: (start positions, end positions), layer by
    layer (a dense block per adjacent-layer pair), then put in start-hit order (the dense N x N masks of a
    detector-size event would not fit)."""
    if lay.shape[0] <= _DENSE_HITS:                      # a small event: cell 8 as it stands, one N x N block
        d = wrap_dphi32(phi[:, None] - phi[None, :])
        dz = z[None, :] - z[:, None]
        assert d.dtype == dz.dtype == np.float32
        return np.nonzero(((lay[None, :] - lay[:, None]) == 1) & (np.abs(d) < dphi_cut) & (np.abs(dz) < dz_cut))
    starts, ends = [], []
    order = np.argsort(lay, kind="stable")
    ls = lay[order]
    vals, first = np.unique(ls, return_index=True)
    last = np.append(first[1:], ls.shape[0])
    for k in range(vals.shape[0] - 1):
        if vals[k + 1] - vals[k] != 1:
            continue
        a, b = order[first[k]:last[k]], order[first[k + 1]:last[k + 1]]        # ascending positions on each layer
        d = wrap_dphi32(phi[a][:, None] - phi[b][None, :])                      # cell 7 as cell 8 calls it
        dz = z[b][None, :] - z[a][:, None]
        assert d.dtype == dz.dtype == np.float32
        ii, jj = np.nonzero((np.abs(d) < dphi_cut) & (np.abs(dz) < dz_cut))
        starts.append(a[ii])
        ends.append(b[jj])
    if not starts:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    i, j = np.concatenate(starts), np.concatenate(ends)
    o = np.argsort(i, kind="stable")          # each block is start-major with ascending ends: only starts interleave
    return i[o], j[o]


def build_event_graphs_numpy(r, phi, z, volid, layid, barcode, event_ptr, dphi_max=np.pi / 4, dz_max=300.0,
                             feature_scale=(1000.0, np.pi, 1000.0), n_nodes_min=NO_MIN, n_nodes_max=NO_MAX,
                             n_edges_max=NO_MAX):
    """The specification (host arrays, validated by build_event_graphs): a CPU EventGraphs."""
    r, phi, z = (np.asarray(c, dtype=np.float32) for c in (r, phi, z))
    bc = np.asarray(barcode).astype(np.int64)
    ep = np.asarray(event_ptr, dtype=np.int64)
    n, E = r.shape[0], ep.shape[0] - 1
    if not (np.isfinite(r).all() and np.isfinite(phi).all() and np.isfinite(z).all()):
        _raise_status(EG_STATUS_FINITE)
    sel, layer = barrel_layers(volid, layid)
    dphi_cut, dz_cut = np.float32(dphi_max), np.float32(dz_max)
    scale = np.asarray(feature_scale, dtype=np.float64)
    evt = np.repeat(np.arange(E, dtype=np.int64), np.diff(ep))
    rows = np.flatnonzero(sel)
    # cell 5: the hit of smallest r per (event, barcode, layer), the first row on ties; (event, barcode, layer) order
    order = rows[np.lexsort((rows, r[rows], layer[rows], bc[rows], evt[rows]))]
    ke, kb, kl = evt[order], bc[order], layer[order]
    first = np.ones(order.shape[0], dtype=bool)
    first[1:] = (ke[1:] != ke[:-1]) | (kb[1:] != kb[:-1]) | (kl[1:] != kl[:-1])
    kept = order[first]
    kevt = evt[kept]
    eh = np.searchsorted(kevt, np.arange(E + 1))           # kept hits of event e: kept[eh[e]:eh[e + 1]]
    Xs, srcs, dsts, ys, idx, events = [], [], [], [], [], []
    hit_ptr, seg_ptr, tested = [0], [0], 0
    for e in np.flatnonzero(np.diff(eh) > 0):
        h = kept[eh[e]:eh[e + 1]]
        nh = h.shape[0]
        if not (nh > n_nodes_min and nh < n_nodes_max):    # cell 18, the two tests that need no segments
            continue
        a, b = _event_segments(phi[h], z[h], layer[h], dphi_cut, dz_cut)
        tested += a.shape[0]
        if not a.shape[0] < n_edges_max:
            continue
        Xs.append((np.stack([r[h], phi[h], z[h]], axis=1).astype(np.float64) / scale).astype(np.float32))
        srcs.append(a + hit_ptr[-1])
        dsts.append(b + hit_ptr[-1])
        ys.append((bc[h][a] == bc[h][b]).astype(np.float32))
        idx.append(h)
        events.append(e)
        hit_ptr.append(hit_ptr[-1] + nh)
        seg_ptr.append(seg_ptr[-1] + a.shape[0])
    if tested >= 2 ** 31:
        _raise_status(EG_STATUS_INT32)
    cat = (lambda v, dt, shape=(0,): np.concatenate(v).astype(dt) if v else np.zeros(shape, dt))
    batch = HitGraphBatch(cat(Xs, np.float32, (0, 3)), cat(srcs, np.int32), cat(dsts, np.int32),
                          y=cat(ys, np.float32), hit_ptr=hit_ptr, seg_ptr=seg_ptr, _checked=True)
    hit_index = cat(idx, np.int64)
    return EventGraphs(batch, torch.from_numpy(np.array(events, dtype=np.int64)), torch.from_numpy(hit_index),
                       torch.from_numpy(layer[hit_index].astype(np.int32)))


def _build_device(r, phi, z, volid, layid, barcode, event_ptr, cuts, scale, bounds):
    from . import _lib
    _check_on_device(r.device, phi=phi, z=z, volid=volid, layid=layid, barcode=barcode)
    volid, layid = (t.to(torch.int32).contiguous() for t in (volid, layid))
    barcode = barcode.to(torch.int64).contiguous()
    ep = torch.from_numpy(event_ptr).to(r.device)
    r, phi, z = (t.contiguous() for t in (r, phi, z))
    ws, sizes, hit_ptr, seg_ptr, event_index = _lib.event_graphs_sizes(r, phi, z, volid, layid, barcode, ep, cuts,
                                                                       bounds)
    _raise_status(int(sizes.status))
    X, src, dst, y, hit_index, layer = _lib.event_graphs_fill(ws, sizes, r, phi, z, barcode,
                                                              int(event_ptr.shape[0]) - 1, cuts, scale)
    batch = HitGraphBatch._from_device_arrays(X, src, dst, y, hit_ptr, seg_ptr)
    return EventGraphs(batch, event_index, hit_index, layer)
