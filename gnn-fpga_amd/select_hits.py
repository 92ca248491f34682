"""TrackML barrel hits from raw event tables: the reference's hit selection on the GPU.

Replaces `select_hits` of gnn/prepareGraphs.py:53-85, the first step of `process_event` (:136-170), which runs on the
host in pandas: ten `get_group` calls and a concat for the barrel layers, two merges (truth with particles, hits with
truth), an optional "hits every layer" filter and a groupby for the deduplication.  `select_hits` takes the three raw
tables of any number of events and returns the selected hits as a SelectedHits, whose columns are exactly what
`build_graphs` takes: `sel.build_graphs(...)` is the rest of `process_event`.

The tables are dicts of columns plus `event_ptr` (event e owns rows event_ptr[e] .. event_ptr[e+1] of its table;
absent: one event), TrackML's dtypes: hits `hit_id` int32/int64, `x, y, z` float32, `volume_id`, `layer_id` integer;
truth `hit_id`, `particle_id` integer; particles `particle_id` integer, `px, py` float32.  The three event_ptr name
the same number of events.

What it computes, exactly as the reference does on float32 columns (checked against it on pandas 2.3):

* layer: the index of (volume_id, layer_id) in `barrel_layers` (the first match); other rows are dropped (:55-62);
* pt = sqrt(px px + py py) in float32, every operation rounded on its own; a particle is kept when
  pt > float32(pt_min), strictly: a particle whose pt equals pt_min is dropped (:64-67);
* joins, both inner and per event (hit_ids restart in every TrackML event, particle ids repeat across events): a hit
  survives only if its hit_id has a truth row in its own event whose particle_id is a kept particle of its own event.
  Noise (particle id 0, absent from particles) drops out here (:68-69, :74-76);
* r = sqrt(x x + y y) in the same float32 chain (:71);
* `no_missing_hits`: a particle is kept only if its hits cover len(barrel_layers) distinct layers.  The reference
  hard-codes 10 (:80), which is the same for the default table;
* deduplication: per (event, particle_id, layer) the hit of smallest r, the lowest input row on equal r (:82-84);
* output order: within an event by particle_id ascending (signed int64), then by layer - what `.loc[idxmin]` yields.
  It decides the segment order downstream;
* particle ids and hit ids are compared as 64-bit integers throughout: ids above 2^53 that differ by 1 stay distinct.

Differences from the reference: (1) a barrel layer with no rows in an event gives no hits on that layer (the
reference raises KeyError from `get_group`); (2) a hit_id twice in an event's hits or in its truth rows, a
particle_id twice in an event's particles (the reference would multiply rows), a non-finite x or y in any row (it
would propagate NaN) and a malformed event_ptr raise ValueError: the device path flags them in its status word;
(3) phi is not recomputed bit for bit: numpy's float32 arctan2 is not correctly rounded, so no device function can
promise its bits.  `phi=None` gives atan2f(y, x) on the device (np.arctan2 on the host path), a few ulps from each
other; `phi=<float32 per input hit row>` is gathered as given; (4) under pandas 2.3 `hits.loc[<DataFrame>]` does
not run: the fixtures take the `r` column of the idxmin result, which is the deduplication above; (5) `max_tracks`
(an unseeded shuffle) and `select_phi_sector` are not provided; (6) at most 64 barrel layers.

CUDA tensors run csrc/select_hits.hip (two calls around one read-back of the sizes); numpy arrays or CPU tensors run
`select_hits_numpy`, the specification, and give a CPU result.  Known cliff on the device: one particle id shared by
very many hits of an event is one lane's serial walk.
"""
import numpy as np
import torch

from ._abi import GNN_SELECT_HITS_MAX_LAYERS as MAX_LAYERS
from .graph_build import _check_on_device, _host, _raise_builder_status, build_graphs

BARREL_VLIDS = ((8, 2), (8, 4), (8, 6), (8, 8), (13, 2), (13, 4), (13, 6), (13, 8), (17, 2), (17, 4))   # :55-57
SH_STATUS_EVENTS = 4              # csrc/select_hits.hip: an event_ptr not 0 .. its table's rows, non-decreasing
SH_STATUS_FINITE = 8              # a non-finite x or y
SH_STATUS_DUPLICATE = 16          # an id twice in one event's table
_STATUS_WORDS = ((SH_STATUS_EVENTS, "malformed event_ptr"), (SH_STATUS_FINITE, "a non-finite x or y"),
                 (SH_STATUS_DUPLICATE, "a duplicated hit_id or particle_id in an event's table"))

_HITS = ("hit_id", "x", "y", "z", "volume_id", "layer_id")
_TRUTH = ("hit_id", "particle_id")
_PARTICLES = ("particle_id", "px", "py")
_FLOATS = ("x", "y", "z", "px", "py")


def _raise_status(st):
    _raise_builder_status("hit selection", _STATUS_WORDS, st)


class SelectedHits:
    """The hits select_hits keeps, where the inputs live, event by event in (particle_id, layer) order.

    r, phi, z float32, layer int32, particle_id, hit_id int64, row int64 (the hit's row in the input hits table), one
    entry per selected hit; event_ptr: host int64 [n_events + 1], event e owns entries event_ptr[e] .. event_ptr[e+1]."""

    def __init__(self, r, phi, z, layer, particle_id, hit_id, row, event_ptr):
        self.r, self.phi, self.z, self.layer, self.particle_id = r, phi, z, layer, particle_id
        self.hit_id, self.row, self.event_ptr = hit_id, row, event_ptr

    def __len__(self):
        return int(self.r.shape[0])

    def build_graphs(self, layer_pairs=None, **cuts):
        """The rest of process_event (gnn/prepareGraphs.py:146-169): `graph_build.build_graphs` on these hits, with
        their particle ids and event_ptr.  layer_pairs defaults to the adjacent pairs of ten layers (:153-155); `cuts`
        are build_graphs' keywords (n_phi_sectors, phi_slope_max, phi_slope_outer_max, z0_max, feature_scale)."""
        if layer_pairs is None:
            l = np.arange(10)
            layer_pairs = np.stack([l[:-1], l[1:]], axis=1)
        return build_graphs(self.r, self.phi, self.z, self.layer, layer_pairs, particle_id=self.particle_id,
                            event_ptr=self.event_ptr, **cuts)


def _is_integer(c):
    if torch.is_tensor(c):
        return not c.dtype.is_floating_point and c.dtype not in (torch.bool, torch.complex64, torch.complex128)
    return np.issubdtype(c.dtype, np.integer)


def _check_table(name, table, columns):
    """The columns of one table, validated: (number of rows, event_ptr as a host int64 array)."""
    for k in columns:
        if k not in table:
            raise ValueError("%s needs a %r column" % (name, k))
        c = table[k]
        if not (torch.is_tensor(c) or isinstance(c, np.ndarray)):
            raise ValueError("%s %s must be a numpy array or a tensor" % (name, k))
        if len(c.shape) != 1:
            raise ValueError("%s %s must be one-dimensional" % (name, k))
        if k in _FLOATS:
            if c.dtype in (np.float64, torch.float64):
                raise ValueError("%s %s is float64: the reference's selection is float32 arithmetic on float32 "
                                 "columns; convert explicitly if that is what you mean" % (name, k))
            if c.dtype not in (np.float32, torch.float32):
                raise ValueError("%s %s must be float32, got %s" % (name, k, c.dtype))
        elif not _is_integer(c):
            raise ValueError("%s %s must be an integer column, got %s" % (name, k, c.dtype))
    n = int(table[columns[0]].shape[0])
    for k in columns[1:]:
        if int(table[k].shape[0]) != n:
            raise ValueError("%s %s has %d entries, %s has %d" % (name, k, int(table[k].shape[0]), columns[0], n))
    if n >= 2 ** 31 - 1:
        raise ValueError("more than 2^31 - 1 rows in %s" % name)
    if table.get("event_ptr") is None:
        return n, np.array([0, n], dtype=np.int64)
    ep = _host(table["event_ptr"], "event_ptr")
    if not np.issubdtype(ep.dtype, np.integer):
        raise ValueError("%s event_ptr must be integer" % name)
    ep = ep.astype(np.int64).ravel()
    if ep.size < 2 or ep[0] != 0 or ep[-1] != n or np.any(np.diff(ep) < 0):
        raise ValueError("%s event_ptr must run non-decreasing from 0 to its number of rows (%d)" % (name, n))
    return n, ep


def select_hits(hits, truth, particles, pt_min=0.0, no_missing_hits=False, barrel_layers=BARREL_VLIDS, phi=None):
    """The selected hits of every event (see the module docstring) as SelectedHits.

    hits, truth, particles: dicts of columns plus event_ptr; pt_min: the cut, rounded to float32; no_missing_hits:
    keep only particles with a hit on every one of len(barrel_layers) layers; barrel_layers: (volume_id, layer_id)
    pairs, the layer is the index in this list; phi: float32 per input hit row, gathered as given, or None."""
    n, hep = _check_table("hits", hits, _HITS)
    nt, tep = _check_table("truth", truth, _TRUTH)
    npart, pep = _check_table("particles", particles, _PARTICLES)
    if not (hep.shape == tep.shape == pep.shape):
        raise ValueError("the three event_ptr name %d, %d and %d events" % (hep.size - 1, tep.size - 1, pep.size - 1))
    tab = np.asarray(barrel_layers, dtype=np.int64).reshape(-1, 2) if len(barrel_layers) else np.zeros((0, 2), np.int64)
    if not 1 <= tab.shape[0] <= MAX_LAYERS:
        raise ValueError("barrel_layers needs 1 .. %d (volume, layer) pairs" % MAX_LAYERS)
    if np.abs(tab).max() >= 2 ** 31:
        raise ValueError("barrel_layers entry outside int32")
    pt_min = float(pt_min)
    if pt_min != pt_min:
        raise ValueError("pt_min is NaN")
    if phi is not None:
        if not (torch.is_tensor(phi) or isinstance(phi, np.ndarray)) or phi.dtype not in (np.float32, torch.float32):
            raise ValueError("phi must be a float32 array or tensor, one entry per hit row")
        if len(phi.shape) != 1 or int(phi.shape[0]) != n:
            raise ValueError("phi has %s entries, hits has %d rows" % (tuple(phi.shape), n))
    x = hits["x"]
    if torch.is_tensor(x) and x.is_cuda:
        return _select_device(hits, truth, particles, (hep, tep, pep), tab, pt_min, bool(no_missing_hits), phi)
    h, t, p = ({k: _host(tb[k], k) for k in cols} for tb, cols in ((hits, _HITS), (truth, _TRUTH), (particles, _PARTICLES)))
    return select_hits_numpy(h, t, p, (hep, tep, pep), pt_min, bool(no_missing_hits), tab,
                             None if phi is None else _host(phi, "phi"))


def _unique_per_event(ids, ep):
    """No id twice among an event's rows?"""
    evt = np.repeat(np.arange(ep.shape[0] - 1, dtype=np.int64), np.diff(ep))
    o = np.lexsort((ids, evt))
    e, v = evt[o], ids[o]
    return not np.any((e[1:] == e[:-1]) & (v[1:] == v[:-1]))


def select_hits_numpy(hits, truth, particles, event_ptrs, pt_min=0.0, no_missing_hits=False,
                      barrel_layers=BARREL_VLIDS, phi=None):
    """The specification (host column dicts and the three event_ptr, validated by select_hits): a CPU SelectedHits."""
    hep, tep, pep = (np.asarray(ep, dtype=np.int64) for ep in event_ptrs)
    tab = np.asarray(barrel_layers, dtype=np.int64).reshape(-1, 2)
    hid = np.asarray(hits["hit_id"]).astype(np.int64)
    x, y, z = (np.asarray(hits[k], dtype=np.float32) for k in ("x", "y", "z"))
    vol, lid = (np.asarray(hits[k]).astype(np.int64) for k in ("volume_id", "layer_id"))
    thid, tpid = (np.asarray(truth[k]).astype(np.int64) for k in _TRUTH)
    pid = np.asarray(particles["particle_id"]).astype(np.int64)
    px, py = (np.asarray(particles[k], dtype=np.float32) for k in ("px", "py"))
    if not (np.isfinite(x).all() and np.isfinite(y).all()):
        _raise_status(SH_STATUS_FINITE)
    if not (_unique_per_event(hid, hep) and _unique_per_event(thid, tep) and _unique_per_event(pid, pep)):
        _raise_status(SH_STATUS_DUPLICATE)
    layer = np.full(hid.shape[0], -1, dtype=np.int64)
    for k in range(tab.shape[0] - 1, -1, -1):                      # the first match wins
        layer[(vol == tab[k, 0]) & (lid == tab[k, 1])] = k
    with np.errstate(over="ignore", invalid="ignore"):
        pt = np.sqrt(px * px + py * py)                           # :64
        keep = pt > np.float32(pt_min)                            # :67
        r = np.sqrt(x * x + y * y)                                # :71
    assert pt.dtype == r.dtype == np.float32
    if phi is None:
        phi = np.arctan2(y, x)                                    # :72
    phi = np.asarray(phi, dtype=np.float32)
    rows_out, pids_out = [], []
    out_ptr = [0]
    for e in range(hep.shape[0] - 1):
        kept_ids = np.sort(pid[pep[e]:pep[e + 1]][keep[pep[e]:pep[e + 1]]])
        th, tp = thid[tep[e]:tep[e + 1]], tpid[tep[e]:tep[e + 1]]
        at = np.searchsorted(kept_ids, tp)
        ok = np.zeros(tp.shape[0], dtype=bool)
        inside = at < kept_ids.shape[0]
        ok[inside] = kept_ids[at[inside]] == tp[inside]           # :68-69
        o = np.argsort(th[ok], kind="stable")
        th, tp = th[ok][o], tp[ok][o]
        rows = np.arange(hep[e], hep[e + 1])
        rows = rows[layer[rows] >= 0]                             # :60-62
        at = np.searchsorted(th, hid[rows])
        inside = at < th.shape[0]
        found = np.zeros(rows.shape[0], dtype=bool)
        found[inside] = th[at[inside]] == hid[rows[inside]]       # :74-76
        rows, p_of = rows[found], tp[at[found]]
        o = np.lexsort((rows, r[rows], layer[rows], p_of))        # (particle, layer), the smallest r, the lowest row
        rows, p_of = rows[o], p_of[o]
        lay = layer[rows]
        first = np.ones(rows.shape[0], dtype=bool)
        first[1:] = (p_of[1:] != p_of[:-1]) | (lay[1:] != lay[:-1])   # :82-84
        if no_missing_hits and rows.size:                         # :77-80: a particle's groups are its layers
            new_p = np.ones(rows.shape[0], dtype=bool)
            new_p[1:] = p_of[1:] != p_of[:-1]
            seg = np.cumsum(new_p) - 1
            first &= np.bincount(seg, weights=first)[seg] == tab.shape[0]
        rows_out.append(rows[first])
        pids_out.append(p_of[first])
        out_ptr.append(out_ptr[-1] + int(first.sum()))
    rows = np.concatenate(rows_out).astype(np.int64)
    pid_out = np.concatenate(pids_out).astype(np.int64)
    t = torch.from_numpy
    return SelectedHits(t(r[rows]), t(phi[rows]), t(z[rows]), t(layer[rows].astype(np.int32)), t(pid_out),
                        t(hid[rows]), t(rows), np.asarray(out_ptr, dtype=np.int64))


def _select_device(hits, truth, particles, event_ptrs, tab, pt_min, no_missing_hits, phi):
    from . import _lib
    dev = hits["x"].device
    _check_on_device(dev, phi=phi, **{"hits " + k: hits[k] for k in _HITS}, **{"truth " + k: truth[k] for k in _TRUTH},
                     **{"particles " + k: particles[k] for k in _PARTICLES})
    i64, i32 = torch.int64, torch.int32
    hid = hits["hit_id"].to(i64).contiguous()
    x, y, z = (hits[k].contiguous() for k in ("x", "y", "z"))
    vol, lay = (hits[k].to(i32).contiguous() for k in ("volume_id", "layer_id"))
    thid, tpid = (truth[k].to(i64).contiguous() for k in _TRUTH)
    pid = particles["particle_id"].to(i64).contiguous()
    px, py = (particles[k].contiguous() for k in ("px", "py"))
    E = event_ptrs[0].shape[0] - 1
    eps = torch.from_numpy(np.concatenate(event_ptrs)).to(dev)         # one upload
    eps = tuple(eps[k * (E + 1):(k + 1) * (E + 1)] for k in range(3))
    ws, sizes, out_ptr = _lib.select_hits_sizes((hid, x, y, vol, lay), (thid, tpid), (pid, px, py), eps, tab, pt_min,
                                                no_missing_hits)
    _raise_status(int(sizes.status))
    if phi is not None:
        phi = phi.contiguous()
    cols = _lib.select_hits_fill(ws, sizes, hid, x, y, z, phi, int(thid.shape[0]), int(pid.shape[0]), E,
                                 no_missing_hits)
    return SelectedHits(*cols, out_ptr)
