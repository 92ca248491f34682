"""Choosing `build_graphs`' arguments on the GPU: all-pair histograms of the cut quantities, and a layer census.

The reference picks `layer_pairs`, `phi_slope_max`, `phi_slope_outer_max` and `z0_max` in two notebooks,
gnn/GraphConstructionDev.ipynb and gnn/GraphConstructionDev_mu200.ipynb, in pandas:

* the layer census (GraphConstructionDev cells 16-17 and 37-41): group the hits by (evtid, barcode), sort each group
  by r and count which layer follows which -> `count_layer_transitions`, which decides `layer_pairs`;
* the all-pair histograms (GraphConstructionDev cell 20, mu200 cell 18, plotted in cells 21-25): pair every hit of
  layer l1 with every hit of layer l2, compute phi_slope and z0 of each pair, and histogram them for true and fake
  pairs -> `study_segment_cuts`;
* purity and efficiency of a cut (mu200 cells 30-33, GraphConstructionDev cells 45-48) -> `SegmentCutStudy.purity`
  and `.efficiency`.

`study_segment_cuts` takes `build_graphs`' inputs and makes the same graphs (events x phi sectors, a hit exactly on a
sector edge in no sector, phi re-centred in float32) and the same float32 pair arithmetic (`graph_build.pair_values`),
so `SegmentCutStudy.kept(cuts)` is exactly the number of segments `build_graphs` keeps with those cuts, and the
number of true ones among them.  |phi_slope| and |z0| are binned (the cuts act on absolute values,
gnn/graph.py:65): the bin of a value v is the number of edges <= v, np.searchsorted(edges, v, side="right"); bin 0 is
below the first edge, bin len(edges) at or above the last, and NaN goes there too, so a pair with r2 == r1 (inf or
NaN in both quantities) sits in the last bin of both axes and is never kept, as in the builder.

CUDA tensors run csrc/graph_build.hip (gnn_cut_study) and csrc/layer_census.hip; numpy arrays or CPU tensors run
`study_segment_cuts_numpy` and `count_layer_transitions_numpy`, the specifications.
"""
import numpy as np
import torch

from .graph_build import (GB_STATUS_EVENTS, GB_STATUS_LAYER, INNER_LAYERS, _check_inputs, _check_on_device, _host,
                          _raise_builder_status, pair_values, sector_edges)

MAX_CELLS = 4096          # csrc/graph_build.hip kMaxCells: (NS + 1) * (NZ + 1) cells per class fit the LDS table
LC_STATUS_NAN = 8         # csrc/layer_census.hip: a NaN r
_STUDY_WORDS = ((GB_STATUS_LAYER, "layer outside [0, n_layers)"), (GB_STATUS_EVENTS, "malformed event_ptr"))
_CENSUS_WORDS = _STUDY_WORDS + ((LC_STATUS_NAN, "NaN in r"),)


def _edges32(edges, name):
    """The edges of one axis, rounded to float32 once: 1-D, at least one, strictly increasing, no NaN."""
    e = np.asarray(_host(edges), dtype=np.float64)
    if e.ndim != 1 or e.size < 1:
        raise ValueError("%s must be one-dimensional with at least one edge" % name)
    with np.errstate(over="ignore"):
        e = e.astype(np.float32)
    if np.any(np.isnan(e)):
        raise ValueError("%s holds NaN" % name)
    if np.any(np.diff(e) <= 0):
        raise ValueError("%s must be strictly increasing (as float32)" % name)
    return e


class SegmentCutStudy:
    """All-pair counts of one data set: `counts` int64 [P, 2, NS + 1, NZ + 1] (axis 1: fake, true; summed over events
    and sectors; row p belongs to layer_pairs[p], repeated pairs have their own rows), `phi_slope_edges` [NS] and
    `z0_edges` [NZ] (float32 numpy arrays, the values used) and `layer_pairs` (int32 numpy [P, 2])."""

    def __init__(self, counts, phi_slope_edges, z0_edges, layer_pairs):
        self.counts = counts
        self.phi_slope_edges = phi_slope_edges
        self.z0_edges = z0_edges
        self.layer_pairs = layer_pairs

    @staticmethod
    def _edge_index(edges, cut, name):
        with np.errstate(over="ignore"):
            c = np.float32(cut)
        k = np.flatnonzero(edges == c)
        if k.size != 1:
            raise ValueError("%s = %r is not one of the edges: a cut can be counted only at an edge" % (name, cut))
        return int(k[0])

    def kept(self, phi_slope_max, z0_max, phi_slope_outer_max=None):
        """int64 [P, 2] (fake, true): the pairs with |phi_slope| < cut and |z0| < z0_max, where a pair whose first
        layer is below 5 takes phi_slope_max and the others phi_slope_outer_max (default: phi_slope_max), as
        gnn/graph.py:65 chooses; exactly what build_graphs keeps.  float32(cut) must be an edge."""
        if phi_slope_outer_max is None:
            phi_slope_outer_max = phi_slope_max
        ki = self._edge_index(self.phi_slope_edges, phi_slope_max, "phi_slope_max")
        ko = self._edge_index(self.phi_slope_edges, phi_slope_outer_max, "phi_slope_outer_max")
        kz = self._edge_index(self.z0_edges, z0_max, "z0_max")
        c = self.counts
        inner = torch.from_numpy(self.layer_pairs[:, 0] < INNER_LAYERS).to(c.device)
        # bins 0 .. k hold the values below edges[k]
        return torch.where(inner[:, None], c[:, :, :ki + 1, :kz + 1].sum(dim=(2, 3)),
                           c[:, :, :ko + 1, :kz + 1].sum(dim=(2, 3)))

    def purity(self, phi_slope_max, z0_max, phi_slope_outer_max=None):
        """True kept pairs over all kept pairs (mu200 cell 33), over all layer pairs; NaN when nothing is kept."""
        fake, true = (int(v) for v in self.kept(phi_slope_max, z0_max, phi_slope_outer_max).sum(dim=0).tolist())
        return true / (fake + true) if fake + true else float("nan")

    def efficiency(self, phi_slope_max, z0_max, phi_slope_outer_max=None):
        """True kept pairs over all true pairs of the listed layer pairs; NaN when there is no true pair."""
        true = int(self.kept(phi_slope_max, z0_max, phi_slope_outer_max)[:, 1].sum())
        n_true = int(self.counts[:, 1].sum())
        return true / n_true if n_true else float("nan")

    def marginals(self):
        """(|phi_slope| histogram int64 [P, 2, NS + 1], |z0| histogram int64 [P, 2, NZ + 1]): what cells 21-25 plot,
        per layer pair and class, on absolute values."""
        return self.counts.sum(dim=3), self.counts.sum(dim=2)

    def __add__(self, other):
        if not isinstance(other, SegmentCutStudy):
            return NotImplemented
        if not (np.array_equal(self.phi_slope_edges, other.phi_slope_edges) and
                np.array_equal(self.z0_edges, other.z0_edges) and
                np.array_equal(self.layer_pairs, other.layer_pairs)):
            raise ValueError("only studies with equal edges and layer pairs add up")
        if self.counts.device != other.counts.device:
            raise ValueError("the studies live on %s and %s" % (self.counts.device, other.counts.device))
        return SegmentCutStudy(self.counts + other.counts, self.phi_slope_edges, self.z0_edges, self.layer_pairs)


def study_segment_cuts(r, phi, z, layer, layer_pairs, particle_id, *, event_ptr=None, n_phi_sectors=1,
                       phi_slope_edges, z0_edges):
    """All-pair histograms of |phi_slope| and |z0| for true and fake pairs (see the module docstring): a
    SegmentCutStudy on the inputs' device.

    r, phi, z, layer, layer_pairs, event_ptr, n_phi_sectors: as build_graphs takes them, with the same checks;
    particle_id: integer [n], required; phi_slope_edges, z0_edges: 1-D, strictly increasing, rounded to float32
    once (the last may be +inf), at most 4096 cells (NS + 1) * (NZ + 1).
    """
    if particle_id is None:
        raise ValueError("particle_id is required: the study counts true and fake pairs")
    n, pairs, ep = _check_inputs(r, phi, z, layer, layer_pairs, particle_id, event_ptr, n_phi_sectors)
    se, ze = _edges32(phi_slope_edges, "phi_slope_edges"), _edges32(z0_edges, "z0_edges")
    if (se.size + 1) * (ze.size + 1) > MAX_CELLS:
        raise ValueError("(%d + 1) x (%d + 1) histogram cells: at most %d" % (se.size, ze.size, MAX_CELLS))
    if ep is None:
        ep = np.array([0, n], dtype=np.int64)
    S = int(n_phi_sectors)
    if torch.is_tensor(r) and r.is_cuda:
        counts = _study_device(r, phi, z, layer, pairs, particle_id, ep, S, se, ze)
    else:
        cols = [_host(c) for c in (r, phi, z, layer)]
        counts = torch.from_numpy(study_segment_cuts_numpy(*cols, pairs, _host(particle_id), ep, S, se, ze))
    return SegmentCutStudy(counts, se, ze, pairs)


def study_segment_cuts_numpy(r, phi, z, layer, pairs, particle_id, event_ptr, n_phi_sectors, slope_edges, z0_edges):
    """The specification (host arrays, validated by study_segment_cuts): counts int64 [P, 2, NS + 1, NZ + 1]."""
    r, phi, z = (np.asarray(c, dtype=np.float32) for c in (r, phi, z))
    layer, particle_id = np.asarray(layer), np.asarray(particle_id)
    if layer.size and layer.min() < 0:
        raise ValueError("negative layer id")
    edges, half = sector_edges(n_phi_sectors)
    half32 = np.float32(half)
    NS, NZ = slope_edges.shape[0], z0_edges.shape[0]
    counts = np.zeros((len(pairs), 2, NS + 1, NZ + 1), np.int64)
    for e in range(event_ptr.shape[0] - 1):
        rows = np.arange(event_ptr[e], event_ptr[e + 1])
        ph64 = phi[rows].astype(np.float64)
        for s in range(n_phi_sectors):
            h = rows[(ph64 > edges[s]) & (ph64 < edges[s + 1])]
            cphi = (phi[h] - np.float32(edges[s])) - half32
            rr, zz, lay, pid = r[h], z[h], layer[h], particle_id[h]
            for p, (l1, l2) in enumerate(pairs):
                a = np.flatnonzero(lay == l1)
                b = np.flatnonzero(lay == l2)
                if a.size == 0 or b.size == 0:      # gnn/graph.py:82-89: a layer without hits skips the pair
                    continue
                i = np.repeat(a, b.size)
                j = np.tile(b, a.size)
                slope, z0 = pair_values(rr, cphi, zz, i, j)
                bs = np.searchsorted(slope_edges, np.abs(slope), side="right")      # NaN sorts last: bin NS
                bz = np.searchsorted(z0_edges, np.abs(z0), side="right")
                y = (pid[i] == pid[j]).astype(np.int64)
                cell = (y * (NS + 1) + bs) * (NZ + 1) + bz
                counts[p] += np.bincount(cell, minlength=2 * (NS + 1) * (NZ + 1)).reshape(2, NS + 1, NZ + 1)
    return counts


def _device_layers(layer, n, floor):
    """(int32 contiguous layer, n_layers = max(largest layer, floor) + 1); a negative layer raises."""
    layer = layer.to(torch.int32).contiguous()
    hi = -1
    if n:
        lo, hi = torch.aminmax(layer)
        lo, hi = (int(v) for v in torch.stack([lo, hi]).tolist())
        if lo < 0:
            raise ValueError("negative layer id")
    return layer, max(hi, floor) + 1


def _study_device(r, phi, z, layer, pairs, particle_id, event_ptr, n_phi_sectors, se, ze):
    from . import _lib
    dev = r.device
    _check_on_device(dev, phi=phi, z=z, layer=layer, particle_id=particle_id)
    layer, n_layers = _device_layers(layer, int(r.shape[0]), int(pairs.max()) if pairs.size else -1)
    pid = particle_id.to(torch.int64).contiguous()
    ep = torch.from_numpy(event_ptr).to(dev)
    r, phi, z = (t.contiguous() for t in (r, phi, z))
    out = _lib.cut_study(r, phi, z, layer, pid, ep, pairs, n_layers, n_phi_sectors, torch.from_numpy(se).to(dev),
                         torch.from_numpy(ze).to(dev))
    _raise_builder_status("cut study", _STUDY_WORDS, int(out[-1]))
    return out[:-1].view(pairs.shape[0], 2, se.size + 1, ze.size + 1)


def count_layer_transitions(r, layer, particle_id, *, event_ptr=None, n_layers=None, skip_particle_id=None):
    """int64 [L, L] on the inputs' device: entry [a, b] is the number of times a hit on layer b directly follows a hit
    on layer a when the hits of one (event, particle) are ordered by r (gnn/GraphConstructionDev.ipynb cells 16-17
    and 37-41 with `layer` in place of (volid, layid)).  There are no sectors.

    r: float32 [n]; layer, particle_id: integer [n]; event_ptr: [n_events + 1] (default: one event); n_layers: L
    (default: the largest layer + 1); skip_particle_id: one id whose hits are left out (TrackML's 0 for noise).
    Hits of one particle with equal r are ordered by input row: the reference sorts with pandas' default quicksort,
    which leaves the order of equal keys open, so there the reference itself has no single answer.  A NaN r raises
    ValueError.
    """
    if r.dtype not in (np.float32, torch.float32) or len(r.shape) != 1:
        raise ValueError("r must be one-dimensional float32, got %s %s" % (r.dtype, tuple(r.shape)))
    n = int(r.shape[0])
    for name, c in (("layer", layer), ("particle_id", particle_id)):
        if len(c.shape) != 1 or int(c.shape[0]) != n:
            raise ValueError("%s has %s entries, r has %d" % (name, tuple(c.shape), n))
    if n >= 2 ** 31:
        raise ValueError("more than 2^31 - 1 hits")
    if event_ptr is None:
        ep = np.array([0, n], dtype=np.int64)
    else:
        ep = np.asarray(_host(event_ptr), dtype=np.int64).ravel()
        if ep.size < 2 or ep[0] != 0 or ep[-1] != n or np.any(np.diff(ep) < 0):
            raise ValueError("event_ptr must run non-decreasing from 0 to the number of hits (%d)" % n)
    if n_layers is not None and (int(n_layers) != n_layers or n_layers < 1):
        raise ValueError("n_layers must be a positive integer")
    if torch.is_tensor(r) and r.is_cuda:
        return _census_device(r, layer, particle_id, ep, n_layers, skip_particle_id)
    return torch.from_numpy(count_layer_transitions_numpy(_host(r), _host(layer), _host(particle_id), ep, n_layers,
                                                          skip_particle_id))


def count_layer_transitions_numpy(r, layer, particle_id, event_ptr, n_layers=None, skip_particle_id=None):
    """The specification (host arrays, validated by count_layer_transitions): int64 [L, L]."""
    r, layer, particle_id = np.asarray(r, dtype=np.float32), np.asarray(layer), np.asarray(particle_id)
    if np.any(np.isnan(r)):
        raise ValueError("layer census: NaN in r")
    if layer.size and layer.min() < 0:
        raise ValueError("negative layer id")
    L = int(n_layers) if n_layers is not None else (int(layer.max()) + 1 if layer.size else 1)
    if layer.size and layer.max() >= L:
        raise ValueError("layer census status %d (layer outside [0, n_layers))" % GB_STATUS_LAYER)
    table = np.zeros((L, L), np.int64)
    for e in range(event_ptr.shape[0] - 1):
        rows = np.arange(event_ptr[e], event_ptr[e + 1])
        if skip_particle_id is not None:
            rows = rows[particle_id[rows] != skip_particle_id]
        order = rows[np.lexsort((r[rows], particle_id[rows]))]     # by particle, then r; stable: ties in row order
        a, b = order[:-1], order[1:]
        same = particle_id[a] == particle_id[b]
        np.add.at(table, (layer[a][same], layer[b][same]), 1)
    return table


def _census_device(r, layer, particle_id, event_ptr, n_layers, skip_particle_id):
    from . import _lib
    dev = r.device
    _check_on_device(dev, layer=layer, particle_id=particle_id)
    layer, L = _device_layers(layer, int(r.shape[0]), 0)
    if n_layers is not None:
        L = int(n_layers)
    out = _lib.layer_census(r.contiguous(), layer, particle_id.to(torch.int64).contiguous(),
                            torch.from_numpy(event_ptr).to(dev), L, skip_particle_id)
    _raise_builder_status("layer census", _CENSUS_WORDS, int(out[-1]))
    return out[:-1].view(L, L)
