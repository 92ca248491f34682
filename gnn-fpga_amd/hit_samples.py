"""The hit classifier's track samples from detector hits: the reference's sample preparation on the GPU.

Replaces gnn/MPNN_HitClassifier.ipynb cells 5 and 9-15, which build the samples on the host in pandas: the
deduplication at the end of `select_hits` (cell 5), `select_signal_hits` (cells 5 and 10), the signal keys (cell
11), cells 12 and 14 (constants, arrays) and the per-sample loop of cell 15.  `build_hit_samples` returns every
sample of every event; the barrel volume selection and the layer renumbering of `select_hits` stay with the caller
(column arithmetic: `layer` is taken as build_graphs takes it).

What it computes, exactly as the reference does for float32 hit columns (L = n_det_layers, K = n_layer_hits):

* deduplication: per (event, particle_id, layer) the hit of smallest r is kept (idxmin: the first row on ties);
  only kept hits exist below;
* event selection: an event is dropped when a layer present in it has <= K kept hits (a layer without hits is not
  counted); every distinct particle_id is a particle, negative ids and 0 included (noise sharing one id on all L
  layers is a track, as in the reference);
* samples: the (event, particle_id) pairs whose kept hits cover exactly the L layers, in ascending
  (event, particle_id) order;
* candidates, for sample s and layer j: every kept hit of the event on layer j gets, in float32,
  deta = lay_eta - f32(trk_eta), dphi = lay_phi - trk_phi (minus f32(2 pi) if > f32(pi), then plus f32(2 pi) if
  < -f32(pi)), d = sqrt(deta * deta + dphi * dphi), where lay_eta = -1 * log(tan(arctan2(r, z) / 2)) in float32
  (numpy's float32 ufuncs) and trk_eta is the same chain in float64 on the track's hit (cell 15 takes it from an
  iloc row of a mixed-dtype frame), rounded to float32 by the subtraction; the K smallest d in ascending order,
  layer-major: L * K hits per sample;
* X = [r, phi_c, z] / feature_scale as float32(float64(v) / scale) and a fourth column, phi_c = the candidate's
  phi minus the phi of the track's layer-0 hit, wrapped as above; the fourth column is the label on layers
  < n_seed_layers and 0 elsewhere; y = float32(candidate particle == sample particle);
* segments: every adjacent-layer pair (a, b) of the candidate layout in np.where order, src = a (inner, Ro),
  dst = b (outer, Ri): the same K^2 (L - 1) segments for every sample (synth.hit_classifier_samples' src / dst),
  offset by L * K per sample.

Differences from the reference: (1) on exactly equal d the earlier input row comes first (the reference's
`sort_values()` is not stable, so its order there is not defined); (2) a layer outside [0, L), a non-finite r, phi
or z, a malformed event_ptr and more than 2^31 - 1 sample hits or segments raise ValueError (the device builder
flags them in its status word); (3) cell 10 calls select_signal_hits with its own defaults (5, 10): here the
event and track selections always use n_layer_hits and n_det_layers; (4) no samples give an empty result.  Under
pandas 2.3.3 cell 5 does not run as written (`hits.loc[<DataFrame>]`); the fixtures take the `r` column of the
idxmin result, which is the deduplication above.

The device's atan2f / tanf / logf and their double versions are not bit-identical to numpy's, so on inputs with
near-ties (candidates whose d differ by a few ulps) the device may order them differently from this
specification; every other value is exact.

CUDA tensors run csrc/hit_samples.hip (two calls around one read-back of the sizes); numpy arrays or CPU tensors run
`build_hit_samples_numpy`, the specification, and give a CPU result.
"""
import numpy as np
import torch

from .graph_build import _check_inputs, _check_on_device, _host, _raise_builder_status, wrap_dphi32
from .hitgraph import HitGraphBatch

MAX_LAYER_HITS = 16       # csrc/hit_samples.hip: the top-K list is unrolled per K
MAX_DET_LAYERS = 64       # the layer is 6 bits of a sort key
HS_STATUS_LAYER = 1       # a layer outside [0, n_det_layers)
HS_STATUS_INT32 = 2       # more than 2^31 - 1 sample hits or segments
HS_STATUS_EVENTS = 4      # event_ptr not 0 .. n_hits, non-decreasing
HS_STATUS_FINITE = 8      # a non-finite r, phi or z
_STATUS_WORDS = ((HS_STATUS_LAYER, "layer outside [0, n_det_layers)"),
                 (HS_STATUS_INT32, "more than 2^31 - 1 sample hits or segments"),
                 (HS_STATUS_EVENTS, "malformed event_ptr"), (HS_STATUS_FINITE, "a non-finite r, phi or z"))

_NAN_KEY = np.uint32(0x7FC00000)


def segment_pattern(n_det_layers, n_layer_hits):
    """Cell 15's adj_idx for the fixed candidate layout: (src, dst) int32 [K^2 (L - 1)] within one sample."""
    layers = np.repeat(np.arange(n_det_layers), n_layer_hits)
    adj = np.stack(np.where((layers[None, :] - layers[:, None]) == 1), axis=1)
    return adj[:, 0].astype(np.int32), adj[:, 1].astype(np.int32)


def calc_dphi32(phi1, phi2):
    """Cell 9 calc_dphi on float32: phi2 - phi1 wrapped against float32(pi)."""
    return wrap_dphi32(phi2 - phi1)


def eta32(r, z):
    """Cell 9 calc_eta on float32 columns (numpy's float32 ufuncs)."""
    e = np.float32(-1.0) * np.log(np.tan(np.arctan2(r, z) / np.float32(2.0)))
    assert e.dtype == np.float32
    return e


def eta64(r, z):
    """Cell 9 calc_eta on the track hit: float64."""
    return -1.0 * np.log(np.tan(np.arctan2(np.float64(r), np.float64(z)) / 2.0))


def distance_keys(d):
    """An order-preserving uint32 key of d >= 0 (every NaN one key above +inf)."""
    k = np.asarray(d, np.float32).view(np.uint32).copy()
    k[np.isnan(d)] = _NAN_KEY
    return k


class HitSamples:
    """The samples of build_hit_samples, where the input lives.

    batch: HitGraphBatch of all samples (index form, hit_ptr / seg_ptr per sample, no segment labels); y float32
    [n_samples * L * K] hit labels; keys int64 [n_samples, 2] (event index, particle_id); hit_index int64 [n_samples
    * L * K] the input row of every sample hit."""

    def __init__(self, X, y, hit_index, keys, src, dst, n_det_layers, n_layer_hits):
        self.n_det_layers, self.n_layer_hits = int(n_det_layers), int(n_layer_hits)
        self.hits_per_sample = self.n_det_layers * self.n_layer_hits
        self.segments_per_sample = self.n_layer_hits ** 2 * (self.n_det_layers - 1)
        self.n_samples = int(keys.shape[0])
        self.y, self.keys, self.hit_index = y, keys, hit_index
        S, NH, NE = self.n_samples, self.hits_per_sample, self.segments_per_sample
        self.batch = HitGraphBatch._from_device_arrays(X, src, dst, None, np.arange(S + 1) * NH, np.arange(S + 1) * NE)

    def __len__(self):
        return self.n_samples

    def batch_of(self, j, batch_size):
        """(HitGraphBatch, y) of samples j .. j + batch_size (cut at the end), sliced where they live."""
        j0, j1 = int(j), min(int(j) + int(batch_size), self.n_samples)
        if not 0 <= j0 < j1:
            raise IndexError("no samples in %d .. %d of %d" % (j, j + batch_size, self.n_samples))
        NH, NE = self.hits_per_sample, self.segments_per_sample
        b = self.batch
        off = j0 * NH
        X = b.X[j0 * NH:j1 * NH]
        src = b.src[j0 * NE:j1 * NE] - off
        dst = b.dst[j0 * NE:j1 * NE] - off
        n = j1 - j0
        return (HitGraphBatch._from_device_arrays(X, src, dst, None, np.arange(n + 1) * NH, np.arange(n + 1) * NE),
                self.y[j0 * NH:j1 * NH])

    def dense(self):
        """Cell 14's arrays: X float32 [n, L K, 4], Ri / Ro uint8 [n, L K, K^2 (L-1)], y uint8 [n, L K] (host)."""
        S, NH, NE = self.n_samples, self.hits_per_sample, self.segments_per_sample
        X = self.batch.X.detach().cpu().numpy().reshape(S, NH, 4)
        y = self.y.detach().cpu().numpy().reshape(S, NH).astype(np.uint8)
        src, dst = segment_pattern(self.n_det_layers, self.n_layer_hits)
        Ri = np.zeros((S, NH, NE), dtype=np.uint8)
        Ro = np.zeros((S, NH, NE), dtype=np.uint8)
        e = np.arange(NE)
        Ri[:, dst, e] = 1
        Ro[:, src, e] = 1
        return X, Ri, Ro, y


def _check_sample_args(n_det_layers, n_layer_hits, n_seed_layers, feature_scale):
    for name, v, hi in (("n_det_layers", n_det_layers, MAX_DET_LAYERS), ("n_layer_hits", n_layer_hits, MAX_LAYER_HITS)):
        if int(v) != v or not 1 <= v <= hi:
            raise ValueError("%s must be an integer in [1, %d], got %r" % (name, hi, v))
    if int(n_seed_layers) != n_seed_layers or n_seed_layers < 0:
        raise ValueError("n_seed_layers must be a non-negative integer")
    scale = tuple(float(s) for s in np.asarray(feature_scale, dtype=np.float64).ravel())
    if len(scale) != 3:
        raise ValueError("feature_scale needs one value per feature (r, phi, z)")
    if not all(s != 0.0 for s in scale):
        raise ValueError("a feature scale is zero or NaN")
    return int(n_det_layers), int(n_layer_hits), int(n_seed_layers), scale


def build_hit_samples(r, phi, z, layer, particle_id, event_ptr=None, n_det_layers=10, n_layer_hits=5,
                      n_seed_layers=3, feature_scale=(1000.0, np.pi, 1000.0)):
    """Every track sample of every event (see the module docstring) as HitSamples.

    r, phi, z: float32 [n]; layer: integer [n] in [0, n_det_layers); particle_id: integer [n]; event_ptr:
    [n_events + 1], event e owns rows event_ptr[e] .. event_ptr[e+1] (default: one event).  n_det_layers <= 64,
    n_layer_hits <= 16."""
    if particle_id is None:
        raise ValueError("particle_id is required: the samples are the particles' tracks")
    n, _, ep = _check_inputs(r, phi, z, layer, [], particle_id, event_ptr, 1)
    L, K, NS, scale = _check_sample_args(n_det_layers, n_layer_hits, n_seed_layers, feature_scale)
    if ep is None:
        ep = np.array([0, n], dtype=np.int64)
    if torch.is_tensor(r) and r.is_cuda:
        return _build_device(r, phi, z, layer, particle_id, ep, L, K, NS, scale)
    cols = [_host(c, k) for c, k in ((r, "r"), (phi, "phi"), (z, "z"), (layer, "layer"), (particle_id, "pid"))]
    return build_hit_samples_numpy(*cols, ep, L, K, NS, scale)


def build_hit_samples_numpy(r, phi, z, layer, particle_id, event_ptr, n_det_layers, n_layer_hits, n_seed_layers,
                            feature_scale):
    """The specification (host arrays, validated by build_hit_samples): a CPU HitSamples."""
    L, K = int(n_det_layers), int(n_layer_hits)
    r, phi, z = (np.asarray(c, dtype=np.float32) for c in (r, phi, z))
    layer = np.asarray(layer).astype(np.int64)
    pid = np.asarray(particle_id).astype(np.int64)
    ep = np.asarray(event_ptr, dtype=np.int64)
    n, E = r.shape[0], ep.shape[0] - 1
    if n and (layer.min() < 0 or layer.max() >= L):
        _raise_builder_status("hit-sample", _STATUS_WORDS, HS_STATUS_LAYER)
    if not (np.isfinite(r).all() and np.isfinite(phi).all() and np.isfinite(z).all()):
        _raise_builder_status("hit-sample", _STATUS_WORDS, HS_STATUS_FINITE)
    NH, NE = L * K, K * K * (L - 1)
    evt = np.repeat(np.arange(E, dtype=np.int64), np.diff(ep))
    rows = np.arange(n, dtype=np.int64)
    # cell 5: the hit of smallest r per (event, particle, layer), the first row on ties
    order = np.lexsort((rows, r, layer, pid, evt))
    ke, kp, kl = evt[order], pid[order], layer[order]
    first = np.ones(n, dtype=bool)
    first[1:] = (ke[1:] != ke[:-1]) | (kp[1:] != kp[:-1]) | (kl[1:] != kl[:-1])
    kept = order[first]                                   # (event, particle, layer) order
    # cells 5 and 10: events with more than K kept hits on every present layer; tracks on all L layers
    cnt = np.zeros((E, L), dtype=np.int64)
    np.add.at(cnt, (evt[kept], layer[kept]), 1)
    ok = np.all((cnt == 0) | (cnt > K), axis=1)
    ge, gp = evt[kept], pid[kept]
    start = np.ones(kept.shape[0], dtype=bool)
    start[1:] = (ge[1:] != ge[:-1]) | (gp[1:] != gp[:-1])
    gs = np.flatnonzero(start)
    glen = np.diff(np.append(gs, kept.shape[0]))
    is_s = (glen == L) & ok[ge[gs]] if gs.size else np.zeros(0, bool)
    trk = np.stack([kept[gs[is_s] + l] for l in range(L)], axis=1) if is_s.any() else np.zeros((0, L), np.int64)
    S = trk.shape[0]
    if S * NH >= 2 ** 31 or S * NE >= 2 ** 31:
        _raise_builder_status("hit-sample", _STATUS_WORDS, HS_STATUS_INT32)
    keys = np.stack([evt[trk[:, 0]], pid[trk[:, 0]]], axis=1) if S else np.zeros((0, 2), np.int64)
    # cells 9 and 15: the K nearest kept hits per (sample, layer)
    cand = np.zeros((S, L, K), dtype=np.int64)
    keep_mask = np.zeros(n, dtype=bool)
    keep_mask[kept] = True
    leta = np.zeros(n, dtype=np.float32)
    leta[keep_mask] = eta32(r[keep_mask], z[keep_mask])
    for e in np.unique(keys[:, 0]) if S else ():
        smp = np.flatnonzero(keys[:, 0] == e)
        in_e = keep_mask & (evt == e)
        for l in range(L):
            h = np.flatnonzero(in_e & (layer == l))           # frame order
            t = trk[smp, l]
            teta = np.array([eta64(r[i], z[i]) for i in t], dtype=np.float64).astype(np.float32)
            deta = leta[h][None, :] - teta[:, None]
            dphi = calc_dphi32(phi[t][:, None], phi[h][None, :])
            d = np.sqrt(deta * deta + dphi * dphi)
            assert d.dtype == np.float32
            sel = np.argsort(distance_keys(d), axis=1, kind="stable")[:, :K]
            cand[smp, l] = h[sel]
    hit_index = cand.reshape(-1)
    phi0 = np.repeat(phi[trk[:, 0]], NH) if S else np.zeros(0, np.float32)
    phic = calc_dphi32(phi0, phi[hit_index])
    X = np.zeros((S * NH, 4), dtype=np.float32)
    X[:, :3] = (np.stack([r[hit_index], phic, z[hit_index]], axis=1).astype(np.float64)
                / np.asarray(feature_scale, np.float64)).astype(np.float32)
    y = (pid[hit_index] == np.repeat(keys[:, 1], NH)).astype(np.float32)
    seed = np.tile(np.repeat(np.arange(L) < n_seed_layers, K), S)
    X[:, 3] = np.where(seed, y, np.float32(0))
    src0, dst0 = segment_pattern(L, K)
    off = (np.arange(S, dtype=np.int64) * NH)[:, None]
    src = (src0[None, :] + off).reshape(-1).astype(np.int32)
    dst = (dst0[None, :] + off).reshape(-1).astype(np.int32)
    return HitSamples(torch.from_numpy(X), torch.from_numpy(y), torch.from_numpy(hit_index), torch.from_numpy(keys),
                      torch.from_numpy(src), torch.from_numpy(dst), L, K)


def _build_device(r, phi, z, layer, particle_id, event_ptr, L, K, n_seed, feature_scale):
    from . import _lib
    _check_on_device(r.device, phi=phi, z=z, layer=layer, particle_id=particle_id)
    layer = layer.to(torch.int32).contiguous()
    pid = particle_id.to(torch.int64).contiguous()
    ep = torch.from_numpy(event_ptr).to(r.device)
    r, phi, z = (t.contiguous() for t in (r, phi, z))
    E = int(event_ptr.shape[0]) - 1
    ws, sizes = _lib.hit_samples_sizes(r, phi, z, layer, pid, ep, L, K)
    _raise_builder_status("hit-sample builder", _STATUS_WORDS, sizes.status)
    X, y, hit_index, src, dst, keys = _lib.hit_samples_fill(ws, sizes, r, phi, z, pid, E, L, K, n_seed,
                                                            feature_scale)
    return HitSamples(X, y, hit_index, keys, src, dst, L, K)
