"""Batches and references the tests of the one-launch fixed-point forward share (test infrastructure, not product;
imported by test_fixed_events_host.py, test_gpu_fixed_events.py and test_gpu_fixed_events_sweeps.py)."""
import functools

import numpy as np

import fixed_point_cases as fc
from gnn_fpga_amd import HitGraph, HitGraphBatch, fixed_forward_numpy, synth


def _cut(g, F):
    """The graph with the first F of its features (the muon graphs have 11)."""
    return g if g.X.shape[1] == F else g._replace(X=np.ascontiguousarray(g.X[:, :F]))


@functools.lru_cache(maxsize=None)
def muon(n, F=11):
    return tuple(_cut(synth.muon_graph(s), F) for s in range(n))


@functools.lru_cache(maxsize=None)
def mixed600(F=11):
    """600 muon graphs (seeds 0..599) with graph 100 empty, graph 300 hits without segments and graph 500 one hit."""
    gs = list(muon(600, F))
    none = np.zeros(0, np.int32)
    gs[100] = HitGraph(np.zeros((0, F), np.float32), none, none, np.zeros(0, np.float32))
    gs[300] = HitGraph(gs[300].X, none, none, np.zeros(0, np.float32))
    gs[500] = HitGraph(gs[500].X[:1], none, none, np.zeros(0, np.float32))
    return tuple(gs)


def graphs(kind, F):
    """(graphs, pad_segments) of a named batch."""
    if kind == "muon64":
        return list(muon(64, F)), False
    if kind == "single":
        return list(muon(1, F)), False
    if kind == "toy32":
        return [_cut(synth.toy2d_graph(s), F) for s in range(32)], False
    if kind == "block3_padded":     # lists of 130 entries, more than 64 hits, hundreds of padded segments
        return [fc.layered(70, 150, F, 1), fc.layered(33, 41, F, 2), fc.cached_star(5, F)], True
    if kind == "mixed600":
        return list(mixed600(F)), False
    if kind == "mixed600_padded":   # the empty graph owns padded segments only
        return list(mixed600(F)), True
    if kind == "no_segments":
        g = fc.layered(40, 50, F, 3)
        return [HitGraph(g.X, g.src[:0], g.dst[:0], g.y[:0])] * 2, False
    raise KeyError(kind)


def host_batch(kind, F):
    gs, pad = graphs(kind, F)
    return HitGraphBatch.from_graphs(gs, pad_segments=pad)


def gained(F, D, T, gain=1.0):
    """The ten float weights of fc.default_model, every one times `gain`."""
    return [w * np.float32(gain) for w in fc.host_weights(fc.default_model(F, D, T))]


def spec(hb, weights, T, f):
    """The specification on a whole host batch."""
    return fixed_forward_numpy(hb.X.numpy(), hb.src.numpy(), hb.dst.numpy(), weights, T, f)


def spec_per_graph(hb, weights, T, f):
    """The specification run on every graph's slice alone, hit ids made local: a list of FixedPointScores."""
    X, src, dst = hb.X.numpy(), hb.src.numpy(), hb.dst.numpy()
    out = []
    for i in range(hb.n_graphs):
        h0, h1, s0, s1 = int(hb.hit_ptr[i]), int(hb.hit_ptr[i + 1]), int(hb.seg_ptr[i]), int(hb.seg_ptr[i + 1])
        s, d = src[s0:s1], dst[s0:s1]
        out.append(fixed_forward_numpy(X[h0:h1], np.where(s < 0, -1, s - h0), np.where(s < 0, -1, d - h0), weights, T, f))
    return out


def device_args(weights, f, F, D, s=lambda t: t):
    """(params, fmt, tables) as _lib.fxev_forward and _lib.fx_forward take them; `s` re-seats every device tensor."""
    import torch
    from gnn_fpga_amd import _lib
    from gnn_fpga_amd import fixed_point as fp
    q = [s(torch.from_numpy(w.astype(np.int32)).cuda()) for w in fp.quantize_weights(weights, f)]
    tabs = [s(torch.from_numpy(t.astype(np.int32)).cuda()) for t in fp.activation_tables(f)]
    return (_lib.fx_params_struct(q, F, D), _lib.fx_format_struct(*f._key()),
            _lib.fx_tables_struct(tabs[0], tabs[1], f.table_bits))
