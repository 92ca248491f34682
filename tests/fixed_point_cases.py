"""Graphs, weights and references the fixed-point tests share (test infrastructure, not product; imported by
test_fixed_point_host.py, test_gpu_fixed_point.py and test_gpu_fixed_point_sweeps.py)."""
import functools

import numpy as np
import torch

from gnn_fpga_amd import FixedPointFormat, HitGraph, fixed_forward_numpy, synth


def star_graph(seed=0, n_features=3):
    """140 hits, 306 segments: hit 0 ends 130 segments and starts 130 (lists longer than a wave), 40 random segments
    among hits 1 .. 135, 6 padded ones, hits 136 .. 139 of degree 0; the segment order is shuffled."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.0, 1.0, size=(140, n_features)).astype(np.float32)
    spokes = np.arange(1, 131)
    a, b = rng.integers(1, 136, size=40), rng.integers(1, 136, size=40)
    b = np.where(a == b, (b % 135) + 1, b)
    src = np.concatenate([spokes, np.zeros(130, np.int64), a, -np.ones(6, np.int64)])
    dst = np.concatenate([np.zeros(130, np.int64), spokes, b, -np.ones(6, np.int64)])
    order = rng.permutation(src.size)
    y = (rng.random(src.size) < 0.4).astype(np.float32)
    return HitGraph(X, src[order].astype(np.int32), dst[order].astype(np.int32), y)


def default_model(F, D, T, seed=0):
    """A SegmentClassifier with torch's default initialisation under manual_seed(seed), on the host."""
    from gnn_fpga_amd.model import SegmentClassifier
    torch.manual_seed(seed)
    return SegmentClassifier(input_dim=F, hidden_dim=D, n_iters=T).eval()


def host_weights(model):
    """The ten effective tensors of a model as float32 numpy arrays (state_dict order)."""
    return [w.detach().cpu().numpy() for w in model.effective_weights()]


def fmt(W, I, rounding="trn", overflow="wrap", tb=10):
    return FixedPointFormat(W, I, rounding, overflow, tb)


def spec(graph, weights, T, f):
    return fixed_forward_numpy(graph.X, graph.src, graph.dst, weights, T, f)


@functools.lru_cache(maxsize=None)
def layered(n_hits=70, n_segments=150, F=3, seed=1):
    return synth.layered_graph(n_hits, n_segments, F, seed=seed)


@functools.lru_cache(maxsize=None)
def cached_star(seed=0, F=3):
    return star_graph(seed, F)
