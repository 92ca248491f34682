"""Layered graphs whose per-hit list lengths are drawn from a prescribed set, for the list sweeps of k_iter2 that
score one list step per lane (csrc/sell_pipeline.hip: sweep16_lane).

A quad of lanes walks a hit's list 8 steps at a time (four packed words, two steps each), in two groups of 4;
lane q of the quad takes step 4g + q.  The lengths {0, 1, 3, 4, 5, 7, 8, 9, 23, 24, 25, 33} put the last
real step in either half of a word and in either group, end a list exactly at a group and at a word, leave one step
for a new group and a new word, reach the last of the 24 prefetched steps and the streamed words behind them, and
0 is a hit without a list.  Hits of one 16-hit slice mix the lengths, so lanes of a slice run past their own list's
end into the NULL record at different steps.
tests/test_lane_sweep_host.py asserts that on the graphs and the plan; tests/test_gpu_lane_sweeps.py runs the kernels."""
import numpy as np

from gnn_fpga_amd.synth import HitGraph

import trim_graphs

LENGTHS = (0, 1, 3, 4, 5, 7, 8, 9, 23, 24, 25, 33)
LAYERS, PER_LAYER = 10, 256                     # 2560 hits: two 1280-hit tiles' worth, 16 slices per layer
N_GRAPHS = 3


def _degrees(rng, total=None):
    """PER_LAYER degrees from LENGTHS, every value at least 8 times and 0 exactly 8 times; with `total`, degrees that
    add up to it (hits are moved to the neighbouring value of LENGTHS one at a time: the set has steps of 1, so the
    sum is met)."""
    fixed = np.repeat(LENGTHS, 8)
    free = rng.choice(LENGTHS[1:], size=PER_LAYER - fixed.size)
    if total is not None:
        for _ in range(100000):
            diff = total - int(fixed.sum() + free.sum())
            if diff == 0:
                break
            i = rng.integers(free.size)
            k = LENGTHS.index(int(free[i])) + (1 if diff > 0 else -1)
            if 1 <= k < len(LENGTHS) and abs(LENGTHS[k] - free[i]) <= abs(diff):
                free[i] = LENGTHS[k]
        assert fixed.sum() + free.sum() == total
    deg = np.concatenate([fixed, free])
    rng.shuffle(deg)
    return deg


def lane_graph(n_features=3, seed=0):
    """One such graph: segments between consecutive layers only, no segment twice; `seed` moves degrees, features
    and the order of the segments.  The 8 hits of an inner layer without incoming segments are the 8 without
    outgoing ones: a hit that starts a path in the middle of the graph would take the plan's level 0 and stretch
    its tile's record windows past what k_iter2 holds in LDS.  Lists of length 0 beside real ones are the first
    layer's in-lists and the last layer's out-lists."""
    rng = np.random.default_rng(7000 + seed)
    n = LAYERS * PER_LAYER
    X = rng.uniform(-1.0, 1.0, size=(n, n_features)).astype(np.float32)
    src, dst = [], []
    in_deg = None
    for l in range(LAYERS - 1):
        out_deg = _degrees(rng)
        if in_deg is not None:                              # this layer's in-degrees, from the pair before
            aligned = np.zeros_like(out_deg)
            aligned[in_deg > 0] = out_deg[out_deg > 0]
            out_deg = aligned
        in_deg = _degrees(rng, int(out_deg.sum()))
        s, d = trim_graphs._pair(out_deg, in_deg)
        src.append(s + l * PER_LAYER)
        dst.append(d + (l + 1) * PER_LAYER)
    src, dst = np.concatenate(src), np.concatenate(dst)
    order = np.argsort(rng.random(src.shape[0]) + src // PER_LAYER, kind="stable")    # shuffled inside a layer pair
    src, dst = src[order].astype(np.int32), dst[order].astype(np.int32)
    return HitGraph(X, src, dst, rng.integers(0, 2, size=src.shape[0]).astype(np.float32))


_cache = {}


def lane_graphs(n_features=3):
    """The N_GRAPHS graphs of the tests for `n_features` (built once per process)."""
    if n_features not in _cache:
        _cache[n_features] = [lane_graph(n_features, seed=i) for i in range(N_GRAPHS)]
    return _cache[n_features]
