"""Small layered graphs with prescribed degrees, for the list sweeps' last step group.

The fused kernels walk a 16-hit slice's neighbour list in groups of 4 steps; the wide kernels gather and score only
the real steps of the last group (`n` = 1 .. 4, csrc/sell_pipeline.hip: sweep_w), k_iter2 scores it whole (sweep16).
A graph from here has 4 layers of 48 hits (3 slices per level) and segments between consecutive layers only, with
degrees chosen so that the slice lengths of BOTH lists of the host plan take every residue mod 4, include 1, 4, 5
and 8, reach 27 (longer than the 24 steps k_iter2 prefetches) and 0 (a level without incoming / outgoing segments,
and one such hit inside a level that has them).
tests/test_trim_host.py asserts exactly that on the plan; tests/test_gpu_trimmed_sweeps.py runs the kernels on it."""
import numpy as np

from gnn_fpga_amd.synth import HitGraph

LAYERS, PER_LAYER = 4, 48

# out-degrees of layer l and in-degrees of layer l + 1, hit by hit (equal sums per layer pair)
_OUT = [
    [8] * 16 + [4] * 16 + [2] * 16,                               # layer 0 (no incoming segments at all)
    [6] * 16 + [27] + [7] * 15 + [2] * 14 + [0] + [2],            # layer 1: one hit with 27, one with none
    [8] * 16 + [5] * 16 + [1] * 16,                               # layer 2
]
_IN = [
    [27] + [5] * 15 + [4] * 16 + [4] * 13 + [3] * 2 + [0],        # layer 1: one hit with 27, the last one with none
    [9] * 16 + [6] * 16 + [1] * 15 + [3],                         # layer 2
    [8] * 16 + [5] * 16 + [1] * 16,                               # layer 3 (no outgoing segments at all)
]


def _pair(out_deg, in_deg):
    """Segments (i, j) with the given degrees and no pair twice: every start hit, heaviest first, takes the end hits
    with the most stubs left."""
    out_deg, left = np.asarray(out_deg), np.asarray(in_deg).copy()
    assert out_deg.sum() == left.sum()
    s, d = [], []
    for i in np.argsort(-out_deg, kind="stable"):
        k = int(out_deg[i])
        if k == 0:
            continue
        js = np.argsort(-left, kind="stable")[:k]
        assert (left[js] > 0).all(), "degrees are not realisable without a double segment"
        left[js] -= 1
        s += [int(i)] * k
        d += js.tolist()
    assert not left.any()
    return np.asarray(s, np.int64), np.asarray(d, np.int64)


def trim_graph(n_features=3, seed=0):
    """One such graph; `seed` only moves the features and the order of the segments."""
    rng = np.random.default_rng(1000 + seed)
    n = LAYERS * PER_LAYER
    X = rng.uniform(-1.0, 1.0, size=(n, n_features)).astype(np.float32)
    src, dst = [], []
    for l in range(LAYERS - 1):
        s, d = _pair(_OUT[l], _IN[l])
        src.append(s + l * PER_LAYER)
        dst.append(d + (l + 1) * PER_LAYER)
    src, dst = np.concatenate(src), np.concatenate(dst)
    order = np.argsort(rng.random(src.shape[0]) + src // PER_LAYER, kind="stable")    # shuffled inside a layer pair
    src, dst = src[order].astype(np.int32), dst[order].astype(np.int32)
    return HitGraph(X, src, dst, rng.integers(0, 2, size=src.shape[0]).astype(np.float32))


def trim_graphs(n_graphs, n_features=3):
    return [trim_graph(n_features, seed=i) for i in range(n_graphs)]


def slice_steps(plan):
    """(in, out) list steps of every slice of a SellPlan: what the sweeps take as `len`."""
    off_in, off_out = plan.in_off.cpu().numpy().astype(np.int64), plan.out_off.cpu().numpy().astype(np.int64)
    return np.diff(off_in) // 16, np.diff(off_out) // 16


def visit_ratios(plan):
    """Record visits of the two sweeps per real record (a segment is one record in each list), with every list
    rounded up to whole groups of 4 steps and at the slice's own step count: ((in, out, both) rounded, same exact)."""
    si, so = slice_steps(plan)
    real = float((plan.src_abs < plan.n_pad).sum())                # (padded segments point at the NULL hit)
    rounded = np.array([((si + 3) // 4 * 4).sum() * 16, ((so + 3) // 4 * 4).sum() * 16], dtype=np.float64)
    exact = np.array([si.sum() * 16, so.sum() * 16], dtype=np.float64)
    both = lambda v: (v[0] / real, v[1] / real, v.sum() / (2 * real))
    return both(rounded), both(exact)
