"""What the batch-assembly tests on the host and on the GPU share: the two tiny datasets, a restatement of the
reference's batch rule (gnn/trainSegmentClassifier.py:66-111) in plain Python loops over graphs and segments -
nothing of batcher.py or hitgraph.py runs in it - and the array-for-array comparison of an assembled batch with it.

The rule: a batch is `graphs[j:j + batch_size]` in list order, features float32.  `padded`: every graph's segments go
into its row of [B, E_max], the free columns are src = dst = -1 with label 0, hits are never padded and dense_shape =
(B, N_max, E_max).  `flat`: plain concatenation.  A graph's own padded segments stay -1, and any pair of negative
endpoints becomes (-1, -1).
"""
import collections

import numpy as np
import torch

from gnn_fpga_amd import synth
from gnn_fpga_amd.hitgraph import _csr_by

Assembled = collections.namedtuple("Assembled", ["X", "src", "dst", "y", "hit_ptr", "seg_ptr", "dense_shape"])
LAYOUTS = ("padded", "flat")


def _ragged():
    gs = [synth.layered_graph(n, e, 3, n_layers=2, seed=s)
          for s, (n, e) in enumerate([(5, 9), (40, 0), (2, 1), (33, 80), (7, 7)])]
    big, small = gs[3], gs[0]
    at = (31, 47)                                      # two padded segments of the graph's own, in the middle
    ins = lambda a, v: np.insert(a, at, v).astype(a.dtype)      # noqa: E731
    gs.append(synth.HitGraph(big.X.copy(), ins(big.src, -1), ins(big.dst, -1), ins(big.y, 0.0)))
    src, dst = small.src.copy(), small.dst.copy()
    src[4], dst[4] = -2, -7                            # a negative pair that is not (-1, -1)
    gs.append(synth.HitGraph(small.X.copy(), src, dst, small.y.copy()))
    return gs


RAGGED = _ragged()                                     # F = 3; (hits, segments) 5/9 40/0 2/1 33/80 7/7 33/82 5/9
MUON = [synth.muon_graph(s) for s in range(6)]         # F = 11: the one-launch kernels' graphs


def windows(n_samples, batch_size):
    """The batch starts of one epoch: 0, batch_size, ... < n_samples (trainSegmentClassifier.py:99)."""
    out, j = [], 0
    while j < n_samples:
        out.append(j)
        j += batch_size
    return out


def assemble(graphs, j, batch_size, layout="padded"):
    """The batch of graphs[j:j + batch_size], restated: one loop over the graphs, one over each graph's segments."""
    assert layout in LAYOUTS
    members = list(graphs[j:j + batch_size])
    B = len(members)
    n_feat = int(np.asarray(graphs[0].X).shape[1])
    e_max = n_max = 0
    for g in members:
        e_max = max(e_max, len(g.src))
        n_max = max(n_max, len(g.X))
    rows, src, dst, y = [], [], [], []
    hit_ptr, seg_ptr = [0], [0]
    for g in members:
        first_hit = len(rows)
        for row in np.asarray(g.X):
            rows.append([np.float32(v) for v in row])
        for k in range(len(g.src)):
            a, b = int(g.src[k]), int(g.dst[k])
            if a < 0 and b < 0:
                a = b = -1
            else:
                assert 0 <= a < len(g.X) and 0 <= b < len(g.X), "the datasets hold well-formed graphs only"
                a, b = a + first_hit, b + first_hit
            src.append(a)
            dst.append(b)
            y.append(np.float32(g.y[k]))
        if layout == "padded":
            for _ in range(e_max - len(g.src)):
                src.append(-1)
                dst.append(-1)
                y.append(np.float32(0.0))
        hit_ptr.append(len(rows))
        seg_ptr.append(len(src))
    X = np.zeros((len(rows), n_feat), dtype=np.float32)
    for r, row in enumerate(rows):
        for c, v in enumerate(row):
            X[r, c] = v
    return Assembled(X, np.asarray(src, dtype=np.int32).reshape(-1), np.asarray(dst, dtype=np.int32).reshape(-1),
                     np.asarray(y, dtype=np.float32).reshape(-1), np.asarray(hit_ptr, dtype=np.int64),
                     np.asarray(seg_ptr, dtype=np.int64), (B, n_max, e_max) if layout == "padded" else None)


def _same_bits(got, want, dtype, what):
    assert torch.is_tensor(got) and got.dtype == dtype, (what, getattr(got, "dtype", type(got)))
    assert tuple(got.shape) == want.shape, (what, tuple(got.shape), want.shape)
    g = got.detach().cpu().contiguous().numpy()
    assert np.array_equal(g.view(np.int32), np.ascontiguousarray(want).view(np.int32)), what


def assert_batch_equal(got, want, device=None):
    """got: (HitGraphBatch, y) as every assembly path returns it; want: `assemble`'s Assembled.  dtype, shape and bits
    of X / src / dst / y, both pointers, dense_shape, the three counts, and the six arrays of `_ensure_csr()` against
    `hitgraph._csr_by` on the restated endpoints (a list built on the GPU keeps all n_segments entries: the list, then
    -1).  `device`: where every tensor has to live (None: wherever they are)."""
    batch, y = got
    _same_bits(batch.X, want.X, torch.float32, "X")
    _same_bits(batch.src, want.src, torch.int32, "src")
    _same_bits(batch.dst, want.dst, torch.int32, "dst")
    _same_bits(batch.y, want.y, torch.float32, "batch.y")
    y_shape = want.y.shape if want.dense_shape is None else (want.dense_shape[0], want.dense_shape[2])
    _same_bits(y, want.y.reshape(y_shape), torch.float32, "y")
    for k in ("hit_ptr", "seg_ptr"):
        p = np.asarray(getattr(batch, k))
        assert p.dtype == np.int64 and np.array_equal(p, getattr(want, k)), (k, p, getattr(want, k))
    assert batch.dense_shape == want.dense_shape, (batch.dense_shape, want.dense_shape)
    assert type(batch.n_graphs) is int and type(batch.n_hits) is int and type(batch.n_segments) is int
    assert (batch.n_graphs, batch.n_hits, batch.n_segments) == (len(want.hit_ptr) - 1, len(want.X), len(want.src))
    assert batch.n_features == want.X.shape[1]
    n, E = len(want.X), len(want.src)
    lists = _csr_by(want.dst, want.src, n) + _csr_by(want.src, want.dst, n)
    csr = batch._ensure_csr()
    assert len(csr) == 6
    for name, a, w in zip(batch._CSR_NAMES, csr, lists):
        assert a.dtype == torch.int32, name
        a = a.detach().cpu().numpy()
        if name.endswith("_ptr"):
            assert np.array_equal(a, w), name
        else:
            assert a.shape[0] in (w.shape[0], E), (name, a.shape, w.shape, E)
            assert np.array_equal(a[:w.shape[0]], w) and np.all(a[w.shape[0]:] == -1), name
    if device is not None:
        dev = torch.device(device).type
        for t in (batch.X, batch.src, batch.dst, batch.y, y) + tuple(csr):
            assert t.device.type == dev, (t.device, dev)


def short_y(g, by=3):
    return synth.HitGraph(g.X, g.src, g.dst, g.y[:len(g.y) - by].copy())


def long_y(g, by=4):
    return synth.HitGraph(g.X, g.src, g.dst, np.concatenate([g.y, np.zeros(by, np.float32)]))


def _ends(g, src=None, dst=None):
    return synth.HitGraph(g.X, g.src.copy() if src is None else src, g.dst.copy() if dst is None else dst, g.y)


def _set(a, k, v):
    a = a.copy()
    a[k] = v
    return a


# name -> graph -> the malformed copy of it every assembly entry has to refuse (tests put it at a chosen list position)
MALFORMED = {
    "y_short": short_y,
    "y_long": long_y,
    "x_1d": lambda g: synth.HitGraph(g.X.reshape(-1), g.src, g.dst, g.y),
    "x_3d": lambda g: synth.HitGraph(g.X[None], g.src, g.dst, g.y),
    "x_narrow": lambda g: synth.HitGraph(g.X[:, :1], g.src, g.dst, g.y),
    "x_wide": lambda g: synth.HitGraph(np.concatenate([g.X, g.X[:, :1]], axis=1), g.src, g.dst, g.y),
    "ends_float32": lambda g: _ends(g, g.src.astype(np.float32), g.dst.astype(np.float32)),
    "dst_float64": lambda g: _ends(g, dst=g.dst.astype(np.float64)),
    "ends_bool": lambda g: _ends(g, g.src > 0, g.dst > 0),
    "one_negative_src": lambda g: _ends(g, src=_set(g.src, 2, -1)),
    "one_negative_dst": lambda g: _ends(g, dst=_set(g.dst, 0, -3)),
    "src_at_n_hits": lambda g: _ends(g, src=_set(g.src, 1, g.X.shape[0])),
    "dst_past_n_hits": lambda g: _ends(g, dst=_set(g.dst, 5, g.X.shape[0] + 7)),
}
