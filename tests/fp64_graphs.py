"""Seeded graph families of tests/test_gpu_fp64_reference.py (test infrastructure, not product).

Each family is one block-diagonal batch in index form, built on the host:

  c3x4      4 x layered_graph(10000, 100000): about 1 % of the segments padded (src = dst = -1), scattered
  hubs      one graph of 36 080 hits: a layered background with 300 duplicated segments; for every degree in
            HUB_DEGREES one hit with exactly that in-degree and one with exactly that out-degree (asserted); 50
            isolated hits; segments shuffled
  superhub  one graph of 36 001 hits, one hit with 70 000 incoming segments (past the plan builder's 16-bit degree
            keys: the torch builder takes the batch) and 2 000 outgoing ones
  c3        one layered_graph(10000, 100000)
  ragged    a detector-size graph, a 1-hit graph (a self-loop), a 2-hit graph, a graph without segments, a graph of
            padded segments only, 200 small graphs
  events    300 muon-sized graphs, every 25th replaced by a hub event of up to 1 200 segments
  mu200     one layered_graph(50000, 500000)
"""
import functools
from collections import namedtuple

import numpy as np

from gnn_fpga_amd import synth

HUB_DEGREES = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000, 4097)

# X, src, dst, y, hit_ptr, seg_ptr: the batch; info: family-specific facts (hub ids, ...)
Family = namedtuple("Family", ["X", "src", "dst", "y", "hit_ptr", "seg_ptr", "info"])


def _concat(graphs):
    hp = np.concatenate([[0], np.cumsum([g.X.shape[0] for g in graphs])]).astype(np.int64)
    sp = np.concatenate([[0], np.cumsum([g.src.shape[0] for g in graphs])]).astype(np.int64)
    X = np.concatenate([g.X for g in graphs]).astype(np.float32)
    off = lambda a, i: np.where(a >= 0, a + hp[i], -1)                   # noqa: E731
    src = np.concatenate([off(np.asarray(g.src, np.int64), i) for i, g in enumerate(graphs)]).astype(np.int32)
    dst = np.concatenate([off(np.asarray(g.dst, np.int64), i) for i, g in enumerate(graphs)]).astype(np.int32)
    y = np.concatenate([np.asarray(g.y, np.float32) for g in graphs]).astype(np.float32)
    return X, src, dst, y, hp, sp


def _graph(X, src, dst, rng):
    src = np.asarray(src, np.int32)
    return synth.HitGraph(np.asarray(X, np.float32), src, np.asarray(dst, np.int32),
                          (rng.random(src.shape[0]) < 0.3).astype(np.float32))


def _family(graphs, info=None):
    return Family(*_concat(graphs), info or {})


@functools.lru_cache(maxsize=None)
def c3x4(F=3):
    X, src, dst, y, hp, sp = _concat([synth.layered_graph(10000, 100000, F, seed=180 + i) for i in range(4)])
    rng = np.random.default_rng(181)
    pad = rng.choice(src.shape[0], src.shape[0] // 100, replace=False)
    src, dst = src.copy(), dst.copy()
    src[pad] = -1
    dst[pad] = -1
    return Family(X, src, dst, y, hp, sp, {"padded": np.sort(pad)})


@functools.lru_cache(maxsize=None)
def c3(F=3):
    return _family([synth.layered_graph(10000, 100000, F, seed=190)])


@functools.lru_cache(maxsize=None)
def hubs(F=3):
    rng = np.random.default_rng(170)
    bg = synth.layered_graph(36000, 100000, F, seed=171)
    n0 = bg.X.shape[0]
    dup = rng.integers(0, bg.src.shape[0], 300)                           # duplicate segments (background only:
    src, dst = [bg.src, bg.src[dup]], [bg.dst, bg.dst[dup]]               # the hub degrees stay exact)
    in_hub, out_hub = {}, {}
    for k, d in enumerate(HUB_DEGREES):
        h_in, h_out = n0 + 2 * k, n0 + 2 * k + 1
        in_hub[d], out_hub[d] = h_in, h_out
        src += [rng.integers(0, n0, d), np.full(d, h_out)]
        dst += [np.full(d, h_in), rng.integers(0, n0, d)]
    src, dst = np.concatenate(src), np.concatenate(dst)
    n = n0 + 2 * len(HUB_DEGREES) + 50                                    # the last 50 hits: isolated
    X = np.concatenate([bg.X, rng.uniform(-1, 1, (n - n0, F)).astype(np.float32)])
    perm = rng.permutation(src.shape[0])                                  # hub lists scattered in the caller's order
    src, dst = src[perm], dst[perm]
    g = _graph(X, src, dst, rng)
    deg_in, deg_out = np.bincount(dst, minlength=n), np.bincount(src, minlength=n)
    for d in HUB_DEGREES:
        assert deg_in[in_hub[d]] == d and deg_out[in_hub[d]] == 0 and deg_out[out_hub[d]] == d and deg_in[out_hub[d]] == 0
    assert not deg_in[n - 50:].any() and not deg_out[n - 50:].any()
    return _family([g], {"in_hub": in_hub, "out_hub": out_hub, "isolated": np.arange(n - 50, n)})


@functools.lru_cache(maxsize=None)
def superhub(F=3):
    rng = np.random.default_rng(172)
    bg = synth.layered_graph(36000, 60000, F, seed=173)
    n0 = bg.X.shape[0]
    hub = n0
    src = np.concatenate([bg.src, rng.integers(0, n0, 70000), np.full(2000, hub)])
    dst = np.concatenate([bg.dst, np.full(70000, hub), rng.integers(0, n0, 2000)])
    X = np.concatenate([bg.X, rng.uniform(-1, 1, (1, F)).astype(np.float32)])
    perm = rng.permutation(src.shape[0])
    g = _graph(X, src[perm], dst[perm], rng)
    return _family([g], {"hub": hub})


@functools.lru_cache(maxsize=None)
def ragged(F=3):
    rng = np.random.default_rng(174)
    graphs = [synth.layered_graph(20000, 100000, F, seed=175)]
    x = lambda n: rng.uniform(-1, 1, (n, F))                              # noqa: E731
    graphs.append(_graph(x(1), [0], [0], rng))                             # one hit, a self-loop
    graphs.append(_graph(x(2), [0, 1, 0], [1, 0, 1], rng))                 # two hits, a duplicate
    graphs.append(_graph(x(7), [], [], rng))                               # no segments
    graphs.append(_graph(x(5), [-1] * 4, [-1] * 4, rng))                   # padded segments only
    for i in range(200):
        graphs.append(synth.layered_graph(int(rng.integers(8, 80)), int(rng.integers(1, 300)), F, n_layers=4,
                                          seed=1000 + i))
    order = rng.permutation(len(graphs))                                    # the big graph somewhere in the middle
    return _family([graphs[i] for i in order])


@functools.lru_cache(maxsize=None)
def events(F=11):
    rng = np.random.default_rng(176)
    graphs = []
    for i in range(300):
        if i % 25 == 7:                                                    # a hub event: hit 0 with up to 1200 segments
            n, half = 41, (600, 450, 150)[(i // 25) % 3]
            src = np.concatenate([np.zeros(half, int), rng.integers(1, n, half)])
            dst = np.concatenate([rng.integers(1, n, half), np.zeros(half, int)])
            graphs.append(_graph(rng.uniform(-1, 1, (n, F)), src, dst, rng))
        else:
            g = synth.muon_graph(seed=2000 + i)
            if F != g.X.shape[1]:
                g = synth.HitGraph(g.X[:, :F] if F < g.X.shape[1] else np.pad(g.X, ((0, 0), (0, F - g.X.shape[1]))),
                                   g.src, g.dst, g.y)
            graphs.append(g)
    return _family(graphs)


@functools.lru_cache(maxsize=None)
def mu200(F=3):
    return _family([synth.layered_graph(50000, 500000, F, seed=200)])


FAMILIES = {"c3x4": c3x4, "c3": c3, "hubs": hubs, "superhub": superhub, "ragged": ragged, "events": events,
            "mu200": mu200}


def family(name, F):
    return FAMILIES[name](F)
