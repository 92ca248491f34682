"""Batches past the 4 GiB record-table and 2^31-element marks for tests/test_gpu_index_width.py (test infrastructure,
not product).

A wrapped or truncated offset does not fault: it reads a valid row of another hit.  So a batch here is made of
copies of a small pool of distinct seeded layered graphs, each with an ODD hit count, laid out in a seeded random
order (no period that a power-of-two wrap distance could map onto an identical row), and every copy's scores are
checked against its own pool graph's reference.

The wide kernels (k_iter_w, k_iter_wx) address record rows with 32-bit byte offsets; choose_route
(csrc/sell_pipeline.hip) takes them only while the table stays below 4 GiB:

  bf16 records        (n_pad + 2) * D * 4 < 2^32
  exact fp32 records  (n_pad + 2) * D * 8 < 2^32

`window(D, B, side)` gives the n_pad range on each side of that guard ("below": the last rows within 1 MiB of
4 GiB; "above": the first 1 MiB past it).  `tiled` then builds a batch whose plan has an n_pad inside a window: the
plan's padding (plan.py: (graph, level) units merged greedily into tiles of at most tile_hits hits, every tile padded
to a multiple of 16) is simulated on the pool graphs' levels, and a last "filler" graph is sized so that n_pad lands
in the window.  The arrays are built on the host with numpy, copy by copy, never through from_graphs.
"""
import functools
from collections import namedtuple

import numpy as np

from gnn_fpga_amd import synth
from gnn_fpga_amd.plan import SLICE, topological_levels

GUARD_BYTES = 1 << 32
WINDOW_BYTES = 1 << 20
POOL_GRAPHS = 8
SEGS_PER_HIT = 4
RECORD_BYTES = {"bf16": 4, "exact": 8}        # bytes per hidden dim of one record row in the wide kernels' tables


def guard_ok(n_pad, D, B, limit=GUARD_BYTES):
    """choose_route's condition for the wide kernels: (n_pad + 2) * D * B < 2^32."""
    return (n_pad + 2) * D * B < limit


def window(D, B, side, limit=GUARD_BYTES):
    """(lo, hi): the n_pad values (multiples of SLICE) on one side of the guard.  "below": the largest n_pad that
    satisfies it and the rows up to WINDOW_BYTES under it; "above": the first n_pad that violates it and the rows up
    to WINDOW_BYTES past it."""
    rows = limit // (D * B)                   # a power of two: the guard holds iff n_pad + 2 < rows
    span = WINDOW_BYTES // (D * B)
    if side == "below":
        hi = (rows - 3) // SLICE * SLICE
        return hi - span, hi
    lo = (rows - 2 + SLICE - 1) // SLICE * SLICE
    return lo, lo + span


def _odd_sizes(rng, n, lo=20001, hi=39999):
    return [int(2 * k + 1) for k in rng.integers(lo // 2, hi // 2 + 1, n)]


@functools.lru_cache(maxsize=None)
def pool(F, sizes=(20001, 39999), segs_per_hit=SEGS_PER_HIT, seed=900):
    """POOL_GRAPHS distinct seeded layered graphs of sizes[0] - sizes[1] hits (odd), segs_per_hit segments per hit."""
    rng = np.random.default_rng(seed)
    return tuple(synth.layered_graph(n, segs_per_hit * n, F, seed=seed + 1 + i)
                 for i, n in enumerate(_odd_sizes(rng, POOL_GRAPHS, *sizes)))


def filler(F, n, seed=950):
    return synth.layered_graph(n, SEGS_PER_HIT * n, F, seed=seed + n)


def units(g):
    """Sizes of the graph's (level) units in level order, as plan.py groups its hits."""
    lv = topological_levels(np.asarray(g.src, np.int64), np.asarray(g.dst, np.int64), g.X.shape[0])
    c = np.bincount(lv)
    return c[c > 0].tolist()


@functools.lru_cache(maxsize=None)
def _pool_units(F):
    return tuple(units(g) for g in pool(F))


class _Tiler:
    """plan.py's greedy tiling of (graph, level) units, one unit at a time: n_pad of everything added so far."""

    def __init__(self, tile_hits):
        self.tile_hits, self.closed, self.cur = tile_hits, 0, 0

    @staticmethod
    def _pad(n):
        return (n + SLICE - 1) // SLICE * SLICE

    def add(self, sizes):
        th = self.tile_hits
        for sz in sizes:
            if sz > th:                        # a big unit is split: full tiles, then the remainder
                if self.cur:
                    self.closed += self._pad(self.cur)
                    self.cur = 0
                k = (sz - 1) // th
                self.closed += k * th + self._pad(sz - k * th)
                continue
            if self.cur + sz > th:
                self.closed += self._pad(self.cur)
                self.cur = 0
            self.cur += sz

    def n_pad(self):
        return self.closed + self._pad(self.cur)

    def copy(self):
        t = _Tiler(self.tile_hits)
        t.closed, t.cur = self.closed, self.cur
        return t


def tile_hits_for(n_hits, limits):
    """The tile size plan.py uses for a batch of n_hits (small batches shrink their tiles)."""
    th = int(limits["tile_hits"])
    want = 512 if int(limits["iter_records"]) > 0 else 256
    if n_hits < want * th:
        th = max(64, ((n_hits + want - 1) // want + SLICE - 1) // SLICE * SLICE)
    return th


def simulate_n_pad(graph_units, n_hits, limits):
    t = _Tiler(tile_hits_for(n_hits, limits))
    for u in graph_units:
        t.add(u)
    return t.n_pad()


# graphs: the pool graphs, then the filler of `tiled` (index POOL_GRAPHS); copies: the graph index of every copy in
# batch order; hit_ptr / seg_ptr [len(copies) + 1]: where every copy starts; n_pad: the simulated plan n_pad (tiled)
Tiled = namedtuple("Tiled", ["X", "src", "dst", "y", "hit_ptr", "seg_ptr", "graphs", "copies", "n_pad"])


def assemble(graphs, copies):
    """The batch of graphs[copies[0]], graphs[copies[1]], ... with ids offset per copy (numpy, on the host)."""
    nh = np.array([graphs[c].X.shape[0] for c in copies], np.int64)
    ns = np.array([graphs[c].src.shape[0] for c in copies], np.int64)
    hp = np.concatenate([[0], np.cumsum(nh)])
    sp = np.concatenate([[0], np.cumsum(ns)])
    if hp[-1] >= 2 ** 31 or sp[-1] >= 2 ** 31:
        raise ValueError("batch outside the int32 index range")
    F = graphs[copies[0]].X.shape[1]
    X = np.empty((int(hp[-1]), F), np.float32)
    src = np.empty(int(sp[-1]), np.int32)
    dst = np.empty(int(sp[-1]), np.int32)
    y = np.empty(int(sp[-1]), np.float32)
    for k, c in enumerate(copies):
        g, h0, s0, s1 = graphs[c], int(hp[k]), int(sp[k]), int(sp[k + 1])
        X[h0:int(hp[k + 1])] = g.X
        np.add(g.src, h0, out=src[s0:s1], dtype=np.int32)       # (layered graphs have no padded segments)
        np.add(g.dst, h0, out=dst[s0:s1], dtype=np.int32)
        y[s0:s1] = g.y
    return X, src, dst, y, hp, sp


def tiled(F, limits, lo, hi, edge="hi", seed=910):
    """A batch of pool copies in seeded random order plus one filler graph, with a simulated plan n_pad in [lo, hi].
    n_pad is taken as close to `edge` ("hi" / "lo") of the window as a filler size gets it.  Batches small enough
    for the tile shrink of plan.py are refused (the simulation assumes the full tile size)."""
    graphs = list(pool(F))
    gu = _pool_units(F)
    th = int(limits["tile_hits"])
    want = 512 if int(limits["iter_records"]) > 0 else 256
    if lo < want * th + 50000:
        raise ValueError("target below the tile-shrink size of plan.py")
    rng = np.random.default_rng(seed)
    t = _Tiler(th)
    copies = []
    while True:                                # pool copies up to one pool graph's size short of the window
        c = int(rng.integers(0, POOL_GRAPHS))
        nxt = t.copy()
        nxt.add(gu[c])
        if nxt.n_pad() > lo - 45000:
            break
        t = nxt
        copies.append(c)
    base = t.n_pad()

    def with_filler(n):
        f = filler(F, n)
        s = t.copy()
        s.add(units(f))
        return f, s.n_pad()

    # the filler's n_pad grows with its size in steps of SLICE, nearly monotonically: bisect on the side of the
    # window nearest the guard (`edge`: "hi" for "below", "lo" for "above"), then take the closest size around it
    target = hi if edge == "hi" else lo
    a, b = 1001 // 2, 99999 // 2
    while b - a > 4:
        m = (a + b) // 2
        if with_filler(2 * m + 1)[1] <= target:
            a = m
        else:
            b = m
    best = None
    for m in range(max(a - 48, 500), a + 48):
        f, n_pad = with_filler(2 * m + 1)
        if lo <= n_pad <= hi and (best is None or abs(n_pad - target) < abs(best[1] - target)):
            best = (f, n_pad)
    if best is None:
        raise ValueError("no filler puts n_pad in [%d, %d] (pool copies end at %d)" % (lo, hi, base))
    f, n_pad = best
    graphs.append(f)
    copies.append(POOL_GRAPHS)
    X, src, dst, y, hp, sp = assemble(graphs, copies)
    assert simulate_n_pad([units(graphs[c]) if c == POOL_GRAPHS else gu[c] for c in copies], X.shape[0],
                          limits) == n_pad
    return Tiled(X, src, dst, y, hp, sp, graphs, np.asarray(copies), n_pad)


def repeated(g, n_min):
    """Identical copies of ONE graph until the batch holds at least n_min hits."""
    k = -(-n_min // g.X.shape[0])
    X, src, dst, y, hp, sp = assemble([g], [0] * k)
    return Tiled(X, src, dst, y, hp, sp, [g], np.zeros(k, np.int64), None)


def by_hits(F, n_min, pool_sizes=(20001, 39999), segs_per_hit=SEGS_PER_HIT, seed=920):
    """Pool copies in seeded random order until the batch holds at least n_min hits (no plan target)."""
    rng = np.random.default_rng(seed)
    graphs = list(pool(F, pool_sizes, segs_per_hit))
    sizes = [g.X.shape[0] for g in graphs]
    copies, n = [], 0
    while n < n_min:
        c = int(rng.integers(0, POOL_GRAPHS))
        copies.append(c)
        n += sizes[c]
    X, src, dst, y, hp, sp = assemble(graphs, copies)
    return Tiled(X, src, dst, y, hp, sp, graphs, np.asarray(copies), None)
