"""tests/big_graphs.py on the host (no GPU): the guard windows against forward_t's formulas, the simulated plan
padding against plan.py's own plan, and the tiled batches' layout (copies map back to their pool graphs, every hit
count odd).  Small targets: a 64 MiB stand-in for the 4 GiB guard puts n_pad near 131 072."""
import numpy as np
import pytest

import big_graphs
from gnn_fpga_amd import HitGraphBatch, _lib
from gnn_fpga_amd.plan import SellPlan

SMALL = 1 << 26


@pytest.mark.parametrize("D,B", [(64, 8), (32, 8), (16, 8), (64, 4), (32, 4)])
@pytest.mark.parametrize("limit", [big_graphs.GUARD_BYTES, SMALL])
def test_windows_sit_on_the_guard(D, B, limit):
    """"below": every n_pad of the window satisfies (n_pad + 2) * D * B < limit, its top is the largest multiple of 16
    that does, and its rows end within 1 MiB of the limit; "above": every n_pad violates it and its bottom is the
    first multiple of 16 that does."""
    lo, hi = big_graphs.window(D, B, "below", limit)
    assert lo % 16 == 0 and hi % 16 == 0 and lo < hi
    assert all(big_graphs.guard_ok(n, D, B, limit) for n in (lo, hi))
    assert not big_graphs.guard_ok(hi + 16, D, B, limit)
    assert limit - (lo + 2) * D * B <= (1 << 20) + 16 * D * B
    alo, ahi = big_graphs.window(D, B, "above", limit)
    assert alo % 16 == 0 and alo == hi + 16
    assert not any(big_graphs.guard_ok(n, D, B, limit) for n in (alo, ahi))
    assert (ahi - alo) * D * B == 1 << 20
    if limit == big_graphs.GUARD_BYTES:       # forward_t's values: the n_pad the issue's table names
        assert hi + 2 == (1 << 32) // (D * B) - 14


def test_pool_hit_counts_are_odd():
    for F in (2, 3):
        sizes = [g.X.shape[0] for g in big_graphs.pool(F)]
        assert len(set(sizes)) == big_graphs.POOL_GRAPHS and all(n % 2 == 1 for n in sizes), sizes
        assert all(20000 < n < 40000 for n in sizes), sizes


@pytest.mark.parametrize("side", ["below", "above"])
def test_tiled_batch_lands_in_its_window(side):
    """The simulated n_pad of a tiled batch is the n_pad plan.py's SellPlan gives it, inside the window; the copies
    map back to their pool graphs (features, endpoints offset by the copy's first hit, labels); every graph's hit
    count is odd."""
    F, D, B = 3, 64, 8
    lim = _lib.plan_limits(F, D)
    lo, hi = big_graphs.window(D, B, side, SMALL)
    t = big_graphs.tiled(F, lim, lo, hi, "hi" if side == "below" else "lo")
    assert lo <= t.n_pad <= hi
    assert all(g.X.shape[0] % 2 == 1 for g in t.graphs)
    b = HitGraphBatch(t.X, t.src, t.dst, y=t.y, hit_ptr=t.hit_ptr, seg_ptr=t.seg_ptr)
    plan = SellPlan(b, lim)
    assert plan.n_pad == t.n_pad, (plan.n_pad, t.n_pad)
    assert big_graphs.guard_ok(plan.n_pad, D, B, SMALL) == (side == "below")
    assert len(t.copies) == len(t.hit_ptr) - 1 == len(t.seg_ptr) - 1
    assert t.copies[-1] == big_graphs.POOL_GRAPHS and (t.copies[:-1] < big_graphs.POOL_GRAPHS).all()
    assert len(set(t.copies[:-1].tolist())) > 1
    for k, c in enumerate(t.copies):
        g = t.graphs[c]
        h0, h1, s0, s1 = (int(v) for v in (t.hit_ptr[k], t.hit_ptr[k + 1], t.seg_ptr[k], t.seg_ptr[k + 1]))
        assert h1 - h0 == g.X.shape[0] and s1 - s0 == g.src.shape[0]
        assert np.array_equal(t.X[h0:h1], g.X)
        assert np.array_equal(t.src[s0:s1], g.src + h0) and np.array_equal(t.dst[s0:s1], g.dst + h0)
        assert np.array_equal(t.y[s0:s1], g.y)


def test_simulated_padding_matches_plan_at_a_narrow_shape():
    """The same at (3, 8): 1280-hit tiles, whole (graph, level) units merged across graph boundaries."""
    F, D = 3, 8
    lim = _lib.plan_limits(F, D)
    lo = 512 * 1280 + 60000
    t = big_graphs.tiled(F, lim, lo, lo + 2048)
    b = HitGraphBatch(t.X, t.src, t.dst, hit_ptr=t.hit_ptr, seg_ptr=t.seg_ptr)
    assert SellPlan(b, lim).n_pad == t.n_pad


def test_repeated_and_by_hits():
    g = big_graphs.pool(3)[0]
    r = big_graphs.repeated(g, 100000)
    k = len(r.copies)
    assert r.X.shape[0] == k * g.X.shape[0] >= 100000 > (k - 1) * g.X.shape[0]
    assert np.array_equal(r.src.reshape(k, -1) - r.hit_ptr[:-1, None].astype(np.int32), np.tile(g.src, (k, 1)))
    h = big_graphs.by_hits(3, 200000)
    assert h.X.shape[0] >= 200000 and h.hit_ptr[-1] == h.X.shape[0]
