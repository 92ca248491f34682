"""What tests/test_gpu_trimmed_sweeps.py relies on, checked on the host plan (no GPU): the batch of tests/trim_graphs.py
reaches every tail length of the sweeps, the streaming part of a long list, empty lists, and more tiles than the GPU
has compute units - and the padding counts of DESIGN.md section 4 (k_iter2: what whole step groups cost there) are
those of the c3 plan."""
import numpy as np
import pytest

from gnn_fpga_amd import HitGraphBatch, _lib, synth
from gnn_fpga_amd.plan import SellPlan

import trim_graphs

N_GRAPHS = 300                      # the GPU test's batch


@pytest.fixture(scope="module")
def plan():
    batch = HitGraphBatch.from_graphs(trim_graphs.trim_graphs(N_GRAPHS))
    return SellPlan(batch, _lib.plan_limits(3, 8))


def test_graph_is_layered_and_has_the_stated_hits():
    g = trim_graphs.trim_graph()
    n, per = trim_graphs.LAYERS * trim_graphs.PER_LAYER, trim_graphs.PER_LAYER
    assert g.X.shape == (n, 3)
    assert ((g.dst // per) - (g.src // per) == 1).all()             # consecutive layers only
    assert len(set(zip(g.src.tolist(), g.dst.tolist()))) == g.src.shape[0]
    deg_in, deg_out = np.bincount(g.dst, minlength=n), np.bincount(g.src, minlength=n)
    assert deg_in.max() == 27 and deg_out.max() == 27
    inner = slice(per, 2 * per)                                     # layer 1 has segments on both sides ...
    assert (deg_in[inner] == 0).sum() == 1 and (deg_out[inner] == 0).sum() == 1     # ... and one hit without each
    assert np.flatnonzero(deg_in[inner] == 0)[0] != np.flatnonzero(deg_out[inner] == 0)[0]


def test_slice_lengths_reach_every_tail_path(plan):
    steps_in, steps_out = trim_graphs.slice_steps(plan)
    for steps in (steps_in, steps_out):
        real = steps[steps > 0]
        assert set((real % 4).tolist()) == {0, 1, 2, 3}             # rem = 4, 1, 2, 3 of the last group
        assert {1, 4, 5, 8} <= set(real.tolist())                   # a tail alone, a full group alone, one + a tail, two
        assert real.max() > 24                                      # past the prefetched words of k_iter2
        assert (steps == 0).any()                                   # slices without a list
    assert plan.max_list_steps == 27
    assert plan.n_tiles > 256                                       # several tiles per persistent workgroup
    assert plan.n_lds_tiles == plan.n_tiles                         # every tile in LDS mode: the k_iter2 route
    assert plan.n_pad >= 32768                                      # wide shapes: k_iter_wx without a switch


@pytest.mark.parametrize("D", [16, 64])
def test_wide_plans_reach_every_tail_path_too(D):
    """The wide kernels' plan has other tiles (256 hits): the same residues there."""
    batch = HitGraphBatch.from_graphs(trim_graphs.trim_graphs(N_GRAPHS))
    p = SellPlan(batch, _lib.plan_limits(3, D))
    for steps in trim_graphs.slice_steps(p):
        real = steps[steps > 0]
        assert set((real % 4).tolist()) == {0, 1, 2, 3}
        assert real.max() == 27 and (steps == 0).any()
    assert p.n_pad >= 32768


def test_visit_ratios_of_the_c3_plan():
    """Record visits per real record of the two sweeps on the benchmark's graphs (c3: 10k hits, 100k segments), with
    lists rounded up to whole groups of 4 steps (what sweep16 visits) and at the slice's own step count: the table
    of DESIGN.md section 4 within 0.01.  66 graphs is the smallest batch that gets the kernels' own 1280-hit tiles
    (smaller ones get smaller tiles, and other padding)."""
    batch = HitGraphBatch.from_graphs([synth.layered_graph(10000, 100000, 3, seed=i) for i in range(66)])
    p = SellPlan(batch, _lib.plan_limits(3, 8))
    assert p.n_tiles == 660 and 1024 < p.tile_hits_max <= 1280      # whole levels of ~1000 hits, one per tile
    rounded, exact = trim_graphs.visit_ratios(p)
    assert np.abs(np.array(rounded) - np.array([1.154, 1.225, 1.189])).max() < 0.01, rounded
    assert np.abs(np.array(exact) - np.array([1.108, 1.090, 1.099])).max() < 0.01, exact
    assert abs(exact[2] - 1.0 - p.padding) < 1e-9                   # (the bench line's "list padding")
