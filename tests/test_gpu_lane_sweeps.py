"""The list sweeps of k_iter2 (csrc/sell_pipeline.hip: sweep16 and the one-step-per-lane form sweep16_lane) against
the C oracle on the graphs of tests/lane_graphs.py: three graphs of 2560 hits whose per-hit in- and out-list lengths
are drawn from {0, 1, 3, 4, 5, 7, 8, 9, 23, 24, 25, 33} - both halves of a list word, both step groups of a word, the
streamed words past the 24 prefetched steps, and slices that mix the lengths (tests/test_lane_sweep_host.py asserts
that on the plan).

Every shape of the k_iter2 route that differs in the sweeps - (F, D) = (3, 8), (2, 8), (3, 4), (11, 8) - with the
exp-product arithmetic on and off and T = 1 .. 4: the first (fused where the shape has it), middle and last launch
variants and both walk directions.  The launched kernels are asserted through the profile, scores are within the
suite's 1e-5 of the oracle, and two forwards give the same bits."""
import numpy as np
import pytest
import torch

from gnn_fpga_amd import HitGraphBatch
from gnn_fpga_amd.model import SegmentClassifier
from oracle import index_c

import lane_graphs

TOL = 1e-5          # edge scores, as in tests/test_gpu_parity.py and tests/test_gpu_trimmed_sweeps.py
SWITCHES = ("GNN_NO_ITER2", "GNN_NO_FUSE_FIRST", "GNN_NO_WIDE_EXACT", "GNN_WIDE_LOCKSTEP", "GNN_WIDE_ROLES")
SHAPES = [(3, 8), (2, 8), (3, 4), (11, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 2, 3, 4])
@pytest.mark.parametrize("xp", [True, False], ids=["exp_product", "plain_exp"])
@pytest.mark.parametrize("F,D", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_lane_sweeps_against_the_oracle(hip, F, D, xp, T, monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    graphs = lane_graphs.lane_graphs(F)
    torch.manual_seed(1000 * F + 10 * D + T)
    model = SegmentClassifier(input_dim=F, hidden_dim=D, n_iters=T).cuda().eval()
    model.use_plan, model.use_events = True, False
    model.exp_product, model.mlp_bf16 = xp, False
    batch = HitGraphBatch.from_graphs(graphs).cuda()
    with torch.no_grad():
        model(batch)                                # (the batch's one-time work: the plan)
        with hip.profile(64) as prof:
            first = model(batch).clone()
        second = model(batch).clone()
    torch.cuda.synchronize()

    names = [k for k, _ in prof.records]
    assert names.count("k_iter2") == T, names
    assert "k_iter" not in names and names[-1] == "k_edge", names
    if xp:
        assert model._xp_cache[1] == hip.GNN_FLAG_EXP_PRODUCT       # the exp-product kernels really ran

    assert torch.equal(first, second)

    params = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    worst = 0.0
    for g, eg in zip(graphs, batch.split_scores(first.cpu().numpy())):
        ref = index_c.segment_classifier(g.X, g.src, g.dst, params, T)
        worst = max(worst, float(np.abs(eg - ref).max()))
    print("max |HIP - oracle| = %.3g (bound %g)" % (worst, TOL))
    assert worst < TOL, worst
