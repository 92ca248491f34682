"""The alternating tile walk of the k_iter2 route (csrc/sell_pipeline.hip: `backward` of k_iter2 and k_edge) and the
wide sweeps' trimmed last step group (sweep_w) against the C oracle, on the batch of tests/trim_graphs.py: 300 graphs
whose slice lengths take every residue mod 4 in both lists, with lists of 1, 4, 5, 8 and 27 steps and empty ones
(tests/test_trim_host.py asserts that on the plan).  57.6 k hits in more than 256 tiles: every persistent workgroup
of k_iter2 walks several tiles, forward and backward, and the wide shapes take k_iter_wx without a switch.

Bounds are the project's: 1e-5 for the fp32 routes, TOL_BF16 for bf16 records.  Two forwards of a case give the same
bits, and the launched kernels are the intended family (a fallback to the general k_iter cannot pass)."""
import numpy as np
import pytest
import torch

from gnn_fpga_amd import HitGraphBatch
from gnn_fpga_amd.model import SegmentClassifier
from oracle import index_c

import trim_graphs

TOL_BF16 = 2e-3     # bf16 records and matrix-core operands (GNN_FLAG_BF16_MLP): the project's bound for that route

N_GRAPHS = 300
SWITCHES = ("GNN_NO_ITER2", "GNN_NO_FUSE_FIRST", "GNN_NO_WIDE_EXACT", "GNN_WIDE_LOCKSTEP", "GNN_WIDE_ROLES")

_graphs = {}


def _batch_graphs(F):
    if F not in _graphs:
        _graphs[F] = trim_graphs.trim_graphs(N_GRAPHS, F)
    return _graphs[F]


def _case(F, D, T, family, xp=True, bf16=False, env=None, fused_first=None):
    name = "%dx%d_T%d%s%s%s" % (F, D, T, "" if xp else "_plain_exp", "_bf16" if bf16 else "", "_" + env if env else "")
    return pytest.param(dict(F=F, D=D, T=T, family=family, xp=xp, bf16=bf16, env=env, fused_first=fused_first), id=name)


CASES = [
    # k_iter2: T = 1 is a last launch behind k_input4; from T = 2 on the first launch runs the input network too,
    # and the launches walk forward, backward, forward, backward - k_edge against the last one
    _case(3, 8, 1, "k_iter2", fused_first=False),
    _case(3, 8, 2, "k_iter2", fused_first=True),
    _case(3, 8, 3, "k_iter2", fused_first=True),
    _case(3, 8, 4, "k_iter2", fused_first=True),
    _case(3, 8, 3, "k_iter2", xp=False, fused_first=False),
    _case(3, 4, 3, "k_iter2", fused_first=True),
    _case(11, 8, 3, "k_iter2", fused_first=False),          # the unfused input stage
    # the wide kernels: exact fp32 rows, bf16 rows, and the lockstep kernel
    _case(3, 16, 2, "k_iter_wx"),
    _case(3, 32, 2, "k_iter_wx"),
    _case(3, 64, 2, "k_iter_wx"),
    _case(3, 64, 2, "k_iter_wx", bf16=True),
    _case(3, 32, 2, "k_iter_w", env="GNN_WIDE_LOCKSTEP"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_walk_and_trimmed_sweeps_against_the_oracle(hip, case, monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if case["env"]:
        monkeypatch.setenv(case["env"], "1")
    F, D, T = case["F"], case["D"], case["T"]
    graphs = _batch_graphs(F)
    torch.manual_seed(100 * F + D + T)
    model = SegmentClassifier(input_dim=F, hidden_dim=D, n_iters=T).cuda().eval()
    model.use_plan, model.use_events = True, False
    model.exp_product, model.mlp_bf16 = case["xp"], case["bf16"]
    batch = HitGraphBatch.from_graphs(graphs).cuda()
    with torch.no_grad():
        model(batch)                                # (the batch's one-time work: the plan)
        with hip.profile(64) as prof:
            first = model(batch).clone()
        second = model(batch).clone()
    torch.cuda.synchronize()
    plan = batch.plan
    assert plan.n_tiles > 256 or D >= 16
    assert plan.n_pad >= 32768

    names = [k for k, _ in prof.records]
    assert names.count(case["family"]) == T, names
    assert "k_iter" not in names and names[-1] == "k_edge", names
    if case["xp"]:
        assert model._xp_cache[1] == hip.GNN_FLAG_EXP_PRODUCT       # the exp-product kernels really ran
    if case["fused_first"] is not None:
        assert ("k_input4" not in names) == case["fused_first"], names

    assert torch.equal(first, second)

    params = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    tol = TOL_BF16 if case["bf16"] else 1e-5
    worst = 0.0
    for g, eg in zip(graphs, batch.split_scores(first.cpu().numpy())):
        ref = index_c.segment_classifier(g.X, g.src, g.dst, params, T)
        worst = max(worst, float(np.abs(eg - ref).max()))
    print("max |HIP - oracle| = %.3g (bound %g)" % (worst, tol))
    assert worst < tol, worst
