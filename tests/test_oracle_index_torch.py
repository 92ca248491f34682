"""Pins oracle/index_torch.py (the fp64 training reference of tests/test_gpu_fp64_reference.py) before any GPU test
depends on it: against autograd through the dense restatement (oracle/dense_torch.py) in fp64, and against the
outputs and training steps of the reference itself (tests/golden/)."""
import numpy as np
import pytest
import torch

from golden_util import BATCHES, SINGLE, Fixture, assert_grad_close
from gnn_fpga_amd import synth
from oracle import dense_torch, index_torch
from oracle.dense_torch import KEYS

REL = 1e-12


def _graph(kind, F, seed):
    """Small graphs with the irregularities the kernels must get right (index form, padded segments = -1)."""
    rng = np.random.default_rng(seed)
    if kind == "no_segments":
        X = rng.uniform(-1, 1, (9, F)).astype(np.float32)
        return X, np.zeros(0, np.int32), np.zeros(0, np.int32)
    if kind == "all_padded":
        X = rng.uniform(-1, 1, (6, F)).astype(np.float32)
        return X, -np.ones(4, np.int32), -np.ones(4, np.int32)
    g = synth.layered_graph(60, 180, F, n_layers=5, seed=seed)
    src, dst = list(g.src), list(g.dst)
    n = g.X.shape[0]
    src += list(src[:7]); dst += list(dst[:7])                          # duplicate segments
    src += [0, 1, 2]; dst += [1, 2, 0]                                   # within one layer, a cycle
    src += [3]; dst += [3]                                               # a self-loop
    X = np.concatenate([g.X, rng.uniform(-1, 1, (4, F)).astype(np.float32)])   # 4 isolated hits (n .. n+3)
    if kind == "hub":
        hub = 5
        others = rng.integers(0, n, 200)
        half = 100
        src += [hub] * half + list(others[half:]); dst += list(others[:half]) + [hub] * half
    src, dst = np.array(src, np.int32), np.array(dst, np.int32)
    pad = rng.permutation(src.shape[0])[:9]                              # padded segments anywhere in the order
    src[pad] = -1
    dst[pad] = -1
    return X, src, dst


def _params(F, D, seed, scale=1.0):
    torch.manual_seed(seed)
    C = F + D
    shapes = {"input_network.0.weight": (D, F), "input_network.0.bias": (D,),
              "edge_network.network.0.weight": (D, 2 * C), "edge_network.network.0.bias": (D,),
              "edge_network.network.2.weight": (1, D), "edge_network.network.2.bias": (1,),
              "node_network.network.0.weight": (D, 3 * C), "node_network.network.0.bias": (D,),
              "node_network.network.2.weight": (D, D), "node_network.network.2.bias": (D,)}
    return {k: (scale * (torch.rand(*shapes[k], dtype=torch.float64) * 2 - 1)).requires_grad_(True) for k in KEYS}


def _masks(F, D, seed):
    g = torch.Generator().manual_seed(seed)
    C = F + D
    return {"edge_network.network.0.weight": (torch.rand(D, 2 * C, generator=g) < 0.7).double(),
            "edge_network.network.2.weight": (torch.rand(1, D, generator=g) < 0.8).double(),
            "node_network.network.0.weight": (torch.rand(D, 3 * C, generator=g) < 0.7).double(),
            "node_network.network.2.weight": (torch.rand(D, D, generator=g) < 0.8).double()}


def _close(a, r, what, rel=REL):
    if a is None or r is None:              # T = 0: the node network takes no part
        assert a is None and r is None, what
        return
    a, r = a.detach(), r.detach()
    scale = float(r.abs().max()) if r.numel() else 0.0
    err = float((a - r).abs().max()) if r.numel() else 0.0
    assert err <= rel * max(scale, 1e-300), (what, err, scale)


CASES = [("layered", 3, 8, 3, False), ("hub", 3, 8, 2, False), ("hub", 2, 4, 3, True), ("layered", 11, 32, 2, True),
         ("hub", 11, 8, 1, False), ("layered", 2, 32, 0, False), ("no_segments", 3, 4, 2, False),
         ("all_padded", 3, 8, 2, False), ("hub", 3, 32, 2, True)]


@pytest.mark.parametrize("kind,F,D,T,masked", CASES)
def test_index_torch_equals_the_dense_restatement_in_fp64(kind, F, D, T, masked):
    """Scores, every traced e / H, a BCE loss and all ten gradients against autograd through dense_torch (the
    reference's own bmm formulation) at 1e-12 relative: padded segments (scored, summed nowhere), isolated hits,
    duplicate segments, segments within one layer and a self-loop, a hub of 200 segments, masked weights, graphs
    without segments or with padded ones only; F in {2, 3, 11}, D in {4, 8, 32}."""
    X, src, dst = _graph(kind, F, seed=F * 100 + D + T)
    masks = _masks(F, D, seed=D) if masked else None
    p_i = _params(F, D, seed=7 * D + F)
    p_d = {k: v.detach().clone().requires_grad_(True) for k, v in p_i.items()}
    y = torch.from_numpy((np.arange(src.shape[0]) % 3 == 0).astype(np.float64))
    tr_i, tr_d = {}, {}
    e_i = index_torch.segment_classifier(X, src, dst, p_i, T, masks, trace=tr_i)
    # dense: padded segments are all-zero columns of Ri / Ro
    ok = src >= 0
    n, E = X.shape[0], src.shape[0]
    Ri = torch.zeros(1, n, E, dtype=torch.float64)
    Ro = torch.zeros(1, n, E, dtype=torch.float64)
    j = np.flatnonzero(ok)
    Ri[0, dst[ok], j] = 1.0
    Ro[0, src[ok], j] = 1.0
    Xd = torch.from_numpy(X).double()[None]
    e_d = dense_torch.segment_classifier(Xd, Ri, Ro, p_d, T, masks, trace=tr_d)[0]
    assert e_i.dtype == torch.float64 and e_i.shape == (E,)
    _close(e_i, e_d, "scores")
    for t in range(T + 1):
        _close(tr_i["e"][t], tr_d["e"][t][0], "e_trace[%d]" % t)
        _close(tr_i["H"][t], tr_d["H"][t][0], "H_trace[%d]" % t)
    if E == 0:
        return
    l_i = torch.nn.BCELoss()(e_i, y)
    l_d = torch.nn.BCELoss()(e_d, y)
    l_i.backward()
    l_d.backward()
    assert abs(l_i.item() - l_d.item()) <= REL * abs(l_d.item())
    for k in KEYS:
        _close(p_i[k].grad, p_d[k].grad, "grad " + k)
        if masked and k in masks:
            assert bool((p_i[k].grad[masks[k] == 0] == 0).all()), k


def test_index_torch_submodules_equal_the_dense_ones():
    """edge_network / node_network on their own (the oracle of the GPU submodule checks): values and the
    gradients of H, e and the four weights of each."""
    F, D = 3, 8
    X, src, dst = _graph("hub", F, seed=3)
    n, E = X.shape[0], src.shape[0]
    ok = src >= 0
    j = np.flatnonzero(ok)
    Ri = torch.zeros(1, n, E, dtype=torch.float64)
    Ro = torch.zeros(1, n, E, dtype=torch.float64)
    Ri[0, dst[ok], j] = 1.0
    Ro[0, src[ok], j] = 1.0
    p_i = _params(F, D, seed=1)
    p_d = {k: v.detach().clone().requires_grad_(True) for k, v in p_i.items()}
    H0 = torch.rand(n, F + D, dtype=torch.float64) * 2 - 1
    e0 = torch.rand(E, dtype=torch.float64)
    Hi, Hd = H0.clone().requires_grad_(True), H0.clone()[None].requires_grad_(True)
    ei, ed = e0.clone().requires_grad_(True), e0.clone()[None].requires_grad_(True)
    a = index_torch.edge_network(Hi, src, dst, p_i)
    b = dense_torch.edge_network(Hd, Ri, Ro, p_d)[0]
    _close(a, b, "edge_network")
    a2 = index_torch.node_network(Hi, ei, src, dst, p_i)
    b2 = dense_torch.node_network(Hd, ed, Ri, Ro, p_d)[0]
    _close(a2, b2, "node_network")
    w = torch.rand(a2.shape, dtype=torch.float64)
    ((a * torch.arange(E)).sum() + (a2 * w).sum()).backward()
    ((b * torch.arange(E)).sum() + (b2 * w).sum()).backward()
    _close(Hi.grad, Hd.grad[0], "grad H")
    _close(ei.grad, ed.grad[0], "grad e")
    for k in KEYS[2:]:
        _close(p_i[k].grad, p_d[k].grad, "grad " + k)


def _t(d):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in d.items()} if d else None


@pytest.mark.parametrize("name", SINGLE)
def test_index_torch_matches_reference(name):
    """Every single-graph golden fixture: scores and traces at the tolerances test_index_c_matches_reference uses."""
    fx = Fixture(name)
    tr = {}
    params = {k: v.double() for k, v in _t(fx.params).items()}
    masks = {k: v.double() for k, v in _t(fx.masks).items()} if fx.masks else None
    with torch.no_grad():
        e = index_torch.segment_classifier(fx.graph.X, fx.graph.src, fx.graph.dst, params, fx.n_iters, masks,
                                           trace=tr).numpy()
    tol = 2e-6
    assert np.abs(e - fx.scores).max() < tol
    if fx.e_trace is None:
        return
    for t in range(fx.n_iters + 1):
        assert np.abs(tr["e"][t].numpy() - fx.e_trace[t]).max() < tol
        assert np.abs(tr["H"][t].numpy() - fx.H_trace[t]).max() < 5e-6


@pytest.mark.parametrize("name", BATCHES)
def test_index_torch_training_step_matches_reference(name):
    """The reference's own training steps (gnn/estimator.py:49-60: BCELoss mean over all B x E_max entries of a
    zero-padded batch, padded ones included): each graph's padding as src = dst = -1 segments; loss at 1e-6 and
    all ten gradients at golden_util's bound."""
    fx = Fixture(name)
    Emax = fx.scores.shape[1]
    params = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in fx.params.items()}
    outs = []
    for g in fx.graphs:
        pad = -np.ones(Emax - g.src.shape[0], np.int32)
        outs.append(index_torch.segment_classifier(g.X, np.concatenate([g.src, pad]), np.concatenate([g.dst, pad]),
                                                   params, fx.n_iters))
    out = torch.stack(outs)
    assert np.abs(out.detach().numpy() - fx.scores).max() < 2e-6
    loss = torch.nn.BCELoss()(out, torch.from_numpy(fx.y).double())
    loss.backward()
    assert abs(loss.item() - fx.loss) < 1e-6
    for k in KEYS:
        assert_grad_close(params[k].grad, fx.grads[k], "index_torch golden step " + k)
