"""The hit classifier (gnn/MPNN_HitClassifier.ipynb cells 20-21) on the GPU: forward and training against the
reference's fixtures (tests/golden/node_classifier, written by tools/gen_nodeclf_golden.py from the notebook's own
classes and gnn/estimator.py) and against the fp64 restatement (tests/nodeclf_fp64.py), at the notebook's
configuration and at detector scale; the trunk shared with SegmentClassifier; reproducible gradients; evaluate();
and SegmentClassifier(input_dim=4), which the new input_dim-4 kernels make reachable."""
import glob
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import nodeclf_fp64 as ref64
from golden_util import assert_grad_close
from gnn_fpga_amd import HitGraphBatch, _lib, evaluate, synth
from gnn_fpga_amd.loss import BCELoss
from gnn_fpga_amd.metrics import segment_metrics_numpy
from gnn_fpga_amd.model import NodeClassifier, SegmentClassifier

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "node_classifier")
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, "*.npz")))
TOL_Y = 1e-5
TOL_H = 2e-5
DEV = torch.device("cuda:0")


def _fixture(case):
    return ref64.fixture(os.path.join(GOLD, case + ".npz"))


def _model(params, D, T):
    m = NodeClassifier(input_dim=4, hidden_dim=D, n_iters=T)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in params.items()})
    return m.to(DEV)


def _dense(fx):
    B, N, E = int(fx["B"]), int(fx["N"]), int(fx["E"])
    X = torch.from_numpy(fx["X"].reshape(B, N, 4))
    Ri = torch.zeros(B, N, E)
    Ro = torch.zeros(B, N, E)
    src, dst = fx["src"].reshape(B, E).astype(np.int64), fx["dst"].reshape(B, E).astype(np.int64)
    for b in range(B):
        ok = src[b] >= 0
        cols = np.flatnonzero(ok)
        Ro[b, src[b, ok] - b * N, cols] = 1
        Ri[b, dst[b, ok] - b * N, cols] = 1
    return [X.to(DEV), Ri.to(DEV), Ro.to(DEV)]


def _index_batch(fx):
    B, N = int(fx["B"]), int(fx["N"])
    return HitGraphBatch(fx["X"], fx["src"], fx["dst"], hit_ptr=np.arange(B + 1) * N,
                         seg_ptr=np.arange(B + 1) * int(fx["E"])).to(DEV)


def _params_of(m):
    return {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}


def _grads_of(m):
    return {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in m.named_parameters()}


# ---- forward -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_forward_matches_the_reference(hip, case):
    fx = _fixture(case)
    B, N, D, T = int(fx["B"]), int(fx["N"]), int(fx["hidden_dim"]), int(fx["n_iters"])
    m = _model(fx["params"], D, T).eval()
    with torch.no_grad():
        y_dense = m(_dense(fx))                                           # [B, N], every hit (padded ones too)
        y_index, H = m(_index_batch(fx), trace=True)
    assert tuple(y_dense.shape) == (B, N) and tuple(y_index.shape) == (B * N,)
    assert np.abs(y_dense.cpu().numpy() - fx["scores"]).max() < TOL_Y
    assert np.abs(y_index.cpu().numpy().reshape(B, N) - fx["scores"]).max() < TOL_Y
    H = H.cpu().numpy()
    for t in range(1, T + 1):
        if "H%d" % t in fx:
            assert np.abs(H[t, :, :D].reshape(B, N, D) - fx["H%d" % t]).max() < TOL_H, t


def _fp64_forward_check(graphs, D, T, seed):
    torch.manual_seed(seed)
    m = NodeClassifier(input_dim=4, hidden_dim=D, n_iters=T).to(DEV).eval()
    batch = HitGraphBatch.from_graphs(graphs).to(DEV)
    with torch.no_grad():
        y, H = m(batch, trace=True)
    X = np.concatenate([g.X for g in graphs])
    y64, H64 = ref64.forward(X, batch.src.cpu().numpy(), batch.dst.cpu().numpy(), _params_of(m), T)
    assert np.abs(y.cpu().numpy() - y64).max() < TOL_Y
    assert np.abs(H.cpu().numpy() - H64).max() < TOL_H


def test_forward_vs_fp64_notebook_configuration(hip):
    s = synth.hit_classifier_samples(32, seed=11)
    graphs = [synth.HitGraph(s.X[i], s.src, s.dst, np.zeros(225, np.float32)) for i in range(32)]
    _fp64_forward_check(graphs, 64, 7, seed=1)                           # 1 600 hits: k_node's epilogue


@pytest.mark.parametrize("D", [8, 64])
def test_forward_vs_fp64_detector_scale(hip, D):
    # 40 000 hits: past kNodeWideMinHits, so hidden_dim 64 scores its hits in k_node_mlpW's epilogue
    graphs = [synth.layered_graph(10000, 100000, 4, seed=40 + i) for i in range(4)]
    _fp64_forward_check(graphs, D, 3, seed=2)


def test_trunk_identical_to_segment_classifier(hip):
    graphs = [synth.layered_graph(3000, 20000, 4, seed=60 + i) for i in range(2)]
    batch = HitGraphBatch.from_graphs(graphs).to(DEV)
    for D in (8, 64):
        torch.manual_seed(D)
        n = NodeClassifier(input_dim=4, hidden_dim=D, n_iters=3).to(DEV).eval()
        s = SegmentClassifier(input_dim=4, hidden_dim=D, n_iters=3).to(DEV).eval()
        s.load_state_dict({k: v for k, v in n.state_dict().items() if not k.startswith("output_network")})
        with torch.no_grad():
            _, Hn = n(batch, trace=True)
            _, _, Hs = s(batch, trace=True)
        assert torch.equal(Hn, Hs), D


# ---- training ------------------------------------------------------------------------------------------------
def _check_grads(got, ref, what):
    for k in ref64.KEYS:
        assert_grad_close(got[k], ref[k], "%s %s" % (what, k))


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("loss_kind", ["torch", "hip"])
def test_training_step_matches_the_reference(hip, case, loss_kind):
    """The reference's training_step (gnn/estimator.py) replayed with the drop-in model: loss and twelve gradients
    against the fixture and against fp64."""
    fx = _fixture(case)
    D, T, l1 = int(fx["hidden_dim"]), int(fx["n_iters"]), float(fx["l1"])
    m = _model(fx["params"], D, T).train()
    inputs = _dense(fx)
    targets = torch.from_numpy(fx["y"]).to(DEV)
    loss_func = nn.BCELoss() if loss_kind == "torch" else BCELoss()
    # gnn/estimator.py training_step, statement for statement (the reference module is not importable here)
    m.zero_grad()
    outputs = m(inputs)
    node_w = [l.weight for l in m.node_network.network if hasattr(l, "weight")]
    edge_w = [l.weight for l in m.edge_network.network if hasattr(l, "weight")]
    l1_reg = l1 * sum([a.abs().sum() for a in node_w]) + l1 * sum([a.abs().sum() for a in edge_w])
    loss = loss_func(outputs, targets) + l1_reg
    loss.backward()
    assert abs(float(loss.item()) - float(fx["loss"])) < 1e-5
    got = _grads_of(m)
    _check_grads(got, fx["grads"], case + " vs reference")
    lo64, g64, _ = ref64.training_step(fx["X"], fx["src"], fx["dst"], fx["params"], T, fx["y"], l1)
    assert abs(float(loss.item()) - lo64) < 1e-5
    _check_grads(got, g64, case + " vs fp64")


def _lib_grads(m, batch, gy, keep_q):
    out = m.output_network[0]
    w = [t.detach().contiguous() for t in m.effective_weights()]
    Wo, bo = out.weight.detach().contiguous(), out.bias.detach().contiguous()
    e_all, H_all, Q_all, y = _lib.nodeclf_forward_train(batch, w, Wo, bo, 4, m.hidden_dim, m.n_iters, keep_q=keep_q)
    grads, gWo, gbo = _lib.nodeclf_backward(batch, w, Wo, bo, 4, m.hidden_dim, m.n_iters, e_all, H_all, y, gy,
                                            Q_all=Q_all)
    return y, dict(zip(ref64.KEYS, list(grads) + [gWo, gbo]))


@pytest.mark.parametrize("D,T", [(8, 0), (8, 1), (16, 1), (16, 7), (64, 1), (64, 7)])
@pytest.mark.parametrize("keep_q", [True, False])
def test_backward_vs_fp64_both_forms(hip, D, T, keep_q):
    """Every backward form starts from the seeded hit gradient: the pull form (hidden_dim <= 16, with and without
    the kept hidden layers), the wide loop (hidden_dim 64 with Q_all) and the per-pass form (without)."""
    graphs = [synth.layered_graph(3000, 20000, 4, seed=70 + i) for i in range(2)]
    batch = HitGraphBatch.from_graphs(graphs).to(DEV)
    torch.manual_seed(100 + D + T)
    m = NodeClassifier(input_dim=4, hidden_dim=D, n_iters=T).to(DEV)
    rng = np.random.default_rng(D * 10 + T)
    target = (rng.random(batch.n_hits) < 0.3).astype(np.float32)
    with torch.no_grad():
        y = m(batch)
    # dLoss/dy of the mean BCE, as torch forms it, fed to the backward
    yv = y.detach().clone().requires_grad_(True)
    nn.BCELoss()(yv, torch.from_numpy(target).to(DEV)).backward()
    y, got = _lib_grads(m, batch, yv.grad.contiguous(), keep_q)
    X = np.concatenate([g.X for g in graphs])
    _, g64, y64 = ref64.training_step(X, batch.src.cpu().numpy(), batch.dst.cpu().numpy(), _params_of(m), T, target)
    assert np.abs(y.cpu().numpy() - y64).max() < TOL_Y
    _check_grads(got, g64, "D=%d T=%d Q_all=%s" % (D, T, keep_q))


@pytest.mark.parametrize("D", [8, 64])
def test_gradients_bit_reproducible(hip, D):
    graphs = [synth.layered_graph(5000, 40000, 4, seed=80 + i) for i in range(2)]
    batch = HitGraphBatch.from_graphs(graphs).to(DEV)
    torch.manual_seed(D)
    m = NodeClassifier(input_dim=4, hidden_dim=D, n_iters=3).to(DEV)
    gy = torch.from_numpy(np.random.default_rng(D).standard_normal(batch.n_hits).astype(np.float32)).to(DEV)
    _, a = _lib_grads(m, batch, gy, True)
    _, b = _lib_grads(m, batch, gy, True)
    for k in ref64.KEYS:
        assert torch.equal(a[k], b[k]), k


def test_loss_backward_through_the_module(hip):
    """Adam steps through loss.backward() (the notebook's Estimator loop) lower the loss."""
    s = synth.hit_classifier_samples(32, seed=5)
    inputs = [torch.from_numpy(s.X).to(DEV), torch.from_numpy(s.Ri.astype(np.float32)).to(DEV),
              torch.from_numpy(s.Ro.astype(np.float32)).to(DEV)]
    y = torch.from_numpy(s.y.astype(np.float32)).to(DEV)
    torch.manual_seed(3)
    m = NodeClassifier(input_dim=4, hidden_dim=16, n_iters=2).to(DEV).train()
    opt = torch.optim.Adam(m.parameters())
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss = BCELoss()(m(inputs), y)
        loss.backward()
        opt.step()
        losses.append(float(loss.item()))
    assert losses[-1] < losses[0]


# ---- metrics -------------------------------------------------------------------------------------------------
def test_evaluate_counts_every_hit(hip):
    s = synth.hit_classifier_samples(16, seed=9)
    torch.manual_seed(4)
    m = NodeClassifier(input_dim=4, hidden_dim=8, n_iters=2).to(DEV)

    def gen():
        for b in range(4):
            sl = slice(4 * b, 4 * b + 4)
            yield ([torch.from_numpy(s.X[sl]).to(DEV), torch.from_numpy(s.Ri[sl].astype(np.float32)).to(DEV),
                    torch.from_numpy(s.Ro[sl].astype(np.float32)).to(DEV)],
                   torch.from_numpy(s.y[sl].astype(np.float32)).to(DEV))
    th = (0.3, 0.5, 0.7)
    met = evaluate(m, gen(), 4, thresholds=th)
    scores = []
    with torch.no_grad():
        for inp, _ in gen():
            scores.append(m(inp).cpu().numpy())
    spec = segment_metrics_numpy(np.concatenate(scores).reshape(-1), s.y.reshape(-1).astype(np.float32), th)
    status, counts, hist = met._views()
    assert int(status.item()) == 0
    assert np.array_equal(counts.cpu().numpy(), spec["counts"]) and int(spec["counts"][0].sum()) == 16 * 50
    assert np.array_equal(hist.cpu().numpy(), spec["hist"])


# ---- SegmentClassifier(input_dim=4): reachable through the new shapes ------------------------------------------
@pytest.mark.parametrize("events", [False, True])
def test_segment_classifier_input_dim_4(hip, events):
    if events:
        graphs = [synth.layered_graph(40, 150, 4, seed=90 + i) for i in range(8)]        # the one-launch forward
    else:
        graphs = [synth.layered_graph(3000, 20000, 4, seed=95 + i) for i in range(2)]    # per-module kernels
    batch = HitGraphBatch.from_graphs(graphs).to(DEV)
    X = np.concatenate([g.X for g in graphs])
    src, dst = batch.src.cpu().numpy(), batch.dst.cpu().numpy()
    for D in (8, 16):
        torch.manual_seed(D)
        s = SegmentClassifier(input_dim=4, hidden_dim=D, n_iters=2).to(DEV)
        s.use_events = events
        params = _params_of(s)
        with torch.no_grad():
            e = s.eval()(batch).cpu().numpy()
        assert np.abs(e - ref64.segclf_forward(X, src, dst, params, 2)).max() < TOL_Y
        y = np.concatenate([g.y for g in graphs]).astype(np.float32)
        s.train().zero_grad()
        nn.BCELoss()(s(batch), torch.from_numpy(y).to(DEV)).backward()
        _, g64 = ref64.segclf_training_step(X, src, dst, params, 2, y)
        for k, p in s.named_parameters():
            assert_grad_close(p.grad, g64[k], "segclf F=4 D=%d %s" % (D, k))
