"""GPU checks of the graph-convolution classifiers (csrc/gcn.hip, gnn_fpga_amd/gcn.py) against fp64.

Tolerance: a GPU result is compared with the fp64 value of the same model on the same fp32 data, the error taken
relative to the tensor's largest entry.  The bound is 4 x the reference's own fp32 distance from fp64 on the same data
(`ref_err_*` of a fixture; the CPU fp32 dense restatement's distance, computed here, for a synthetic case): the kernels
sum in list order and torch's matmul in its own, two independent fp32 roundings of one value.  Its floor is 16 fp32
ulp (9.6e-7), for tensors where the reference happens to land exactly.  Every figure is printed before it is
asserted (run with -s to see them).  A bound of this kind cannot see ONE dropped, doubled or misindexed list entry where
the lists are long: tests/test_gpu_gcn_exact.py is the check that does, bit for bit on integer-exact inputs."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import gcn_fp64 as ref
from gnn_fpga_amd import synth
from gnn_fpga_amd.autograd import gcn_forward_layers
from gnn_fpga_amd.gcn import (GCNBinaryClassifier, GCRNBinaryClassifier, GraphConv, GraphConvSelfInt, SparseAdjacency,
                              compress_adjacency)

pytestmark = pytest.mark.gpu
CASES = ref.fixture_names()
_FIX = {}


def fixture(case):
    if case not in _FIX:
        _FIX[case] = ref.load_fixture(case)
    return _FIX[case]


def package_model(kind, conv, F, dims, state=None, dev="cuda"):
    cls = GCRNBinaryClassifier if kind == "gcrn" else GCNBinaryClassifier
    m = cls(F, dims, gc_type=GraphConvSelfInt if conv == "selfint" else GraphConv)
    if state is not None:
        m.load_state_dict(state)
    return m.to(dev)


def train_step(m, x, a, y):
    """forward + BCEWithLogitsLoss + backward as the notebooks' training_step does: (logits, loss, {name: grad})."""
    m.train()
    m.zero_grad()
    out = m(x, a)
    loss = nn.BCEWithLogitsLoss()(out, y)
    loss.backward()
    return (out.detach().cpu().numpy(), float(loss.item()),
            {n: p.grad.detach().cpu().numpy().copy() for n, p in m.named_parameters()})


def check(what, got, want, ref_err):
    err, b = ref.rel_err(got, want), ref.bound(ref_err)
    print("  %-44s err %.3e  bound %.3e  (reference's own %.3e)" % (what, err, b, float(ref_err)))
    return [] if err <= b else ["%s: %.3e > %.3e" % (what, err, b)]


# ---- the reference's fixtures ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["dense", "compressed"])
@pytest.mark.parametrize("case", CASES)
def test_fixture(hip, case, form):
    d = fixture(case)
    dev = torch.device("cuda")
    state = ref.fixture_model(d).state_dict()
    m = package_model(d["kind"], d["conv"], d["X"].shape[-1], d["hidden_dims"], state)
    x, y = torch.from_numpy(d["X"]).to(dev), torch.from_numpy(d["y"]).to(dev)
    a = torch.from_numpy(d["A"]).to(dev)
    if form == "compressed":
        a = compress_adjacency(a)
    print("\n%s (%s input)" % (case, form))
    logits, loss, grads = train_step(m, x, a, y)
    bad = check("logits", logits, d["logits64"], d["ref_err_logits"])
    bad += check("loss", loss, d["loss64"], d["ref_err_loss"])
    for k in d["keys"]:
        bad += check("grad " + str(k), grads[str(k)], d["grad64/" + str(k)], d["ref_err_grad/" + str(k)])
    out2, hs = gcn_forward_layers(m, x, a)
    assert np.array_equal(out2.cpu().numpy(), logits)
    for l in range(len(d["hidden_dims"])):
        if "h64_%d" % l in d:
            bad += check("h of layer %d" % l, hs[l].cpu().numpy(), d["h64_%d" % l], d["ref_err_h%d" % l])
    with torch.no_grad():                                        # the inference launch keeps no h: the same logits
        assert np.array_equal(m.eval()(x, a).cpu().numpy(), logits)
    assert not bad, bad


def test_state_dict_round_trip(hip, tmp_path):
    d = fixture("hits_gcrn_selfint_8x12_b8")
    m = package_model(d["kind"], d["conv"], 3, d["hidden_dims"], ref.fixture_model(d).state_dict())
    torch.save(m.state_dict(), tmp_path / "gcrn.pt")
    m2 = package_model(d["kind"], d["conv"], 3, d["hidden_dims"])
    m2.load_state_dict(torch.load(tmp_path / "gcrn.pt"))
    x, a = torch.from_numpy(d["X"]).cuda(), torch.from_numpy(d["A"]).cuda()
    with torch.no_grad():
        out = m2.eval()(x, a).cpu().numpy()
    assert not check("logits", out, d["logits64"], d["ref_err_logits"])


# ---- compress_adjacency ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["seg_gcn_selfint_16x5_b4", "hits_gcrn_selfint_8x12_b8", "hits_kw_gcn_graphconv_8x3_b3"])
def test_compress_round_trip_fixture(hip, case):
    a = torch.from_numpy(fixture(case)["A"]).cuda()
    adj = compress_adjacency(a)
    assert isinstance(adj, SparseAdjacency) and len(adj) == a.shape[0] and adj.shape == tuple(a.shape)
    assert adj.width == int(max((a != 0).sum(-1).max(), (a != 0).sum(-2).max()))
    assert torch.equal(adj.to_dense(), a) and torch.equal(adj.to_dense(transposed=True), a)
    assert torch.equal(adj.row_cnt, (a != 0).sum(-1).int()) and torch.equal(adj.col_cnt, (a != 0).sum(-2).int())


@pytest.mark.parametrize("N,B", [(1, 1), (37, 3), (64, 33), (65, 3), (257, 3)])
def test_compress_round_trip_synthetic(hip, N, B):
    rng = np.random.default_rng(N * 100 + B)
    A = ((rng.random((B, N, N)) < 0.2) * rng.normal(size=(B, N, N))).astype(np.float32)
    A[:, N // 2, :] = rng.normal(size=(B, N))                   # a full row and a full column: list width = N
    A[:, :, N // 3] = rng.normal(size=(B, N))
    A[0, 0, 0] = -0.0                                           # not an entry: comes back as +0.0
    a = torch.from_numpy(A).cuda()
    adj = compress_adjacency(a)
    assert adj.width == N
    dense = adj.to_dense()
    assert torch.equal(dense.view(torch.int32), (a + 0.0).view(torch.int32))            # bit for bit
    assert not torch.signbit(dense[0, 0, 0])
    assert torch.equal(adj.to_dense(transposed=True), dense)
    k = torch.arange(N, device="cuda").view(1, 1, N)
    asc = (adj.row_idx[:, :, 1:] > adj.row_idx[:, :, :-1]) | (k[:, :, 1:] >= adj.row_cnt.unsqueeze(-1))
    assert bool(asc.all())                                      # ascending index within every list
    asc = (adj.col_idx[:, :, 1:] > adj.col_idx[:, :, :-1]) | (k[:, :, 1:] >= adj.col_cnt.unsqueeze(-1))
    assert bool(asc.all())


def test_compress_all_zero_and_empty_lists(hip):
    adj = compress_adjacency(torch.zeros(3, 37, 37, device="cuda"))
    assert adj.width == 1 and int(adj.row_cnt.sum()) == 0 and int(adj.col_cnt.sum()) == 0
    assert not adj.to_dense().any()


def test_compress_past_2g_elements(hip):
    """B N N > 2^31 elements: the entry offsets need 64 bits."""
    B, N = 32800, 257
    assert B * N * N > 2 ** 31
    a = torch.zeros(B, N, N, device="cuda")
    a[B - 1, N - 1, 5], a[B - 1, 3, N - 1], a[B - 2, 7, 7], a[0, 1, 2] = 1.5, -2.5, 3.5, 4.5
    adj = compress_adjacency(a)
    assert adj.width == 1 and int(adj.row_cnt.sum()) == 4 and int(adj.col_cnt.sum()) == 4
    assert torch.equal(adj[B - 2:].to_dense(), a[B - 2:]) and torch.equal(adj[:1].to_dense(transposed=True), a[:1])


def test_slice_is_a_view_and_scores_identically(hip):
    d = fixture("hits_gcrn_selfint_8x12_b8")
    m = package_model(d["kind"], d["conv"], 3, d["hidden_dims"], ref.fixture_model(d).state_dict())
    x, y = torch.from_numpy(d["X"]).cuda(), torch.from_numpy(d["y"]).cuda()
    a = torch.from_numpy(d["A"]).cuda()
    adj = compress_adjacency(a)
    part = adj[2:5]
    assert part.row_idx.data_ptr() == adj.row_idx[2].data_ptr() and len(part) == 3
    own = compress_adjacency(a[2:5].contiguous())
    l1, loss1, g1 = train_step(m, x[2:5], part, y[2:5])
    l2, loss2, g2 = train_step(m, x[2:5], own, y[2:5])
    assert np.array_equal(l1, l2) and loss1 == loss2
    for k in g1:
        assert np.array_equal(g1[k], g2[k]), k
    with torch.no_grad():
        whole = m.eval()(x, adj).cpu().numpy()
    assert np.array_equal(whole[2:5], l1)                       # a graph's logits do not depend on its batch


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_adjacency_raises(hip, value):
    a = torch.from_numpy(fixture("hits_gcn_selfint_8_8_b1")["A"]).cuda().clone()
    a[0, 3, 4] = value
    with pytest.raises(ValueError, match="non-finite"):
        compress_adjacency(a)
    m = package_model("gcn", "selfint", 3, [8, 8])
    with pytest.raises(ValueError, match="non-finite"):         # the dense (slow) form goes through the same check
        m(torch.zeros(1, 40, 3, device="cuda"), a)


# ---- synthetic shapes against the restatement --------------------------------------------------------------------------
CONFIGS = [("gcn", "selfint", [8, 12, 16]), ("gcrn", "graphconv", [8, 12, 16]),
           ("gcrn", "selfint", [64, 64]), ("gcn", "graphconv", [64, 64])]
_REF = {}


def synthetic(N, B, zero=False):
    """x, A, y: A unsymmetric with negative weights, a diagonal, one fully dense row and one fully dense column
    (list width = N); entries scaled so that a row sum stays O(1)."""
    rng = np.random.default_rng(1000 * N + B)
    A = (rng.random((B, N, N)) < min(1.0, 6.0 / N)) * rng.normal(size=(B, N, N))
    A[:, N // 2, :] = rng.normal(size=(B, N)) / np.sqrt(N)
    A[:, :, N // 3] = rng.normal(size=(B, N)) / np.sqrt(N)
    i = np.arange(N)
    A[:, i, i] = rng.normal(size=(B, N))
    if zero:
        A[:] = 0
    x = rng.normal(size=(B, N, 3)).astype(np.float32)
    y = (rng.random((B, N)) < 0.3).astype(np.float32)
    return x, A.astype(np.float32), y


def reference(N, B, cfg, zero=False):
    """The restatement in fp64 and fp32 on the CPU, computed once per case and left unchanged."""
    key = (N, B, cfg, zero)
    if key not in _REF:
        kind, conv, dims = CONFIGS[cfg]
        x, A, y = synthetic(N, B, zero)
        torch.manual_seed(7 + cfg)
        model = ref.DenseGCN(3, dims, kind, conv)
        _REF[key] = (x, A, y, model.state_dict(), ref.run(model, x, A, y, torch.float64),
                     ref.run(model, x, A, y, torch.float32))
    return _REF[key]


def run_synthetic(N, B, cfg, zero=False, compressed=True):
    kind, conv, dims = CONFIGS[cfg]
    x, A, y, state, r64, r32 = reference(N, B, cfg, zero)
    m = package_model(kind, conv, 3, dims, state)
    xt, yt, a = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(A).cuda()
    if compressed:
        a = compress_adjacency(a)
        assert a.width == (1 if zero else N)
    print("\nN=%d B=%d %s %s %s%s" % (N, B, kind, conv, dims, " A=0" if zero else ""))
    logits, loss, grads = train_step(m, xt, a, yt)
    bad = check("logits", logits, r64["logits"], ref.rel_err(r32["logits"], r64["logits"]))
    bad += check("loss", loss, r64["loss"], ref.rel_err(r32["loss"], r64["loss"]))
    for k, g in r64["grads"].items():
        bad += check("grad " + k, grads[k], g, ref.rel_err(r32["grads"][k], g))
    return bad


@pytest.mark.parametrize("cfg", range(len(CONFIGS)))
@pytest.mark.parametrize("B", [1, 3, 33])
@pytest.mark.parametrize("N", [1, 37, 64, 65, 257])
def test_synthetic_shapes(hip, N, B, cfg):
    assert not run_synthetic(N, B, cfg)


@pytest.mark.parametrize("N,B,cfg", [(37, 3, 0), (1, 1, 1), (65, 3, 2), (64, 1, 3)])
def test_all_zero_adjacency(hip, N, B, cfg):
    assert not run_synthetic(N, B, cfg, zero=True)


def test_dense_input_equals_compressed(hip):
    assert not run_synthetic(37, 3, 2, compressed=False)
    x, A, y, state, _, _ = reference(37, 3, 2)
    m = package_model("gcrn", "selfint", 3, [64, 64], state)
    xt, yt, a = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(A).cuda()
    l1, loss1, g1 = train_step(m, xt, a, yt)
    l2, loss2, g2 = train_step(m, xt, compress_adjacency(a), yt)
    assert np.array_equal(l1, l2) and all(np.array_equal(g1[k], g2[k]) for k in g1)


@pytest.mark.parametrize("dims,kind", [([8], "gcn"), ([16], "gcrn"), ([5, 7, 3], "gcrn"), ([8] * 17, "gcrn")])
def test_layer_counts_and_odd_widths(hip, dims, kind):
    """No graph-convolution layer at all, widths that are no power of two, and the most layers the kernels take."""
    x, A, y = synth.toy_hit_graphs(3, seed=11, norm="kw" if len(dims) > 12 else "row")
    torch.manual_seed(3)
    model = ref.DenseGCN(3, dims, kind, "selfint")
    r64, r32 = ref.run(model, x, A, y, torch.float64), ref.run(model, x, A, y, torch.float32)
    m = package_model(kind, "selfint", 3, dims, model.state_dict())
    print("\n%s %s" % (kind, dims))
    logits, loss, grads = train_step(m, torch.from_numpy(x).cuda(), torch.from_numpy(A).cuda(),
                                     torch.from_numpy(y).cuda())
    bad = check("logits", logits, r64["logits"], ref.rel_err(r32["logits"], r64["logits"]))
    for k, g in r64["grads"].items():
        bad += check("grad " + k, grads[k], g, ref.rel_err(r32["grads"][k], g))
    assert not bad, bad


# ---- properties of the training step -----------------------------------------------------------------------------------
def test_two_identical_steps_give_identical_bits(hip):
    x, A, y, state, _, _ = reference(65, 33, 2)
    m = package_model("gcrn", "selfint", 3, [64, 64], state)
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    adj = compress_adjacency(torch.from_numpy(A).cuda())
    l1, loss1, g1 = train_step(m, xt, adj, yt)
    l2, loss2, g2 = train_step(m, xt, adj, yt)
    assert np.array_equal(l1, l2) and loss1 == loss2
    for k in g1:
        assert np.array_equal(g1[k].view(np.int32), g2[k].view(np.int32)), k


def test_batch_gradient_is_the_sum_of_the_graphs(hip):
    N, B, cfg = 37, 3, 0
    kind, conv, dims = CONFIGS[cfg]
    x, A, y, state, r64, r32 = reference(N, B, cfg)
    m = package_model(kind, conv, 3, dims, state)
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    adj = compress_adjacency(torch.from_numpy(A).cuda())
    _, _, whole = train_step(m, xt, adj, yt)
    total = {k: np.zeros_like(v, dtype=np.float64) for k, v in whole.items()}
    for b in range(B):
        m.zero_grad()
        out = m(xt[b:b + 1], adj[b:b + 1])
        (nn.BCEWithLogitsLoss(reduction="sum")(out, yt[b:b + 1]) / (B * N)).backward()
        for k, p in m.named_parameters():
            total[k] += p.grad.detach().cpu().numpy()
    bad = []
    for k in whole:
        bad += check("grad " + k, total[k], whole[k], ref.rel_err(r32["grads"][k], r64["grads"][k]))
    assert not bad, bad


def test_unsupported_shape_names_the_limit(hip):
    m = package_model("gcn", "selfint", 3, [64, 64])
    x, a = torch.zeros(1, 600, 3, device="cuda"), torch.zeros(1, 600, 600, device="cuda")
    with pytest.raises(RuntimeError, match="163840 bytes"):
        m(x, a)
    with torch.no_grad(), pytest.raises(RuntimeError, match="LDS"):
        m.eval()(x, compress_adjacency(a))
    deep = package_model("gcn", "selfint", 3, [4] * 18)
    with pytest.raises(RuntimeError, match="at most 16"):
        deep(torch.zeros(1, 8, 3, device="cuda"), torch.zeros(1, 8, 8, device="cuda"))


def test_inputs_that_require_grad_raise(hip):
    m = package_model("gcn", "selfint", 3, [8, 8])
    x, a = torch.zeros(2, 40, 3, device="cuda"), torch.zeros(2, 40, 40, device="cuda")
    with pytest.raises(RuntimeError, match="requires grad"):
        m(x.clone().requires_grad_(), a)
    with pytest.raises(RuntimeError, match="requires grad"):
        m(x, a.clone().requires_grad_())
    with pytest.raises(RuntimeError):                           # shapes that do not belong together
        m(x[:1], a)


def test_adam_lowers_the_loss(hip):
    """The notebook's training loop (Seg cells 27-28) for 20 steps on one batch of synthetic segment graphs."""
    X, A, y = synth.toy_segment_graphs(8, seed=5)
    torch.manual_seed(0)
    m = GCNBinaryClassifier(5, [16] * 5).cuda()
    opt = torch.optim.Adam(m.parameters())
    loss_func = nn.BCEWithLogitsLoss()
    x, yt = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    adj = compress_adjacency(torch.from_numpy(A).cuda())
    losses = []
    for _ in range(20):
        m.train()
        m.zero_grad()
        loss = loss_func(m(x, adj), yt)
        loss.backward()
        opt.step()
        losses.append(float(loss.item()))
    print("\nloss %.4f -> %.4f" % (losses[0], losses[-1]))
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
