"""csrc/iter_events.hip at every shape it is built for (tests/toy_mpnn_cases.py MATRIX), on ragged and padded batches, by
both routes, against the fp64 restatement; one graph's independence of its batch, bit for bit; the counts no other test
launches (graphs without hits, EVENTS_MAX_GRAPHS graphs, n_iters 0 and 1); and a NaN that stays in its graph.

Bounds are the project's (tests/toy_mpnn_fp64.py): SCORE_BOUND for scores and every e_t / H_t, grad_bound(the reference's
own fp32 error) for the loss and every gradient tensor separately.  Every figure is printed before it is asserted (run
with -s); the worst per shape and route are printed once more when the module ends (profiles/toy_mpnn_shapes.txt)."""
import numpy as np
import pytest
import torch

import nonfinite_cases as nf
import toy_mpnn_fp64 as ref
from gnn_fpga_amd import HitGraphBatch, synth
from gnn_fpga_amd.call_route import EVENTS_MAX_GRAPHS
from gnn_fpga_amd.loss import BCELoss
from test_gpu_uninitialised import check
from toy_mpnn_cases import (MATRIX, MATRIX_T, check_abs, check_graphs, check_rel, host_arrays, matrix_batch,
                            matrix_graphs, matrix_reference, model_of, random_graph, random_params, train_step)

pytestmark = pytest.mark.gpu
ROUTES = ("iter_events", "per_module")
WORST = {}          # (F, D, route) -> {"score" | "trace" | "grad / bound": worst figure}


def _note(key, kind, value):
    w = WORST.setdefault(key, {})
    w[kind] = max(w.get(kind, 0.0), value)


@pytest.fixture(scope="module", autouse=True)
def worst_figures():
    yield
    if WORST:
        print("\n  worst figures per shape and route: |score - fp64| and |e_t, H_t - fp64| (bound %.0e), largest "
              "gradient or loss error over its bound (1 = at the bound)" % ref.SCORE_BOUND)
        for (F, D, route), w in sorted(WORST.items()):
            print("  (%2d, %2d) %-11s score %.2e  trace %.2e  grad/bound %.3f" % (
                F, D, route, w.get("score", 0.0), w.get("trace", 0.0), w.get("grad", 0.0)))


def _abs(key, kind, what, got, want):
    if np.size(want):
        _note(key, kind, float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max()))
    return check_abs(what, got, want)


def _rel(key, what, got, want, own):
    _note(key, "grad", ref.rel_err(got, want) / ref.grad_bound(own))
    return check_rel(what, got, want, own)


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. the shape matrix -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("kind", ["ragged", "padded"])
@pytest.mark.parametrize("shared", [False, True], ids=["own_sets", "shared"])
@pytest.mark.parametrize("F,D", MATRIX)
def test_matrix(hip, F, D, shared, kind, route):
    T, C, key = MATRIX_T, F + D, (F, D, route)
    params, r64, own = matrix_reference(F, D, shared, kind)
    batch = matrix_batch(F, D, kind).to("cuda")
    m = model_of(params, F, D, T, shared, events=route == "iter_events")
    form = (batch.dense_shape[0], batch.dense_shape[2]) if kind == "padded" else (batch.n_segments,)
    assert (kind == "padded") == (batch.dense_shape is not None)
    bad = []
    with torch.no_grad():
        plain = m.eval()(batch)
        assert m._route.kind == route
        e, et, Ht = m(batch, trace=True)
        assert m._route.kind == route
    assert tuple(plain.shape) == form and tuple(e.shape) == form
    assert tuple(et.shape) == (T + 1, batch.n_segments) and tuple(Ht.shape) == (T + 1, batch.n_hits, C)
    bad += _abs(key, "score", "scores", plain.cpu().numpy().reshape(-1), r64["e"][T])
    bad += _abs(key, "score", "traced scores", e.cpu().numpy().reshape(-1), r64["e"][T])
    for t in range(T + 1):
        bad += _abs(key, "trace", "e_%d" % t, et[t].cpu().numpy(), r64["e"][t])
        bad += _abs(key, "trace", "H_%d" % t, Ht[t].cpu().numpy(), r64["H"][t])
    out, loss, grads = train_step(m, batch, batch.y)
    assert m._route.kind == route
    bad += _abs(key, "score", "training scores", out.cpu().numpy(), r64["e"][T])
    bad += _rel(key, "loss", loss, r64["loss"], own["loss"])
    assert list(grads) == list(params)
    for k in params:
        bad += _rel(key, "grad " + k, grads[k], r64["grads"][k], own[k])
    assert not bad, "\n".join(bad)


# ---- 2. one graph is one workgroup's business --------------------------------------------------------------------------
ISOLATION_SHAPES = [(2, 32), (4, 8), (11, 16), (3, 4)]


def _isolation_batches(F):
    """[(name, graphs, place of g, pad_segments)]: g = (17 hits, 33 segments) alone, at three places among four graphs,
    beside a (40, 144) graph - larger caps move every LDS offset - and in a padded batch, trailing -1 segments behind it."""
    rng = np.random.default_rng(700 + F)
    g = random_graph(rng, 17, 33, F)
    a, b, c = random_graph(rng, 12, 20, F), random_graph(rng, 25, 60, F), random_graph(rng, 5, 6, F)
    big = random_graph(rng, 40, 144, F)
    return g, [("alone", [g], 0, False), ("first of four", [g, a, b, c], 0, False),
               ("middle of four", [a, g, b, c], 1, False), ("last of four", [a, b, c, g], 3, False),
               ("beside a larger graph", [g, big], 0, False), ("after a larger graph", [big, g], 1, False),
               ("padded", [g, big], 0, True), ("padded, moved", [b, big, g], 2, True)]


def _own_rows(batch, i, n_seg):
    hp, sp = np.asarray(batch.hit_ptr), np.asarray(batch.seg_ptr)
    return slice(int(hp[i]), int(hp[i + 1])), slice(int(sp[i]), int(sp[i]) + n_seg)


@pytest.mark.parametrize("F,D", ISOLATION_SHAPES)
def test_forward_of_a_graph_does_not_depend_on_its_batch(hip, F, D):
    T = 2
    m = model_of(random_params(F, D, T, False, 31 * F + D), F, D, T, False).eval()
    g, cases = _isolation_batches(F)
    want = None
    for name, graphs, i, pad in cases:
        batch = HitGraphBatch.from_graphs(graphs, pad_segments=pad).to("cuda")
        hits, segs = _own_rows(batch, i, 33)
        with torch.no_grad():
            e, et, Ht = m(batch, trace=True)
            plain = m(batch)
        assert m._route.kind == "iter_events"
        got = [_bits(e.reshape(-1)[segs]), _bits(plain.reshape(-1)[segs]), _bits(et[:, segs]), _bits(Ht[:, hits])]
        if want is None:
            want = got
            assert got[2].shape == (T + 1, 33) and got[3].shape == (T + 1, 17, F + D)
            assert np.isfinite(et.cpu().numpy()).all() and np.isfinite(Ht.cpu().numpy()).all()
        for what, a, b in zip(("traced scores", "scores", "e_t", "H_t"), want, got):
            same = np.array_equal(a, b)
            print("  (%d, %d) %-22s %-14s %s" % (F, D, name, what, "same bits" if same else "DIFFERS in %d of %d" % (
                int((a != b).sum()), a.size)))
            assert same, (name, what)


@pytest.mark.parametrize("F,D", ISOLATION_SHAPES)
def test_backward_of_a_graph_does_not_depend_on_its_batch(hip, F, D):
    """gnn_iter_backward_events with an upstream gradient that is zero on every other graph's segments (and on g's own
    padded ones): every product of the other workgroups is an exact zero, so the flat gradient EQUALS the gradient of
    g alone, element for element (np.array_equal on values: -0.0 equals 0.0)."""
    T = 2
    m = model_of(random_params(F, D, T, False, 31 * F + D), F, D, T, False)
    ip = m._iter_params([p.detach() for p in m.parameters()])
    g, cases = _isolation_batches(F)
    go_own = torch.rand(33, generator=torch.Generator().manual_seed(F + D)) - 0.5
    want = None
    for name, graphs, i, pad in cases:
        batch = HitGraphBatch.from_graphs(graphs, pad_segments=pad).to("cuda")
        lay = batch.event_layout()
        assert lay is not None and hip.iter_events_supported(F, D, lay.max_hits, lay.max_segments, True)
        _, segs = _own_rows(batch, i, 33)
        go = torch.zeros(batch.n_segments)
        go[segs] = go_own
        e_all, H_all = hip.iter_forward_events(batch, lay, ip, train=True)
        flat = hip.iter_backward_events(batch, lay, ip, e_all, H_all, go.cuda()).cpu().numpy()
        if want is None:
            want = flat
            assert np.isfinite(flat).all() and np.count_nonzero(flat) > flat.size // 2
        diff = int((flat != want).sum())
        print("  (%d, %d) %-22s flat gradient: %d of %d elements differ from the graph alone" % (F, D, name, diff, flat.size))
        assert np.array_equal(flat, want), name


@pytest.mark.parametrize("shared", [False, True], ids=["own_sets", "shared"])
@pytest.mark.parametrize("F,D", MATRIX)
def test_both_routes_give_the_same_forward_bits(hip, F, D, shared):
    """include/gnn_hip_iter.h: "the arithmetic per row is that of gnn_input_fwd / gnn_edge_fwd / gnn_node_fwd" - k
    ascending from the bias, sums in list order - so scores, e_t and H_t of the two routes have the same bits.  (Not the
    gradients: the routes fold their partial sums in different orders.)"""
    T = MATRIX_T
    params, _, _ = matrix_reference(F, D, shared, "ragged")
    batch = matrix_batch(F, D, "ragged").to("cuda")
    outs = {}
    for route in ROUTES:
        m = model_of(params, F, D, T, shared, events=route == "iter_events").eval()
        with torch.no_grad():
            outs[route] = m(batch, trace=True)
        assert m._route.kind == route
    bad = []
    for what, a, b in zip(("scores", "e_t", "H_t"), outs["iter_events"], outs["per_module"]):
        a, b = _bits(a), _bits(b)
        print("  (%d, %d) %-6s %d of %d elements differ between the routes" % (F, D, what, int((a != b).sum()), a.size))
        if not np.array_equal(a, b):
            bad.append(what)
    assert not bad, bad


# ---- 3. counts nobody launches -----------------------------------------------------------------------------------------
def _no_hits(F):
    return synth.HitGraph(np.zeros((0, F), np.float32), np.zeros(0, np.int32), np.zeros(0, np.int32),
                          np.zeros(0, np.float32))


@pytest.mark.parametrize("order", ["gzg", "zg", "gz"])
@pytest.mark.parametrize("F,D", [(2, 8), (3, 32)])
def test_graphs_without_hits_among_others(hip, F, D, order):
    rng = np.random.default_rng(800 + D)
    graphs = [random_graph(rng, 17, 33, F) if c == "g" else _no_hits(F) for c in order]
    check_graphs(hip, graphs, F, D, 2, "iter_events", "iter_events", seed=D)


@pytest.mark.parametrize("shared", [False, True], ids=["own_sets", "shared"])
@pytest.mark.parametrize("F,D", [(2, 8), (3, 32)])
def test_a_batch_of_one_graph_without_hits(hip, F, D, shared):
    """[z] through the entry points themselves: no score, and every float of the flat gradient written - 0.0 - on a
    workspace and a gradient buffer that held NaN (the poison of test_gpu_uninitialised.check: all-ones bytes)."""
    T = 2
    m = model_of(random_params(F, D, T, shared, D), F, D, T, shared)
    ip = m._iter_params([p.detach() for p in m.parameters()])
    batch = HitGraphBatch.from_graphs([_no_hits(F)]).to("cuda")
    lay = batch.event_layout()
    assert lay is not None and (batch.n_graphs, batch.n_hits, batch.n_segments) == (1, 0, 0)

    def call():
        scores = hip.iter_forward_events(batch, lay, ip)
        e_all, H_all = hip.iter_forward_events(batch, lay, ip, train=True)
        flat = hip.iter_backward_events(batch, lay, ip, e_all, H_all, torch.zeros(0, device="cuda"))
        return [scores, e_all, H_all, flat]
    scores, e_all, H_all, flat = check(call)
    assert scores.numel() == 0 and tuple(e_all.shape) == (T + 1, 0) and H_all.numel() == 0
    assert flat.numel() == sum(p.numel() for p in m.parameters())
    assert not flat.cpu().numpy().any(), "a gradient without a hit must be 0.0 everywhere"
    with torch.no_grad():
        assert m.eval()(batch).numel() == 0 and m._route.kind == "iter_events"
    m.train()
    m.zero_grad()
    out = m(batch)
    out.sum().backward()
    assert m._route.kind == "iter_events" and out.numel() == 0
    assert all(p.grad is not None and not p.grad.cpu().numpy().any() for p in m.parameters())


@pytest.mark.parametrize("F,D", [(2, 8), (3, 32)])
def test_a_batch_without_segments(hip, F, D):
    """Hits and no segment at all: no score (the e_all handed to the entry points has no element), every H_t within the
    score bound of fp64, and a gradient of zeros."""
    T = 2
    params = random_params(F, D, T, False, D)
    g = random_graph(np.random.default_rng(850 + D), 9, 0, F)
    batch = HitGraphBatch.from_graphs([g]).to("cuda")
    r64 = ref.run(params, g.X, g.src, g.dst, None, T)
    m = model_of(params, F, D, T, False).eval()
    with torch.no_grad():
        e, et, Ht = m(batch, trace=True)
        assert m._route.kind == "iter_events" and m(batch).numel() == 0
    assert e.numel() == 0 and tuple(et.shape) == (T + 1, 0) and tuple(Ht.shape) == (T + 1, 9, F + D)
    bad = []
    for t in range(T + 1):
        bad += check_abs("H_%d" % t, Ht[t].cpu().numpy(), r64["H"][t])
    assert not bad, "\n".join(bad)
    m.train()
    m.zero_grad()
    m(batch).sum().backward()
    assert m._route.kind == "iter_events"
    assert all(p.grad is not None and not p.grad.cpu().numpy().any() for p in m.parameters())


@pytest.mark.parametrize("F,D,T,shared", [(2, 8, 1, False), (2, 32, 2, True)])
def test_as_many_graphs_as_the_one_launch_route_takes(hip, F, D, T, shared):
    """Exactly EVENTS_MAX_GRAPHS graphs: the fold adds 1 024 rows per element (and, shared, the passes too)."""
    rng = np.random.default_rng(900 + D)
    graphs = [random_graph(rng, 3, 2, F, lone=False) for _ in range(EVENTS_MAX_GRAPHS)]
    check_graphs(hip, graphs, F, D, T, "iter_events", "iter_events", shared=shared, seed=D)


FEW_ITERS = [(F, D, T, True) for F, D in [(2, 8), (4, 16), (11, 4)] for T in (0, 1)] + \
            [(F, D, 0, False) for F, D in [(11, 4), (4, 16)]]


@pytest.mark.parametrize("F,D,T,shared", FEW_ITERS)
def test_few_iterations(hip, F, D, T, shared):
    """The shared fold's `extra` term with 0 and 1 slots in front of it; n_iters 0 with own sets: output_network on H_0."""
    check_graphs(hip, matrix_graphs(F, D, "ragged"), F, D, T, "iter_events", "iter_events", shared=shared, seed=T + D)


# ---- 4. non-finite inputs stay in their graph --------------------------------------------------------------------------
def _restated_masks(params, X, src, dst, y, T):
    """NaN masks of the fp64 restatement: ([e_t], {key: gradient}) with nn.BCELoss's terms without its range check."""
    p = {k: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for k, v in params.items()}
    es, _ = ref.forward(p, torch.tensor(np.asarray(X), dtype=torch.float64), torch.tensor(src, dtype=torch.int64),
                        torch.tensor(dst, dtype=torch.int64), T)
    nf.bce_terms(es[-1], torch.tensor(y, dtype=torch.float64)).mean().backward()
    return [np.isnan(e.detach().numpy()) for e in es], {k: np.isnan(v.grad.numpy()) for k, v in p.items()}


def _fused_loss_step(m, batch):
    """A training step through the project's BCELoss, which takes a NaN score (torch.nn.BCELoss refuses one)."""
    m.train()
    m.zero_grad()
    loss = BCELoss()(m(batch).reshape(-1), batch.y)
    loss.backward()
    return float(loss), {n: p.grad.detach().cpu().numpy() for n, p in m.named_parameters()}


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("site", ["X", "W"])
@pytest.mark.parametrize("F,D", [(2, 32), (11, 8)])
def test_a_nan_stays_in_its_graph(hip, F, D, site, route):
    """One NaN in a feature of one hit of the (30, 70) graph: every other graph keeps the clean run's bits, the poisoned
    graph's NaN masks are the restatement's, and so is every gradient tensor's after a training step.  One NaN in
    edge_networks.1's first weight, which every graph reads: the masks alone."""
    T = MATRIX_T
    params, _, _ = matrix_reference(F, D, False, "ragged")
    host = matrix_batch(F, D, "ragged")
    X, src, dst, y = host_arrays(host)
    hp, sp = np.asarray(host.hit_ptr), np.asarray(host.seg_ptr)
    bad_params, Xb = dict(params), X.copy()
    if site == "X":
        Xb[src[3], F - 1] = np.nan                      # a hit of graph 0 with a segment
        assert hp[0] <= src[3] < hp[1]
    else:
        w = params["edge_networks.1.network.0.weight"].copy()
        w[D // 2, 1] = np.nan
        bad_params["edge_networks.1.network.0.weight"] = w
    e_masks, g_masks = _restated_masks(bad_params, Xb, src, dst, y, T)
    assert e_masks[T].any() and (site == "W" or not e_masks[T][sp[1]:].any())
    clean = model_of(params, F, D, T, False, events=route == "iter_events").eval()
    m = model_of(bad_params, F, D, T, False, events=route == "iter_events").eval()
    batch, poisoned = host.to("cuda"), HitGraphBatch(Xb, src, dst, y=y, hit_ptr=hp, seg_ptr=sp).to("cuda")
    with torch.no_grad():
        e0, et0, Ht0 = clean(batch, trace=True)
        e1, et1, Ht1 = m(poisoned, trace=True)
    assert clean._route.kind == route and m._route.kind == route
    bad = []
    if site == "X":
        for what, a, b in (("scores", e0[sp[1]:], e1[sp[1]:]), ("e_t", et0[:, sp[1]:], et1[:, sp[1]:]),
                           ("H_t", Ht0[:, hp[1]:], Ht1[:, hp[1]:])):
            same = np.array_equal(_bits(a), _bits(b))
            print("  (%d, %d) %s the other graphs' %-6s %s" % (F, D, route, what, "keep their bits" if same else "CHANGE"))
            if not same:
                bad.append("the other graphs' %s" % what)
    for t in range(T + 1):
        got = np.isnan(et1[t].cpu().numpy())
        print("  (%d, %d) %s e_%d: %d NaN, the restatement %d" % (F, D, route, t, got.sum(), e_masks[t].sum()))
        if not np.array_equal(got, e_masks[t]):
            bad.append("NaN mask of e_%d" % t)
    if not np.array_equal(np.isnan(e1.cpu().numpy()), e_masks[T]):
        bad.append("NaN mask of the scores")
    loss, grads = _fused_loss_step(m, poisoned)
    assert m._route.kind == route
    print("  (%d, %d) %s loss %r" % (F, D, route, loss))
    if not np.isnan(loss):
        bad.append("loss %r is not NaN" % loss)
    for k in params:
        got = np.isnan(grads[k])
        print("  (%d, %d) %s grad %-40s %d of %d NaN, the restatement %d" % (F, D, route, k, got.sum(), got.size,
                                                                              g_masks[k].sum()))
        if not np.array_equal(got, g_masks[k]):
            bad.append("NaN mask of grad " + k)
    assert not bad, bad
