"""NaN and Inf through the trainable path on the GPU (the contract: INTEGRATION.md, "Non-finite values"): every route of
SegmentClassifier, NodeClassifier, the graph-convolution classifiers and the fused BCELoss, on the cases of
tests/nonfinite_cases.py, which tests/test_nonfinite_host.py has shown to be well posed.

  propagation   the NaN mask of a result equals the mask of the fp64 restatement (nonfinite_cases.expected_mask,
                nodeclf_reference, gcn_list_run, bce_terms) - a non-finite value never comes out as a plausible number
  isolation     everything outside that mask - other hits, other graphs, padded segments - has the BITS of the run
                with the poisoned entry set to 0.0
Every assertion is a mask equality, a bit equality, or TOL = 1e-5 on the scores of an Inf in X (tests/test_gpu_parity.py).
A case collects its failures and reports them together."""
import numpy as np
import pytest
import torch

import nonfinite_cases as nf
import route_cases
import test_gpu_gcn as gcn_cases
from gnn_fpga_amd.autograd import gcn_forward_layers
from gnn_fpga_amd.loss import BCELoss
from gnn_fpga_amd.model import NodeClassifier, SegmentClassifier
from oracle.dense_torch import KEYS
from route_cases import fwd as plan_recorder
from test_nonfinite_host import TRAIN_CASES, gcn_case as _gcn_case, train_case

pytestmark = pytest.mark.gpu

TOL = 1e-5          # tests/test_gpu_parity.py: edge scores against the CPU reference
FUSED = {"k_iter", "k_iter2", "k_iter_w", "k_iter_wx"}
SWITCHES = tuple(plan_recorder.SWITCHES) + tuple(route_cases.bwd.SWITCHES) + ("GNN_NO_FUSED_TRAIN", "GNN_NODE_ONE_LANE")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _weights(F, D, T):
    return route_cases.host_weights(dict(F=F, D=D, T=T))


def _segclf(F, D, T, train=False, **knobs):
    m = SegmentClassifier(input_dim=F, hidden_dim=D, n_iters=T).cuda()
    m.train() if train else m.eval()
    for k, v in knobs.items():
        setattr(m, k, v)
    return m


def _load(m, weights, keys=KEYS):
    m.load_state_dict({k: w.clone() for k, w in zip(keys, weights)})       # (copy_: the parameters' versions change)
    assert all(np.array_equal(_bits(p.detach().cpu().numpy()), _bits(w.numpy())) for p, w in zip(m.parameters(), weights))


def _scores(hip, m, b):
    """(scores [E] as a float32 array, names of the kernels that ran)."""
    with hip.profile(512) as prof:
        with torch.no_grad():
            e = m(b)
        torch.cuda.synchronize()
    return e.cpu().numpy(), {k for k, _ in prof.records}


def _clear_switches(monkeypatch, env=None):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if env:
        monkeypatch.setenv(env, "1")


# ---- forward routes -------------------------------------------------------------------------------------------------
#         id               batch   F   D  T  env                  model knobs                          kernels that must run / must not
ROUTES = [
    ("per_module",         "seg",  3,  8, 3, None,                dict(use_events=False, use_plan=False), {"k_input", "k_edge", "k_node"}, FUSED | {"k_event"}),
    ("plan_k_iter2",       "seg",  3,  8, 3, None,                dict(use_events=False, use_plan=True), {"k_iter2"}, {"k_node", "k_event"}),
    ("plan_k_iter_wx_32",  "seg",  3, 32, 2, "GNN_WIDE_ROLES",    dict(use_events=False, use_plan=True), {"k_iter_wx", "k_pack32"}, {"k_node", "k_iter_w"}),
    ("plan_k_iter_wx_64",  "seg",  3, 64, 2, "GNN_WIDE_ROLES",    dict(use_events=False, use_plan=True), {"k_iter_wx", "k_pack32"}, {"k_node", "k_iter_w"}),
    ("plan_k_iter_w_32",   "seg",  3, 32, 2, "GNN_WIDE_LOCKSTEP", dict(use_events=False, use_plan=True), {"k_iter_w", "k_pack32"}, {"k_node", "k_iter_wx"}),
    ("plan_k_iter_w_64",   "seg",  3, 64, 2, "GNN_WIDE_LOCKSTEP", dict(use_events=False, use_plan=True), {"k_iter_w", "k_pack32"}, {"k_node", "k_iter_wx"}),
    ("bf16_32",            "seg",  3, 32, 2, None,                dict(use_events=False, use_plan=True, mlp_bf16=True), {"k_pack16"}, {"k_node", "k_pack32"}),
    ("bf16_64",            "seg",  3, 64, 2, None,                dict(use_events=False, use_plan=True, mlp_bf16=True), {"k_pack16"}, {"k_node", "k_pack32"}),
    ("events_k_event",     "muon", 11, 8, 3, None,                dict(use_events=True), {"k_event"}, FUSED | {"k_node"}),
]


def _route_setup(hip, route, monkeypatch):
    """The route's model with the clean weights loaded, after one clean forward whose kernels and kind are the
    route's: (host batch, weights, model, X sites, check_names)."""
    name, which, F, D, T, env, knobs, must, must_not = route
    _clear_switches(monkeypatch, env)
    host = nf.seg_batch(F) if which == "seg" else nf.muon_batch()
    graph = nf.SEG_GRAPH if which == "seg" else nf.MUON_GRAPH
    planned = knobs.get("use_plan", False) is True
    w = _weights(F, D, T)
    m = _segclf(F, D, T, **knobs)
    _load(m, w)

    def check_names(names, what=None):
        assert must <= names and not names & must_not, (what, sorted(names))

    clean = nf.with_X(host, host.X.numpy()).cuda()          # (a copy: .cuda() moves the batch it is called on)
    _, names = _scores(hip, m, clean)
    check_names(names)
    assert m._route.kind == ("events" if which == "muon" else "plan" if planned else "per_module")
    sites = nf.x_sites(host, graph, clean.plan if planned else None)
    assert ("tile" in sites) == planned and (which == "muon" or "lonely" in sites)
    return host, w, m, sites, check_names


def _nan_cases(host, w, sites, bf16):
    """(what, X, weights, substituted X, substituted weights): a quiet NaN in X at every site and in the middle element
    of each weight; on the bf16 route also the other three bit patterns, in X (first hit), W1, W3 and W4."""
    cases = []
    for pat, v in (nf.NANS if bf16 else {"quiet": nf.QNAN}).items():
        for site, hit in sites.items():
            if pat == "quiet" or site == "first":
                cases.append(("NaN %s in X, %s hit %d" % (pat, site, hit), nf.poisoned_X(host, hit, v), w,
                              nf.poisoned_X(host, hit, 0.0), w))
        for k in (range(10) if pat == "quiet" else (2, 6, 8)):
            i = nf.w_site(w[k])
            cases.append(("NaN %s in %s[%d]" % (pat, KEYS[k], i), host.X.numpy(), w[:k] + [nf.put(w[k], i, v)] + w[k + 1:],
                          host.X.numpy(), w[:k] + [nf.put(w[k], i, 0.0)] + w[k + 1:]))
    return cases


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_forward_route_nan(hip, route, monkeypatch):
    """One NaN - in X at each site, in one element of each of the ten weights - on every forward route: the scores'
    NaN mask is the fp64 oracle's, with and without the exp-product form; every other score has the bits of the run
    with that entry 0.0.  The bf16 route runs all four NaN bit patterns in X, W1, W3 and W4 (its weights and features
    go through bf16_rne)."""
    T, bf16 = route[4], route[6].get("mlp_bf16", False)
    host, w, m, sites, check_names = _route_setup(hip, route, monkeypatch)
    bad = []
    for what, X, wk, X0, w0 in _nan_cases(host, w, sites, bf16):
        mask, _ = nf.expected_mask(X, host, wk, T)
        m.exp_product = False
        _load(m, w0)
        sub, _ = _scores(hip, m, nf.with_X(host, X0).cuda())
        _load(m, wk)
        got, names = _scores(hip, m, nf.with_X(host, X).cuda())
        check_names(names, what)
        if not np.array_equal(np.isnan(got), mask):
            bad.append("%s: %d scores NaN, the oracle has %d (%d differ)"
                       % (what, np.isnan(got).sum(), mask.sum(), (np.isnan(got) != mask).sum()))
        if not np.array_equal(_bits(got)[~mask], _bits(sub)[~mask]):
            bad.append("%s: %d scores outside the oracle's mask differ from the substituted run"
                       % (what, (_bits(got)[~mask] != _bits(sub)[~mask]).sum()))
        if "lonely" in what and not np.array_equal(_bits(got), _bits(sub)):
            bad.append("%s: a hit without segments changed a score" % what)
        m.exp_product = True
        again, _ = _scores(hip, m, nf.with_X(host, X).cuda())
        if not np.array_equal(np.isnan(again), mask):
            bad.append("%s, default exp_product: %d scores NaN, the oracle has %d" % (what, np.isnan(again).sum(), mask.sum()))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_forward_route_inf(hip, route, monkeypatch):
    """+inf and -inf in X at every site, on every forward route, with the default exp_product: the exp-product form
    is not taken (the plan routes keep the decision in `_xp_cache`), the scores' NaN mask is the fp64 oracle's - no
    NaN: tanh(+-inf) = +-1 - and the scores are within TOL of fp64.  The bf16 route is held to the first two: its
    scores are not within TOL of fp64 on any input (tests/test_gpu_bf16_reference.py has its bounds)."""
    T, knobs = route[4], route[6]
    bf16, planned = knobs.get("mlp_bf16", False), knobs.get("use_plan", False) is True
    host, w, m, sites, check_names = _route_setup(hip, route, monkeypatch)
    m.exp_product = True
    bad = []
    for inf, v in nf.INFS.items():
        for site, hit in sites.items():
            what = "%s in X, %s hit %d" % (inf, site, hit)
            X = nf.poisoned_X(host, hit, v)
            mask, e64 = nf.expected_mask(X, host, w, T)
            m._xp_cache = None
            got, names = _scores(hip, m, nf.with_X(host, X).cuda())
            check_names(names, what)
            if planned and (m._xp_cache is None or m._xp_cache[1] != 0):
                bad.append("%s: the exp-product form was taken (%r)" % (what, m._xp_cache))
            if not np.array_equal(np.isnan(got), mask):
                bad.append("%s: %d scores NaN, the oracle has %d" % (what, np.isnan(got).sum(), mask.sum()))
            elif not bf16 and np.abs(got[~mask] - e64[~mask]).max() >= TOL:
                bad.append("%s: max |HIP - fp64| = %.3g" % (what, np.abs(got[~mask] - e64[~mask]).max()))
    assert not bad, "\n".join(bad)


def test_plan_feature_range_keeps_a_nan(hip):
    """The HIP plan builder's per-feature |X| maximum is NaN where the host builder's is (np.abs(X).max): the
    exp-product bound is then NaN, which is not <= 60."""
    host = nf.seg_batch()
    hit = nf.x_sites(host, nf.SEG_GRAPH)["first"]
    b = nf.with_X(host, nf.poisoned_X(host, hit, nf.QNAN, feature=1)).cuda()
    got = b.build_plan(8).x_absmax.cpu().numpy()
    want = np.abs(b.X.cpu().numpy()).max(axis=0)
    assert list(np.isnan(got)) == [False, True, False] and np.array_equal(_bits(got)[[0, 2]], _bits(want)[[0, 2]])
    w = [t.cuda() for t in _weights(3, 8, 3)]
    assert np.isnan(hip.exp_product_bound(w, 3, 8, b.plan.x_absmax))
    w[2] = nf.put(w[2], 5, nf.QNAN).cuda()
    assert np.isnan(hip.exp_product_bound(w, 3, 8, b.plan.x_absmax.nan_to_num(1.0)))


# ---- training routes ------------------------------------------------------------------------------------------------
_TRAIN_REF = {}


def _train_reference(key, site):
    if (key, site) not in _TRAIN_REF:
        b, X, w, y = train_case(*key, site)
        loss, grads = nf.train_reference(X, b, w, key[3], y)
        _TRAIN_REF[key, site] = (np.isnan(loss), [np.isnan(g) for g in grads])
    return _TRAIN_REF[key, site]


#              id           case            env                   knobs                                              kind        kernels
TRAIN_ROUTES = [
    ("pass",       TRAIN_CASES[0], None,                 dict(use_events=False, level_order_training=True), "pass",    {"k_seg_bwd4"}),
    ("wide_32",    TRAIN_CASES[1], None,                 dict(use_events=False, level_order_training=True), "pass",    {"k_seg_bwdW"}),
    ("events",     TRAIN_CASES[2], None,                 dict(use_events=True),                             "events",  {"k_event", "k_event_bwd"}),
    ("twin",       TRAIN_CASES[3], None,                 dict(use_events=False, level_order_training=True), "twin",    {"k_edge_tw", "k_seg_bwd4"}),
    ("twin_pp",    TRAIN_CASES[3], "GNN_NO_FUSED_TRAIN", dict(use_events=False, level_order_training=True), "twin_pp", {"k_node", "k_seg_bwd4"}),
]


@pytest.mark.parametrize("site", ["X", "W"])
@pytest.mark.parametrize("route", TRAIN_ROUTES, ids=[r[0] for r in TRAIN_ROUTES])
def test_training_route(hip, route, site, monkeypatch):
    """A NaN in X (first hit of the middle graph) or in one element of W3: the loss through the project's BCELoss is
    NaN and every gradient tensor's NaN mask is the fp64 reference's (all NaN: test_nonfinite_host.py)."""
    name, key, env, knobs, kind, must = route
    _clear_switches(monkeypatch, env)
    _, F, D, T = key
    host, X, w, y = train_case(*key, site)
    want_loss, want = _train_reference(key, site)
    m = _segclf(F, D, T, train=True, **knobs)
    _load(m, w)
    b = nf.with_X(host, X).cuda()
    with hip.profile(512) as prof:
        m.zero_grad()
        loss = BCELoss()(m(b), y.cuda())
        loss.backward()
        torch.cuda.synchronize()
    names = {k for k, _ in prof.records}
    assert m._route.kind == kind and must <= names and "k_bce" in names, (m._route.kind, sorted(names))
    assert bool(torch.isnan(loss)) == bool(want_loss) and want_loss
    bad = ["%s: %d of %d NaN, the reference has %d" % (k, g.sum(), g.size, r.sum())
           for k, g, r in zip(KEYS, [np.isnan(p.grad.cpu().numpy()) for p in m.parameters()], want) if not np.array_equal(g, r)]
    assert not bad, "\n".join(bad)


# ---- NodeClassifier -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [8, 64])
def test_node_classifier(hip, D, monkeypatch):
    _clear_switches(monkeypatch)
    host, (F, T) = nf.seg_batch(), (3, 2)
    import nodeclf_fp64
    w12 = _weights(F, D, T) + list(route_cases.head(dict(F=F, D=D, T=T)))
    y = nf.labels(host.n_hits, 1)
    m = NodeClassifier(input_dim=F, hidden_dim=D, n_iters=T).cuda()
    cases = [("NaN in X, %s hit %d" % (s, h), nf.poisoned_X(host, h, nf.QNAN), w12, nf.poisoned_X(host, h, 0.0), w12)
             for s, h in nf.x_sites(host, nf.SEG_GRAPH).items()]
    for k in range(12):
        i = nf.w_site(w12[k])
        cases.append(("NaN in %s[%d]" % (nodeclf_fp64.KEYS[k], i), host.X.numpy(), w12[:k] + [nf.put(w12[k], i, nf.QNAN)] + w12[k + 1:],
                      host.X.numpy(), w12[:k] + [nf.put(w12[k], i, 0.0)] + w12[k + 1:]))
    bad = []
    for what, X, wk, X0, w0 in cases:
        s64, _, _ = nf.nodeclf_reference(X, host, wk, T)
        mask = np.isnan(s64)
        m.eval()
        with torch.no_grad():
            _load(m, w0, nodeclf_fp64.KEYS)
            sub = m(nf.with_X(host, X0).cuda()).cpu().numpy()
            _load(m, wk, nodeclf_fp64.KEYS)
            got = m(nf.with_X(host, X).cuda()).cpu().numpy()
        if not np.array_equal(np.isnan(got), mask):
            bad.append("%s: %d hit scores NaN, the reference has %d" % (what, np.isnan(got).sum(), mask.sum()))
        elif not np.array_equal(_bits(got)[~mask], _bits(sub)[~mask]):
            bad.append("%s: scores outside the mask differ from the substituted run" % what)
        if "first" in what or "node_network.network.0.weight" in what:          # the training step, head backward included
            _, loss64, g64 = nf.nodeclf_reference(X, host, wk, T, y)
            m.train()
            m.zero_grad()
            loss = BCELoss()(m(nf.with_X(host, X).cuda()), y.cuda())
            loss.backward()
            if not (np.isnan(loss64) and bool(torch.isnan(loss))):
                bad.append("%s: loss %r, the reference's %r" % (what, float(loss), loss64))
            for k, p, r in zip(nodeclf_fp64.KEYS, m.parameters(), g64):
                g = np.isnan(p.grad.cpu().numpy())
                if not np.array_equal(g, np.isnan(r)):
                    bad.append("%s: grad %s %d of %d NaN, the reference has %d" % (what, k, g.sum(), g.size, np.isnan(r).sum()))
    assert not bad, "\n".join(bad)


# ---- BCELoss --------------------------------------------------------------------------------------------------------
BAD_SCORES = [nf.QNAN, 1.5, -0.1, float("inf"), float("-inf")]


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("n", [1, 100003, 262145])       # 262145: one past kBlock * kBceBlocks - the grid-stride loop wraps
def test_bce_loss(hip, n, reduction):
    """One bad element - a score that is NaN, outside [0, 1] or infinite, or a NaN label - at index 0, at the last
    index or at index 262144: the loss is NaN, the gradient is NaN on that element and nowhere else, and every other
    element of the gradient has the bits of the clean run."""
    g = torch.Generator().manual_seed(n)
    e0 = (0.01 + 0.98 * torch.rand(n, generator=g)).cuda()
    y0 = (torch.rand(n, generator=g) < 0.4).float().cuda()
    loss_fn = BCELoss(reduction=reduction)

    def run(e, y):
        e = e.clone().requires_grad_(True)
        loss = loss_fn(e, y)
        loss.backward()
        return float(loss.detach()), e.grad.cpu().numpy()

    loss0, grad0 = run(e0, y0)
    assert np.isfinite(loss0) and np.isfinite(grad0).all()
    bad = []
    for at in sorted({0, n - 1, min(262144, n - 1)}):
        for what, value in [("score", v) for v in BAD_SCORES] + [("label", nf.QNAN)]:
            e, y = e0.clone(), y0.clone()
            (e if what == "score" else y)[at] = float(value)
            loss, grad = run(e, y)
            want = np.zeros(n, bool)
            want[at] = True
            if not np.isnan(loss):
                bad.append("%s %r at %d: loss %r" % (what, value, at, loss))
            if not np.array_equal(np.isnan(grad), want):
                bad.append("%s %r at %d: gradient NaN at %s" % (what, value, at, np.flatnonzero(np.isnan(grad))[:5]))
            elif not np.array_equal(_bits(grad)[~want], _bits(grad0)[~want]):
                bad.append("%s %r at %d: the gradient of other elements changed" % (what, value, at))
    assert not bad, "\n".join(bad)


# ---- graph-convolution classifiers ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", range(len(gcn_cases.CONFIGS)))
def test_gcn_nan_weight(hip, cfg):
    """A NaN in one element of each weight: every logit is NaN (torch.relu(NaN) is NaN), in the inference launch and
    in the training one; the loss is NaN and every gradient's NaN mask is the list-form fp64 reference's."""
    kind, conv, dims, model, x, A, y = _gcn_case(cfg)
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    adj = gcn_cases.compress_adjacency(torch.from_numpy(A).cuda())
    state = model.state_dict()
    bad = []
    for k, t in state.items():
        poisoned = dict(state, **{k: nf.put(t, nf.w_site(t), nf.QNAN).reshape(t.shape)})
        m = gcn_cases.package_model(kind, conv, 3, dims, poisoned)
        with torch.no_grad():
            out = m.eval()(xt, adj).cpu().numpy()
        if not np.isnan(out).all():
            bad.append("%s: %d of %d logits NaN (inference)" % (k, np.isnan(out).sum(), out.size))
        logits, loss, grads = gcn_cases.train_step(m, xt, adj, yt)
        model.load_state_dict(poisoned)
        ref = nf.gcn_list_run(model, x, A, y)
        if not (np.isnan(logits).all() and np.isnan(loss) and np.isnan(ref["loss"])):
            bad.append("%s: %d of %d logits NaN, loss %r (training)" % (k, np.isnan(logits).sum(), logits.size, loss))
        for name, r in ref["grads"].items():
            g = np.isnan(grads[name])
            if not np.array_equal(g, np.isnan(r)):
                bad.append("%s: grad %s %d of %d NaN, the reference has %d" % (k, name, g.sum(), g.size, np.isnan(r).sum()))
    model.load_state_dict(state)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("cfg", range(len(gcn_cases.CONFIGS)))
def test_gcn_nan_feature(hip, cfg):
    """A NaN in one x entry of the middle graph: the logits' NaN mask covers the list-form reference's and stays
    inside that graph; the other graphs' logits and kept activations have the clean run's bits; the gradients' NaN
    masks cover the reference's."""
    kind, conv, dims, model, x, A, y = _gcn_case(cfg)
    m = gcn_cases.package_model(kind, conv, 3, dims, model.state_dict())
    yt = torch.from_numpy(y).cuda()
    adj = gcn_cases.compress_adjacency(torch.from_numpy(A).cuda())
    xp = x.copy()
    xp[1, 7, 0] = nf.QNAN
    ref = nf.gcn_list_run(model, xp, A, y)
    want = np.isnan(ref["logits"])
    assert want[1].any() and not want[1].all() and not want[[0, 2]].any()
    clean, hs0 = gcn_forward_layers(m, torch.from_numpy(x).cuda(), adj)
    out, hs = gcn_forward_layers(m, torch.from_numpy(xp).cuda(), adj)
    got = np.isnan(out.cpu().numpy())
    assert (got | ~want).all(), "a node the lists reach is finite: %s" % np.argwhere(want & ~got)[:5]
    assert not got[[0, 2]].any()
    others = [0, 2]
    assert np.array_equal(_bits(out.cpu().numpy())[others], _bits(clean.cpu().numpy())[others])
    for h, h0 in zip(hs, hs0):
        assert np.array_equal(_bits(h.cpu().numpy())[others], _bits(h0.cpu().numpy())[others])
    with torch.no_grad():
        assert np.array_equal(np.isnan(m.eval()(torch.from_numpy(xp).cuda(), adj).cpu().numpy()), got)
    logits, loss, grads = gcn_cases.train_step(m, torch.from_numpy(xp).cuda(), adj, yt)
    assert np.array_equal(np.isnan(logits), got) and np.isnan(loss) and np.isnan(ref["loss"])
    bad = [k for k, r in ref["grads"].items() if not (np.isnan(grads[k]) | ~np.isnan(r)).all()]
    assert not bad, bad
