"""Every HIP entry point on poisoned workspaces and guarded outputs (tests/poisoned_alloc.py).

The other GPU files pin values; the memory the kernels are handed is always whatever torch's caching allocator last
held - often zeros, or the previous run of the same call.  Here every wrapper runs four times through one function,
`check(call)`: twice as it is (the outputs must be bit-equal), then with every workspace and output of the package
filled with 0xFF bytes and with the bytes of int64 1, between 64 KiB guard bands filled the same way.  A poisoned run
must give the plain run's bits (a scratch region or counter read before it is written, or an output element no kernel
writes, changes them) and leave every guard as it was (a write outside the workspace bytes the call asked for, or
outside an output, lands there).  Integer outputs are also compared with the numpy specification the package ships;
float outputs rely on bit-equality with the plain run, which the other files pin to float64.

Caller-provided `out=` / `into=` targets are made through the same proxy (`_empty`); `into=` tensors are then
overwritten with their seeded prefill, since they are inputs.  Buffers the ABI documents as "zero them first" or
"added into" are zero-filled by the wrappers (`torch.zeros`, which the proxy leaves alone): that is the contract.
"""
import contextlib
import os

import numpy as np
import pytest
import torch

import route_cases as rc
from poisoned_alloc import poison

pytestmark = pytest.mark.gpu

_ALLOC = [torch]        # what `_empty` allocates through: the active context's proxy, else torch


def _empty(*shape, dtype=torch.float32):
    return _ALLOC[0].empty(*shape, dtype=dtype, device="cuda")


def _flat(outs):
    """Nested tuples / lists of tensors (None skipped) as a flat list."""
    if outs is None:
        return []
    if torch.is_tensor(outs):
        return [outs]
    return [t for o in outs for t in _flat(o)]


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def _assert_same(want, got, what):
    assert len(want) == len(got), what
    for i, (a, b) in enumerate(zip(want, got)):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, i, a.shape, b.shape, a.dtype, b.dtype)
        if not torch.equal(_bits(a), _bits(b)):
            es = a.element_size()
            bad = (_bits(a) != _bits(b)).reshape(-1, es).any(dim=1).nonzero().flatten()
            first = int(bad[0])
            raise AssertionError("%s: output %d %s %s differs in %d of %d elements, first at flat index %d: %r != %r"
                                 % (what, i, tuple(a.shape), a.dtype, bad.numel(), a.numel(), first,
                                    a.reshape(-1)[first].item(), b.reshape(-1)[first].item()))


def check(call, allocates=True):
    """`call()` runs a public wrapper on device inputs prepared outside and returns its outputs (tensors, nested as
    the wrapper returns them).  Plain twice: bit-equal.  Then under poison("ff") and under poison("one"): bit-equal to
    the plain run, every guard intact - asserted before the next pattern starts.  Returns the plain run's outputs."""
    plain = [t.clone() for t in _flat(call())]
    again = _flat(call())
    torch.cuda.synchronize()
    _assert_same(plain, again, "the plain call twice")
    for pattern in ("ff", "one"):
        with poison(pattern) as p:
            _ALLOC[0] = p.proxy
            try:
                got = [t.clone() for t in _flat(call())]
            finally:
                _ALLOC[0] = torch
            assert bool(p.records) == allocates, "the package's allocations: %d" % len(p.records)
            damaged = p.guards_intact()
        assert damaged == [], "poison(%r): guard bytes overwritten next to the allocation(s) at %s" % (pattern, damaged)
        _assert_same(plain, got, "poison(%r) against the plain run" % pattern)
    return plain


def _np(t):
    return t.detach().cpu().numpy()


@contextlib.contextmanager
def _env(**kv):
    saved = {k: os.environ.get(k) for k in kv}
    for k, v in kv.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


# ---- the training forwards and every backward route ---------------------------------------------------------------
BWD_CASES = rc.backward_cases()


def _device_grad(case, inp):
    go = rc.upstream(case).cuda()
    if case["kind"] == "node":                      # rows of H_all's stride, the first D columns used
        full = torch.zeros_like(inp.H_all[1])
        full[:, :case["D"]] = go
        return full
    return go


def _backward_call(case, into=False):
    head = rc.head(case) if case["kind"] == "nodeclf" else None
    pre = rc.prefill(case) if into else None

    def call():
        inp = rc.bwd.build_inputs(case, head=head)          # the training forward of the case's entry point
        target = None
        if into:
            target = [_empty(tuple(t.shape)) for t in pre]
            for t, v in zip(target, pre):
                t.copy_(v)
        got = rc.bwd.run_inputs(inp, grad=_device_grad(case, inp), into=target)
        return [inp.e_all, inp.H_all, inp.Q_all, inp.y, got]
    return call


@pytest.mark.parametrize("case", BWD_CASES, ids=[rc.case_id(c) for c in BWD_CASES])
def test_training_forward_and_backward(hip, case):
    with rc.bwd.switch(case["env"]):
        check(_backward_call(case))


@pytest.mark.parametrize("name", rc.INTO_CASES, ids=[n.replace(" ", "_") for n in rc.INTO_CASES])
def test_backward_into_the_callers_tensors(hip, name):
    case = rc.case_named(name)
    with rc.bwd.switch(case["env"]):
        check(_backward_call(case, into=True))


# ---- the fused forward on a plan built inside the poisoned context ------------------------------------------------
@pytest.mark.parametrize("case", rc.fwd.CASES, ids=[rc.case_id(c) for c in rc.fwd.CASES])
def test_plan_build_and_fused_forward(hip, case):
    def call():
        inp = rc.fwd.build_inputs(case)                     # HipSellPlan (and the training case's twin) built here
        _, first, second = rc.fwd.run_inputs(inp)           # under the case's switch
        return [first, second]
    check(call)


# ---- the per-module forwards, the list builder and the dense adapter ----------------------------------------------
FWD_SHAPES = [(3, 8), (2, 4), (11, 16), (3, 32), (3, 64)]
T_FWD = 2


def _edge_graphs(F, big=True):
    """A 1-hit self-loop graph, a 2-hit graph, a graph without segments, a graph of padded segments only, 20 layered
    graphs of 8 .. 80 hits and (`big`) one of 700 hits / 4000 segments."""
    from gnn_fpga_amd import synth
    rng = np.random.default_rng(100 + F)
    x = lambda n: rng.uniform(-1.0, 1.0, size=(n, F)).astype(np.float32)    # noqa: E731
    i32 = lambda a: np.asarray(a, dtype=np.int32)                            # noqa: E731
    G = synth.HitGraph
    graphs = [G(x(1), i32([0]), i32([0]), np.ones(1, np.float32)),
              G(x(2), i32([0]), i32([1]), np.zeros(1, np.float32)),
              G(x(5), i32([]), i32([]), np.zeros(0, np.float32)),
              G(x(4), i32([-1] * 6), i32([-1] * 6), np.zeros(6, np.float32))]
    for i in range(20):
        n = 8 + (72 * i) // 19
        graphs.append(synth.layered_graph(n, 3 * n + i, F, n_layers=4, seed=200 + i))
    if big:
        graphs.append(synth.layered_graph(700, 4000, F, seed=300))
    return graphs


def _host_batch(F, big=True):
    """_edge_graphs as one batch on the host, every 7th segment padded."""
    from gnn_fpga_amd import HitGraphBatch
    b = HitGraphBatch.from_graphs(_edge_graphs(F, big))
    src, dst = b.src.numpy().copy(), b.dst.numpy().copy()
    src[3::7] = -1
    dst[3::7] = -1
    return HitGraphBatch(b.X.numpy(), src, dst, y=b.y.numpy(), hit_ptr=b.hit_ptr, seg_ptr=b.seg_ptr)


def _weights(F, D, T=T_FWD):
    from gnn_fpga_amd.model import SegmentClassifier
    torch.manual_seed(7 * D + F)
    m = SegmentClassifier(input_dim=F, hidden_dim=D, n_iters=T)
    w = [t.detach().contiguous().cuda() for t in m.effective_weights()]
    g = torch.Generator().manual_seed(11 * D + F)
    return w, (0.3 * torch.randn(1, F + D, generator=g)).cuda(), torch.randn(1, generator=g).cuda()


def _assert_lists(parts, src, dst, n_hits):
    """gnn_csr_build's seven outputs against hitgraph._csr_by (eid / nbr: the lists, then -1; status 0)."""
    from gnn_fpga_amd.hitgraph import _csr_by
    want = _csr_by(dst, src, n_hits) + _csr_by(src, dst, n_hits)
    for k, name in enumerate(("in_ptr", "in_eid", "in_nbr", "out_ptr", "out_eid", "out_nbr")):
        got = _np(parts[k])
        assert got.dtype == np.int32
        if name.endswith("ptr"):
            assert np.array_equal(got, want[k]), name
        else:
            n = want[k].shape[0]
            assert got.shape[0] == src.shape[0] and np.array_equal(got[:n], want[k]), name
            assert np.all(got[n:] == -1), name
    assert int(_np(parts[6])[0]) == 0


@pytest.mark.parametrize("F,D", FWD_SHAPES, ids=["%dx%d" % s for s in FWD_SHAPES])
def test_per_module_forwards(hip, F, D):
    w, Wo, bo = _weights(F, D)
    host = _host_batch(F)
    src, dst = host.src.numpy().copy(), host.dst.numpy().copy()
    trace = (F, D) == (3, 8)
    ldh = hip.h_stride(F, D)

    def call():
        b = _host_batch(F).cuda()
        parts = hip.csr_build(b.src, b.dst, b.n_hits)
        out = hip.segclf_forward(b, w, F, D, T_FWD, out=_empty(b.n_segments))      # (builds the batch's own lists)
        traced = hip.segclf_forward(b, w, F, D, T_FWD, trace=True) if trace else None
        y = hip.nodeclf_forward(b, w, Wo, bo, F, D, T_FWD, trace=trace)
        H = hip.input_fwd(b.X, w[0], w[1])
        e = hip.edge_fwd(H, b.src, b.dst, *w[2:6], F, D)
        Hn = hip.node_fwd(H, e, b, *w[6:10], F, D)
        return [parts, out, traced, y, H, e, Hn]

    plain = check(call)
    _assert_lists(plain[:7], src, dst, host.n_hits)
    H = plain[-3]
    assert H.shape == (host.n_hits, ldh) and not bool(torch.isnan(H).any())
    assert bool((H[:, F + D:] == 0).all())                  # the documented zero pad of a hit-feature row


def _event_shapes():
    """The FWD_SHAPES whose one-launch forward takes the batch without the 700-hit graph (asked, not listed)."""
    from gnn_fpga_amd import _lib
    out = []
    for F, D in FWD_SHAPES:
        lay = _host_batch(F, big=False).event_layout()
        if lay is not None and _lib.events_supported(F, D, lay.max_hits, lay.max_segments):
            out.append((F, D))
    return out


EVENT_SHAPES = _event_shapes()


def test_one_launch_forward_has_cases():
    assert (3, 8) in EVENT_SHAPES and (2, 4) in EVENT_SHAPES


@pytest.mark.parametrize("F,D", EVENT_SHAPES, ids=["%dx%d" % s for s in EVENT_SHAPES])
def test_one_launch_forward(hip, F, D):
    w, _, _ = _weights(F, D)

    def call():
        b = _host_batch(F, big=False).cuda()
        # (a batch nobody has asked the lists of: the kernel builds them in LDS)
        fresh = hip.segclf_forward_events(b, b.event_layout(), w, F, D, T_FWD, out=_empty(b.n_segments))
        b.in_ptr                                            # the batch's lists (gnn_csr_build), then the same call
        listed = hip.segclf_forward_events(b, b.event_layout(), w, F, D, T_FWD)
        return [fresh, listed]

    fresh, listed = check(call)
    assert torch.equal(fresh, listed)


def test_dense_to_index(hip):
    from gnn_fpga_amd import HitGraphBatch, synth
    graphs = _edge_graphs(3, big=False)[:12]
    n_max = max(g.X.shape[0] for g in graphs)
    e_max = max(g.src.shape[0] for g in graphs) + 3
    dense = [synth.to_dense(synth.HitGraph(g.X, g.src[g.src >= 0], g.dst[g.src >= 0], None), n_max, e_max)
             for g in graphs]
    Ri = torch.from_numpy(np.stack([d[1] for d in dense]).astype(np.float32))
    Ro = torch.from_numpy(np.stack([d[2] for d in dense]).astype(np.float32))
    X = torch.from_numpy(np.stack([d[0] for d in dense]).astype(np.float32))
    want = HitGraphBatch.from_dense(X, Ri, Ro)              # the host adapter: the specification
    Rid, Rod = Ri.cuda(), Ro.cuda()
    src, dst, flags = check(lambda: hip.dense_to_index(Rid, Rod))
    assert np.array_equal(_np(src), want.src.numpy()) and np.array_equal(_np(dst), want.dst.numpy())
    assert int(flags.item()) == 0


# ---- the two classifiers as modules: their own workspace, kept dirty across batches and routes --------------------
def _model_call(make_model, F, train=False, **attrs):
    def call():
        model = make_model()                                # `_workspace` is None: allocated inside the context
        for k, v in attrs.items():
            setattr(model, k, v)
        big, small = _host_batch(F).cuda(), _host_batch(F, big=False).cuda()
        outs = []
        if train:
            model.train()
            for b in (big, small, big):                     # (the same batch object a second time: "auto" policies)
                model.zero_grad(set_to_none=True)
                e = model(b)
                (e * torch.linspace(0.5, 1.5, e.numel(), device=e.device).view_as(e)).sum().backward()
                outs += [e.detach()] + [p.grad.clone() for p in model.parameters()]
            return outs
        model.eval()
        with torch.no_grad():
            for b in (big, small, big, small):              # a smaller batch on the larger one's dirty workspace
                outs.append(model(b).clone())
        return outs
    return call


def _segclf(F=3, D=8, T=2):
    from gnn_fpga_amd.model import SegmentClassifier

    def make():
        torch.manual_seed(5 * D + F)
        return SegmentClassifier(input_dim=F, hidden_dim=D, n_iters=T).cuda()
    return make


def _nodeclf(F=3, D=8, T=2):
    from gnn_fpga_amd.model import NodeClassifier

    def make():
        torch.manual_seed(5 * D + F + 1)
        return NodeClassifier(input_dim=F, hidden_dim=D, n_iters=T).cuda()
    return make


MODEL_ROUTES = {"per_module": dict(use_plan=False, use_events=False), "plan": dict(use_plan=True, use_events=False),
                "auto": dict(use_plan="auto", use_events=False), "events": dict(use_plan=True, use_events=True)}


@pytest.mark.parametrize("route", sorted(MODEL_ROUTES))
@pytest.mark.parametrize("D", [8, 32])
def test_segment_classifier_inference(hip, route, D):
    check(_model_call(_segclf(D=D), 3, **MODEL_ROUTES[route]))


@pytest.mark.parametrize("level_order", [False, True])
@pytest.mark.parametrize("events", [False, True])
@pytest.mark.parametrize("D", [8, 32])
def test_segment_classifier_training(hip, level_order, events, D):
    check(_model_call(_segclf(D=D), 3, train=True, level_order_training=level_order, use_events=events))


@pytest.mark.parametrize("train", [False, True])
def test_node_classifier(hip, train):
    check(_model_call(_nodeclf(), 3, train=train))


def test_masked_model_with_pruned_units(hip):
    from gnn_fpga_amd.model import SegmentClassifier
    from golden_util import Fixture
    fx = Fixture("pruned_units_d8_s0")          # masks that kill whole units: the kernels of hidden_dim 4 run it
    masks = [[torch.from_numpy(fx.masks["%s_network.network.%d.weight" % (net, k)]) for k in (0, 2)]
             for net in ("edge", "node")]

    def make():
        m = SegmentClassifier(input_dim=fx.F, hidden_dim=fx.D, n_iters=fx.n_iters, masks_e=masks[0], masks_n=masks[1])
        m.load_state_dict({k: torch.from_numpy(v) for k, v in fx.params.items()})
        return m.cuda()
    for route in ("plan", "events"):
        check(_model_call(make, fx.F, prune_dead_units=True, **MODEL_ROUTES[route]))
    assert make().eval().pruned_info() is not None


# ---- the loss -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want_grad", [True, False], ids=["grad", "no_grad"])
@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 100003])
def test_bce_loss(hip, n, reduction, want_grad):
    g = torch.Generator().manual_seed(n)
    e = torch.rand(n, generator=g)
    y = (torch.rand(n, generator=g) < 0.3).float()
    for k, (v, t) in enumerate(((0.0, 0.0), (0.0, 1.0), (1.0, 0.0), (1.0, 1.0))):    # the clamps' edges
        if n:
            at = (k * (n - 1)) // 3
            e[at], y[at] = v, t
    scale = 1.0 / max(n, 1) if reduction == "mean" else 1.0
    ed, yd = e.cuda(), y.cuda()
    loss, grad = (check(lambda: hip.bce_loss(ed, yd, scale, want_grad=want_grad)) + [None])[:2]
    assert loss.shape == (1,) and bool(torch.isfinite(loss).all())
    assert (grad is not None) == want_grad and (grad is None or grad.shape == (n,))


# ---- the plan builder's two calls, array for array against plan.SellPlan ------------------------------------------
PLAN_CASES = ["ragged", "padded", "leading_pads", "global", "wide", "cyclic", "tiny_tiles"]
PLAN_MODES = {"graph_local": {}, "global_form": {"GNN_PLAN_GRAPH_LOCAL": "0"},
              "scatter_lists": {"GNN_PLAN_SCATTER_LISTS": "1"}}


@pytest.mark.parametrize("mode", sorted(PLAN_MODES))
@pytest.mark.parametrize("case", PLAN_CASES)
def test_plan_builder(hip, case, mode):
    from gnn_fpga_amd.plan import SellPlan
    from gnn_fpga_amd.plan_hip import HipSellPlan
    from test_plan import _same_plan
    from test_plan_hip import case_batch
    b, F, D, lim_over = case_batch(case)
    lim = hip.plan_limits(F, D)
    lim.update(lim_over)
    host = SellPlan(b, lim)
    forms = []

    def call():
        dev = HipSellPlan(case_batch(case)[0].cuda(), lim, debug=True)      # gnn_plan_build_sizes[_graphs] / _fill
        _same_plan(host, dev)                                               # every array, in every run
        forms.append((dev.graph_local, dev.list_mode))
        return [getattr(dev, k) for k in dev._TENSORS] + list(dev._dbg)

    with _env(**dict({"GNN_PLAN_GRAPH_LOCAL": None, "GNN_PLAN_SCATTER_LISTS": None}, **PLAN_MODES[mode])):
        check(call)
    assert len(set(forms)) == 1                                             # poison does not change the form taken
    if mode == "global_form":
        assert forms[0] == (False, 0)
    elif case != "cyclic":                                                  # (cycles: status 128 -> the global form)
        assert forms[0][0] and (mode != "scatter_lists" or forms[0][1] == 0)


# ---- segment metrics ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_shift", [10, 23])
@pytest.mark.parametrize("per_graph", [False, True], ids=["flat", "per_graph"])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 20000])
def test_segment_metrics_update(hip, n, per_graph, key_shift):
    from gnn_fpga_amd.metrics import segment_metrics_numpy
    from test_gpu_metrics import scores
    thresholds = (0.5, 0.25)
    bpo = 1 << (23 - key_shift)
    e, y = scores("adversarial", n, seed=n + key_shift)
    rng = np.random.default_rng(n)
    src = np.where(rng.random(n) < 0.1, -1, 0).astype(np.int32)
    sp = None
    if per_graph:                       # 12 graphs, the first, the last and a run in the middle empty
        cuts = np.sort(rng.integers(0, n + 1, 8))
        sp = np.concatenate([[0, 0], cuts[:4], [cuts[4]] * 2, cuts[4:], [n, n]]).astype(np.int64)
    spec = segment_metrics_numpy(e, y, thresholds, bpo, src, sp)
    n_bins = hip.metrics_bins(key_shift)
    assert spec["hist"].shape == (2, n_bins)
    ed, yd, sd = torch.from_numpy(e).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(src).cuda()
    spd = None if sp is None else torch.from_numpy(sp).cuda()

    def call():
        counts = torch.zeros((len(thresholds) + 1, 2), dtype=torch.int64, device="cuda")   # the contract: zeroed
        hist = torch.zeros((2, n_bins), dtype=torch.int64, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        pg = _empty((sp.size - 1, len(thresholds) + 1, 2), dtype=torch.int64) if per_graph else None
        hip.segment_metrics_update(ed, yd, sd, thresholds, key_shift, counts, hist, status, spd, pg)
        return [counts, hist, status, pg]

    # (without per_graph the call takes no workspace at these sizes and the caller's targets are its own: nothing of
    # the package's is poisoned there, and the case holds the contract's zeroed targets against the specification)
    need = hip.load().gnn_metrics_workspace_bytes(n, len(thresholds), key_shift, 0 if sp is None else sp.size - 1)
    got = check(call, allocates=per_graph or need > 0)
    assert int(got[2].item()) == spec["status"]
    assert np.array_equal(_np(got[0]), spec["counts"]) and np.array_equal(_np(got[1]), spec["hist"])
    if per_graph:
        assert np.array_equal(_np(got[3]), spec["per_graph"])
        empty = np.flatnonzero(np.diff(sp) == 0)
        assert empty.size >= 4 and not _np(got[3])[empty].any()            # an empty graph's rows: 0, not poison


# ---- track candidates and their matching --------------------------------------------------------------------------
def _tracks_call(batch, scores, threshold, mode, min_hits, pid):
    from tracks_cases import assert_match_equal, assert_tracks_equal, match_spec, spec_of
    from gnn_fpga_amd import build_tracks
    spec = spec_of(batch, scores, threshold, mode, min_hits)
    pid_dev = torch.as_tensor(pid).cuda()

    def call():
        tracks = build_tracks(batch, scores, threshold, mode, min_hits)     # gnn_track_build_labels
        assert_tracks_equal(tracks, spec)                                   # (with the lists where the status is 0)
        outs = [tracks.track_of_hit, tracks.root_of_hit, tracks._sizes]
        if not spec["status"]:
            m = tracks.match(pid_dev)                                       # gnn_track_build_lists, gnn_track_match
            assert_match_equal(m, match_spec(tracks, pid))
            outs += [tracks.track_ptr, tracks.track_hits, tracks.track_graph, tracks.graph_track_ptr,
                     m.majority_particle, m.majority_hits, m.particle_hits, m.matched, m.counts]
        return outs
    return call


TRACK_MODES = ("components", "best")


def _hand_names():
    from tracks_cases import HAND
    return sorted(HAND)


@pytest.mark.parametrize("mode", TRACK_MODES)
@pytest.mark.parametrize("name", _hand_names())
def test_tracks_hand_made(hip, name, mode):
    from tracks_cases import hand_batch
    batch, e, thr, mh = hand_batch(name)
    pid = np.arange(batch.n_hits, dtype=np.int64) // 2 - 1
    check(_tracks_call(batch.cuda(), torch.as_tensor(e).cuda(), thr, mode, mh, pid))


@pytest.mark.parametrize("mode", TRACK_MODES)
@pytest.mark.parametrize("n_hits", [0, 1, 255, 256, 257])
def test_tracks_across_the_block_size(hip, n_hits, mode):
    from test_gpu_tracks import random_batch
    batch, scores = random_batch(n_hits, n_hits // 2 + (3 if n_hits else 0), seed=n_hits)
    pid = np.random.default_rng(3).integers(-2, 40, size=n_hits)
    check(_tracks_call(batch.cuda(), torch.from_numpy(scores).cuda(), 0.3, mode, 2, pid))


@pytest.mark.parametrize("mode", TRACK_MODES)
def test_tracks_barrel(hip, mode):
    from tracks_cases import barrel_batch
    batch, scores, pid = barrel_batch((40, 40, 2, 1, 3), torch.device("cuda", torch.cuda.current_device()))
    check(_tracks_call(batch, scores, 0.5, mode, 3, _np(pid)))


# ---- the graph-convolution classifiers ----------------------------------------------------------------------------
def _gcn_case(kind):
    from gnn_fpga_amd import synth
    from gnn_fpga_amd.gcn import GCNBinaryClassifier, GCRNBinaryClassifier, GraphConv
    if kind == "segments":              # gnn/GCN_Seg_Toy2D.ipynb: five self-interacting layers of 16
        X, A, y = synth.toy_segment_graphs(8, seed=5)
        make = lambda: GCNBinaryClassifier(5, [16] * 5)                     # noqa: E731
    else:                               # gnn/GCN_Toy2D.ipynb: twelve residual layers of 8
        X, A, y = synth.toy_hit_graphs(8, seed=5, norm="row")
        make = lambda: GCRNBinaryClassifier(3, [8] * 12, gc_type=GraphConv)  # noqa: E731
    return X, A, y, make


@pytest.mark.parametrize("kind", ["segments", "hits"])
def test_gcn(hip, kind):
    from gnn_fpga_amd.autograd import gcn_forward_layers
    from gnn_fpga_amd.gcn import compress_adjacency
    X, A, y, make = _gcn_case(kind)
    torch.manual_seed(3)
    model = make().cuda().train()
    x, a = torch.from_numpy(X).float().cuda(), torch.from_numpy(A).float().cuda()
    w = torch.linspace(0.5, 1.5, y.size, device="cuda").view(y.shape)

    def call():
        adj = compress_adjacency(a)                                         # gnn_gcn_compress_count / _fill
        model.zero_grad(set_to_none=True)
        logits = model(x, adj)                                              # gnn_gcn_forward, H_all kept
        (logits * w).sum().backward()                                       # gnn_gcn_backward
        grads = [p.grad.clone() for p in model.parameters()]
        _, layers = gcn_forward_layers(model, x, adj)
        return [adj.row_cnt, adj.row_idx, adj.row_val, adj.col_cnt, adj.col_idx, adj.col_val, logits.detach(), grads,
                layers]

    got = check(call)
    dense = _np(a)
    cnt = _np(got[0])
    assert np.array_equal(cnt, (dense != 0).sum(axis=2))                    # the lists against the dense matrix
    idx, val = _np(got[1]), _np(got[2])
    back = np.zeros_like(dense)
    B, N, W = idx.shape
    for k in range(W):
        live = k < cnt
        bb, nn = np.nonzero(live)
        back[bb, nn, idx[bb, nn, k]] = val[bb, nn, k]
    assert np.array_equal(back, dense)


# ---- the graph builder, the cut study and the layer census --------------------------------------------------------
def _barrel_columns(edges):
    """synth.barrel_event(40, 40, 2); `edges`: the same columns between an empty first and an empty last event, with a
    third event whose hits (the first event's, again) all sit on layer 3."""
    from gnn_fpga_amd import synth
    cols = synth.barrel_event(40, 40, 2, seed=31)
    if not edges:
        return cols
    n0 = int(cols.event_ptr[1])
    cat = lambda a, one=None: np.concatenate([a, a[:n0] if one is None else np.full(n0, one, a.dtype)])  # noqa: E731
    n = cols.r.shape[0] + n0
    ptr = np.array([0, 0, cols.event_ptr[1], cols.event_ptr[2], n, n], dtype=np.int64)
    return synth.HitColumns(cat(cols.r), cat(cols.phi), cat(cols.z), cat(cols.layer, 3), cat(cols.particle_id), ptr)


def _columns_on_device(cols):
    from gnn_fpga_amd import synth
    return synth.HitColumns(*(torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in cols[:5]), cols.event_ptr)


BARREL_PAIRS = np.stack([np.arange(9), np.arange(1, 10)], axis=1)


@pytest.mark.parametrize("edges", [False, True], ids=["two_events", "empty_and_one_layer_events"])
@pytest.mark.parametrize("sectors", [1, 2])
def test_graph_build(hip, sectors, edges):
    from gnn_fpga_amd.graph_build import build_graphs
    cols = _barrel_columns(edges)
    d = _columns_on_device(cols)
    host = build_graphs(cols.r, cols.phi, cols.z, cols.layer, BARREL_PAIRS, particle_id=cols.particle_id,
                        event_ptr=cols.event_ptr, n_phi_sectors=sectors)
    ptrs = []

    def call():
        b = build_graphs(d.r, d.phi, d.z, d.layer, BARREL_PAIRS, particle_id=d.particle_id, event_ptr=cols.event_ptr,
                         n_phi_sectors=sectors)                             # gnn_graph_build_sizes / _fill
        ptrs.append((b.hit_ptr.copy(), b.seg_ptr.copy()))
        return [b.X, b.src, b.dst, b.y, b.hit_index]

    X, src, dst, y, hit_index = check(call)
    for hp, sp in ptrs:
        assert np.array_equal(hp, host.hit_ptr) and np.array_equal(sp, host.seg_ptr)
    assert _np(X).tobytes() == host.X.numpy().tobytes() and _np(y).tobytes() == host.y.numpy().tobytes()
    assert np.array_equal(_np(src), host.src.numpy()) and np.array_equal(_np(dst), host.dst.numpy())
    assert np.array_equal(_np(hit_index), host.hit_index.numpy())
    assert host.n_segments > 0 and (not edges or np.count_nonzero(np.diff(host.seg_ptr) == 0) >= 3 * sectors)


@pytest.mark.parametrize("edges", [False, True], ids=["two_events", "empty_and_one_layer_events"])
@pytest.mark.parametrize("sectors", [1, 2])
def test_cut_study_and_layer_census(hip, sectors, edges):
    from gnn_fpga_amd import count_layer_transitions, study_segment_cuts
    from test_cut_study_host import SLOPE_EDGES, Z0_EDGES
    cols = _barrel_columns(edges)
    d = _columns_on_device(cols)
    kw = dict(event_ptr=cols.event_ptr, n_phi_sectors=sectors, phi_slope_edges=SLOPE_EDGES, z0_edges=Z0_EDGES)
    host = study_segment_cuts(cols.r, cols.phi, cols.z, cols.layer, BARREL_PAIRS, cols.particle_id, **kw)
    census = count_layer_transitions(cols.r, cols.layer, cols.particle_id, event_ptr=cols.event_ptr, n_layers=10)

    def call():
        s = study_segment_cuts(d.r, d.phi, d.z, d.layer, BARREL_PAIRS, d.particle_id, **kw)         # gnn_cut_study
        c = count_layer_transitions(d.r, d.layer, d.particle_id, event_ptr=cols.event_ptr, n_layers=10)
        many = count_layer_transitions(d.r, d.layer, d.particle_id, event_ptr=cols.event_ptr, n_layers=70)
        return [s.counts, c, many]

    counts, c, many = check(call)
    assert np.array_equal(_np(counts), host.counts.numpy()) and int(host.counts.sum()) > 0
    assert np.array_equal(_np(c), census.numpy()) and int(census.sum()) > 0
    assert np.array_equal(_np(many)[:10, :10], census.numpy()) and int(many.sum()) == int(census.sum())


# ---- the toy notebooks' graph builders ----------------------------------------------------------------------------
def _toy_adj(adj):
    return [adj.row_cnt, adj.row_idx, adj.row_val, adj.col_cnt, adj.col_idx, adj.col_val]


@pytest.mark.parametrize("norm", [None, "row", "kw"])
@pytest.mark.parametrize("source", ["fixture", "synthetic"])
def test_toy_hit_graphs(hip, source, norm):
    import toy_graphs_fixtures as fx
    from gnn_fpga_amd import synth, toy_graphs
    from test_gpu_toy_graphs import DET_R, check_hits, expected_width, synth_hits
    if source == "fixture":                                 # the smallest of tests/golden/toy_graphs
        d = fx.load("hits_l2_t1")
        det_r, seed_size = d["det_r"], int(d["seed_size"])
        L = det_r.shape[0]
        x, y = np.array(d["hit_x"]), np.array(d["hit_y"])
        want = (d["X"], fx.dense(d, norm or "none"), d["y0"], d["iso_rows"].shape[0])
    else:
        L, seed_size = 10, 3
        det_r = DET_R[L]
        x, y = synth_hits(7, L, 5, seed=14)
        x, y = x.copy(), y.astype(np.int32)
        x[0, 0] = 0.0                                                       # (an isolated hit)
        X, A, y0 = synth.toy_hit_graphs_from_hits(x, y, det_r=det_r, seed_size=seed_size, norm=norm)
        binary = synth.toy_hit_graphs_from_hits(x, y, det_r=det_r, norm=None)[1]
        want = (X, A, y0, int((binary.sum(axis=1) == 0).sum()))
    T = x.shape[1] // L
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    W = expected_width("hits", L, T, norm)

    def call():
        got = toy_graphs.build_toy_hit_graphs(xd, yd, det_r=det_r, seed_size=seed_size, norm=norm)
        check_hits(got, *want, W)                                           # bit for bit, in every run
        return [got.X, got.y0, got.n_isolated] + _toy_adj(got.adj)
    check(call)


@pytest.mark.parametrize("source", ["fixture", "synthetic"])
def test_toy_segment_graphs(hip, source):
    import toy_graphs_fixtures as fx
    from gnn_fpga_amd import synth, toy_graphs
    from test_gpu_toy_graphs import DET_R, check_segments, expected_width, structure, synth_hits
    if source == "fixture":
        d = fx.load("seg_l2_t1")
        det_r, kw = d["det_r"], dict(sigma=float(d["sigma"]))
        L = det_r.shape[0]
        x, y = np.array(d["hit_x"]), np.array(d["hit_y"])
        mask = np.zeros(tuple(d["A_shape"]), bool)
        mask[d["A_batch"], d["A_rows"], d["A_cols"]] = True
        want = (d["X"], fx.dense(d), d["y"], mask)
    else:
        L, kw = 10, {}
        det_r = DET_R[L]
        x, y = synth_hits(7, L, 5, seed=18)
        want = synth.toy_segment_graphs_from_hits(x, y, det_r=det_r) + (structure(L, 5),)
    T = x.shape[1] // L
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()

    def call():
        got = toy_graphs.build_toy_segment_graphs(xd, yd, det_r=det_r, **kw)
        check_segments(got, *want, expected_width("seg", L, T), "poisoned_alloc %s" % source)
        return [got.X, got.y] + _toy_adj(got.adj)[:3]
    check(call)


# ---- the four detector graph builders: the smallest fixture of each golden directory and a seeded synthetic input -
def _smallest(directory):
    import glob
    files = glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", directory, "*.npz"))
    return os.path.basename(min(files, key=os.path.getsize))[:-4]


def _cols_dev(cols):
    return [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in cols]


def _selection(sel):
    return [getattr(sel, k) for k in ("r", "phi", "z", "layer", "particle_id", "hit_id", "row")]


@pytest.mark.parametrize("source", ["fixture", "synthetic"])
def test_select_hits(hip, source):
    import select_hits_fixtures as sf
    from gnn_fpga_amd import select_hits, synth
    dev = torch.device("cuda", torch.cuda.current_device())
    if source == "fixture":
        f = sf.load(_smallest("select_hits"))
        tables = sf.tables(f, dev)
        phi = torch.from_numpy(f["phi"]).to(dev)
        kw = dict(pt_min=float(f["pt_min"]), no_missing_hits=bool(f["no_missing_hits"]))
        verify = lambda sel: sf.assert_equals_reference(sel, f)               # noqa: E731
    else:                               # three events (the second without truth rows: nothing selected there)
        from test_gpu_select_hits import _without_truth_of
        ev = _without_truth_of(synth.trackml_events(3, 40, 120, seed=47, missing=0.3), 1)
        assert ev["hits"]["x"].shape[0] <= 2000
        host_phi = np.arctan2(ev["hits"]["y"], ev["hits"]["x"])
        kw = dict(pt_min=0.5)
        spec = select_hits(ev["hits"], ev["truth"], ev["particles"], phi=host_phi, **kw)
        assert len(spec) > 0 and np.any(np.diff(spec.event_ptr) == 0)
        tables, phi = sf.to_device(ev, dev), torch.from_numpy(host_phi).to(dev)
        verify = lambda sel: sf.assert_same(sel, spec)                      # noqa: E731

    def call():
        sel = select_hits(*tables, phi=phi, **kw)                           # gnn_select_hits_sizes / _fill
        verify(sel)
        own_phi = select_hits(*tables, **kw)                                # phi by the device's atan2f
        return [_selection(sel), _selection(own_phi)]
    check(call)


@pytest.mark.parametrize("source", ["fixture", "synthetic"])
def test_hit_samples(hip, source):
    from gnn_fpga_amd import build_hit_samples, synth
    from test_gpu_hit_samples import COLS, GOLD, _compare
    if source == "fixture":
        f = dict(np.load(os.path.join(GOLD, _smallest("hit_samples") + ".npz")))
        cols, ep = [f[k] for k in COLS], f["event_ptr"]
        kw = dict(n_det_layers=int(f["n_det_layers"]), n_layer_hits=int(f["n_layer_hits"]),
                  n_seed_layers=int(f["n_seed_layers"]))

        def verify(s):
            X, Ri, Ro, y = s.dense()
            assert np.array_equal(_np(s.keys), f["sig_keys"]) and np.array_equal(y, f["full_y"])
            assert np.array_equal(X.view(np.uint32), f["full_X"].view(np.uint32))
            assert np.array_equal(Ri, f["full_Ri"]) and np.array_equal(Ro, f["full_Ro"])
    else:                               # two events and an empty one between them
        ev = synth.barrel_event(60, 300, n_events=2, seed=103)
        assert ev.r.shape[0] <= 2000
        cols = [ev.r, ev.phi, ev.z, ev.layer, ev.particle_id]
        ep = np.array([ev.event_ptr[0], ev.event_ptr[1], ev.event_ptr[1], ev.event_ptr[2]], dtype=np.int64)
        kw = dict(n_layer_hits=5, n_seed_layers=3)
        host = build_hit_samples(*cols, event_ptr=ep, **kw)
        assert len(host) > 0
        verify = lambda s: _compare(cols, ep, host, s, 10, 5)               # noqa: E731  (near-tie swaps only)
    d = _cols_dev(cols)

    def call():
        s = build_hit_samples(*d, event_ptr=ep, **kw)                       # gnn_hit_samples_sizes / _fill
        verify(s)
        return [s.batch.X, s.batch.src, s.batch.dst, s.y, s.hit_index, s.keys]
    check(call)


@pytest.mark.parametrize("source", ["fixture", "synthetic"])
def test_event_graphs(hip, source):
    import event_graphs_fixtures as ef
    from gnn_fpga_amd import build_event_graphs, synth
    from test_gpu_event_graphs import _same
    if source == "fixture":
        f = ef.load(_smallest("event_graphs"))
        d = _cols_dev([f[k] for k in ef.COLS])
        build = lambda: ef.build(f, cols=d)                                 # noqa: E731
        verify = lambda g: ef.assert_equals_reference(g, f)                 # noqa: E731
    else:                               # four events and an empty one after the first
        ev = synth.acts_events(4, 20, 40, seed=231)
        assert ev.r.shape[0] <= 2000
        ep = np.concatenate([ev.event_ptr[:2], ev.event_ptr[1:]]).astype(np.int64)
        host = build_event_graphs(*ev[:6], ep)
        assert len(host) > 0 and host.batch.n_segments > 0
        d = _cols_dev(ev[:6])
        build = lambda: build_event_graphs(*d, ep)                          # noqa: E731
        verify = lambda g: _same(g, host)                                   # noqa: E731

    def call():
        g = build()                                                         # gnn_event_graphs_sizes / _fill
        verify(g)
        b = g.batch
        return [b.X, b.src, b.dst, b.y, g.event_index, g.hit_index, g.layer]
    check(call)


@pytest.mark.parametrize("layout", ["flat", "padded"])
@pytest.mark.parametrize("source", ["fixture", "synthetic"])
def test_muon_graphs(hip, source, layout):
    from gnn_fpga_amd import build_muon_graphs, synth
    from test_gpu_muon_graph import _dev, _host, _vp, assert_same
    from test_muon_graph_host import assert_matches_case, load_case
    if source == "fixture":
        case = load_case(_smallest("muon_graph"))
        mu, pu, vpt, veta, start, muon_only = case[:6]
        want = build_muon_graphs(mu, pu, vpt, veta, entry_start=start, muon_only=muon_only, layout=layout)
    else:                               # 45 entries, one without any row, the last two without a vp row
        dd = synth.emtf_events(45, seed=21)
        mu, pu, start, muon_only = dd["muon"], dd["pu"], 3, False
        for t in (mu, pu):
            ep = t["event_ptr"]
            keep = np.ones(int(ep[-1]), bool)
            keep[ep[7]:ep[8]] = False
            new = ep.copy()
            new[8:] -= ep[8] - ep[7]
            for k in list(t):
                t[k] = new if k == "event_ptr" else t[k][keep]
        assert int(mu["event_ptr"][-1]) + int(pu["event_ptr"][-1]) <= 2000
        vpt, veta = dd["vp_pt"][:43], dd["vp_eta"][:43]
        want = build_muon_graphs(mu, pu, vpt, veta, entry_start=start, muon_only=muon_only, layout=layout)
        case = None
    args = (_dev(mu), _dev(pu), *_vp(vpt, veta))

    def call():
        res = build_muon_graphs(*args, entry_start=start, muon_only=muon_only, layout=layout)   # gnn_muon_graph_*
        got = _host(res)
        assert_same(got, want)                                              # the specification, bit for bit
        if case is not None and layout == "flat":
            assert_matches_case(got, case)                                  # and the reference's graphs
        b = res.batch
        return [b.X, b.src, b.dst, b.y, res.entry, res.pt, res.eta, res.written, res.vp_missing, res.hit_source,
                res.hit_row, res.present, res.n_hits, res.n_segments]
    check(call)


def test_gcn_layers_of_unequal_width(hip):
    """H_all [B, n_dims, N, max_width] as gnn_gcn_forward itself fills it, with layers narrower than the widest one."""
    from gnn_fpga_amd import _lib, synth
    from gnn_fpga_amd.autograd import _gcn_net
    from gnn_fpga_amd.gcn import GCRNBinaryClassifier, compress_adjacency
    X, A, _ = synth.toy_hit_graphs(3, seed=11, norm="row")
    dims = [5, 7, 3]
    torch.manual_seed(4)
    model = GCRNBinaryClassifier(3, dims).cuda()
    w = [p.detach().float().contiguous() for p in model.parameters()]
    x, adj = torch.from_numpy(X).float().cuda(), compress_adjacency(torch.from_numpy(A).float().cuda())
    go = torch.linspace(0.5, 1.5, X.shape[0] * X.shape[1], device="cuda").view(X.shape[0], X.shape[1])

    def call():
        net = _gcn_net(model, w)
        out, H_all = _lib.gcn_forward(adj, net, x, train=True)
        grads = _lib.gcn_backward(adj, net, x, H_all, go)                   # (reads the kept layers as they are)
        kept = H_all.clone()
        # THE ONE MASKED REGION OF THIS FILE - H_all's columns past a layer's own width: include/gnn_hip.h documents
        # them as unspecified.  No reader can need them (the backward reads dims[l] columns of layer l, and
        # autograd.gcn_forward_layers hands out exactly those); writing them would add stores to the one-launch
        # forward for every layer narrower than the widest
        for l, d in enumerate(dims):
            kept[:, l, :, d:] = 0
        return [out, kept, grads]
    check(call)
