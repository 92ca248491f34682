"""Every HIP entry point on arrays that start off the 16-byte grid (tests/offset_arrays.py).

Every other GPU file hands the kernels tensors fresh from torch's caching allocator, whose blocks start on 512 bytes.
The product does not: a GraphStore window's X starts at a multiple of 12 bytes, a GradBucket's gradients and a
flat-parameter model's weights are packed back to back.  The kernels read hit rows, kept layers and biases 16 bytes at a
time through reinterpret_cast, which promises the compiler an alignment nobody checks (the sites: INTEGRATION.md,
"Alignment").  Here the catalogue of test_gpu_uninitialised.py runs again, one group per section of that file, through
one function, `sweep(call)`: `call(S)` runs public wrappers with every caller-supplied device array passed through
`S(...)` (inputs) or made by `S.empty(...)` (`out=`, `into=`, `workspace=` targets between guard bands), once per mode
of offset_arrays.MODES - k = 0 (fresh copies on the grid), k = 1, 2, 3 (8-byte element types: 1), "mixed" (1, 2, 3,
0, 1, ... over the arrays of the call, which catches a guard that looks at one pointer only) and that sequence begun
one, two and three places later, so that every array of a call is once the aligned one among shifted neighbours.

The assertions take no tolerance.  Every output of a shifted run has the bits of the k = 0 run (`_assert_same` names
the first differing element) and the bytes either side of every target are untouched.  Integer outputs of the k = 0 run
are also compared with the numpy specification the package ships, as test_gpu_uninitialised.py does; float outputs
rest on the k = 0 run, which the other GPU files pin to float64.  Kept training tensors (e_all, H_all, Q_all, y) are
re-seated - copied to shifted addresses - between the forward that wrote them and the backward that reads them.
While a call runs, `offset_arrays.shifted_alloc` also puts every allocation the binding makes itself - the outputs the
kernels STORE 16 bytes at a time (H, Hnext, H_all, Q_all, grad_H, the builders' X), gradient buffers, every workspace -
at the call's next offset between guard bands: the Python wrappers take no `out=` for those, a C caller owns them.

Left out (shapes only, never a k): the shape matrix beyond the 19 recorded backward cases.
Not swept - arrays that other modules of the package make and that stay where torch put them: the arrays of a gnn_plan_t
and the plan builder's workspace (plan_hip; INTEGRATION.md says what a C caller owes for the former); the six segment
lists of a gnn_graph_t (views of gnn_csr_build's two shifted blocks, so off the grid only as the list lengths fall);
the device hit_ptr / seg_ptr of the one-launch entry points (hitgraph._EventLayout); seg_ptr, tw_src and tw_dst of
gnn_segclf_forward_train_plan (HitGraphBatch.level_ordered) - all int32 arrays the kernels read one element at a time;
a model's own `_workspace` (model.py) beyond the three workspace= targets handed in here.  Workspaces move in steps of
4 bytes, not to every address.

COVERS maps every entry point of _lib.SIGNATURES that takes a device pointer to the test here that shifts its arrays;
test_offset_arrays_host.py holds the table to the signatures.
"""
import copy
import functools
import os

import numpy as np
import pytest
import torch

import route_cases as rc
from offset_arrays import COVERS, MODES, NO_ARRAYS, Shift, shift_batch, shift_params, shifted_alloc  # noqa: F401
from test_gpu_uninitialised import (BARREL_PAIRS, EVENT_SHAPES, FWD_SHAPES, MODEL_ROUTES, PLAN_CASES, PLAN_MODES, T_FWD,
                                    _assert_lists, _assert_same, _barrel_columns, _edge_graphs, _env, _flat, _gcn_case,
                                    _host_batch, _np, _smallest, _toy_adj)

pytestmark = pytest.mark.gpu


def sweep(call, shifts=True, device="cuda", allocates=True):
    """`call(S)` once per mode.  Every shifted run: the k = 0 run's bits, every target's guard bands intact.  Returns
    the k = 0 run's outputs (flat).  (`device`: "cpu" in test_offset_arrays_host.py, which holds this function to
    noticing an address-dependent result and a write outside a target.)"""
    base = None
    for mode in MODES:
        S = Shift(mode, device)
        with shifted_alloc(S):                              # the binding's own outputs and workspaces: shifted too
            got = [t.clone() for t in _flat(call(S))]
        assert S.allocated > 0 or not allocates, "the binding allocated nothing through the proxy"
        if device == "cuda":
            torch.cuda.synchronize()
        damaged = S.guards_intact()
        assert damaged == [], "mode %r: bytes next to target(s) %s of the call were overwritten" % (mode, damaged)
        assert S.ks, "the call handed nothing through S"
        if mode == 0:
            assert not any(S.ks)
            base = got
        else:
            # (a rotation of the mixed sequence may begin with its 0: a call with fewer than four arrays may see no shift)
            assert not shifts or any(S.ks) or (isinstance(mode, str) and len(S.ks) < 4)
            _assert_same(base, got, "arrays at k = %r against k = 0" % (mode,))
    return base


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _filled(S, like):
    """A guarded target holding `like`'s values (an `into=` prefill, a zeroed counter)."""
    t = S.empty(tuple(like.shape), dtype=like.dtype)
    t.copy_(like)
    return t


@functools.lru_cache(maxsize=None)
def _cached_host_batch(F, big=True):
    return _host_batch(F, big)              # (shift_batch reads it; nothing moves it)


# ---- the training forwards and every backward route ---------------------------------------------------------------
def _backward_call(case, into=False):
    from gnn_fpga_amd import _lib
    F, D, T, kind = case["F"], case["D"], case["T"], case["kind"]
    hb, hw, go = rc.host_batch(case), rc.host_weights(case), rc.upstream(case)
    head = rc.head(case) if kind == "nodeclf" else None
    pre = rc.prefill(case) if into else None

    def call(S):
        b = shift_batch(hb, S)
        w = S([t.cuda() for t in hw])
        target = [_filled(S, v.cuda()) for v in pre] if into else None
        if kind == "nodeclf":
            Wo, bo = S(head[0].cuda()), S(head[1].cuda())
            kept = _lib.nodeclf_forward_train(b, w, Wo, bo, F, D, T, keep_q=case["q"])
            e_all, H_all, Q_all, y = (S(t) for t in kept)                   # re-seated
            grads, gWo, gbo = _lib.nodeclf_backward(b, w, Wo, bo, F, D, T, e_all, H_all, y, S(go.cuda()), Q_all=Q_all)
            return [kept, grads, gWo, gbo]
        if kind == "events":
            lay = b.event_layout()
            kept = _lib.segclf_forward_train(b, w, F, D, T, layout=lay)[:2]
            e_all, H_all = (S(t) for t in kept)
            return [kept, _lib.segclf_backward_events(b, lay, w, F, D, T, e_all, H_all, S(go.cuda()), into=target)]
        kept = _lib.segclf_forward_train(b, w, F, D, T)
        if not isinstance(S.mode, str):                     # written by the forward at the binding's shifted addresses
            assert all(t.data_ptr() % 16 == 4 * S.mode for t in kept[1:] if t.numel())
        e_all, H_all, Q_all = (S(t) for t in kept)
        if kind == "edge":
            return [kept, _lib.edge_bwd(S(H_all[0]), b, w, F, D, S(e_all[0]), S(go.cuda()))]
        if kind == "node":
            full = torch.zeros_like(H_all[1])               # rows of H_all's stride, the first D columns used
            full[:, :D] = go.cuda()
            return [kept, _lib.node_bwd(S(H_all[0]), S(e_all[0]), S(H_all[1]), b, w, F, D, S(full))]
        return [kept, _lib.segclf_backward(b, w, F, D, T, e_all, H_all, S(go.cuda()), into=target,
                                           Q_all=Q_all if case["q"] else None)]
    return call


@pytest.mark.parametrize("case", rc.bwd.CASES, ids=[rc.case_id(c) for c in rc.bwd.CASES])
def test_training_forward_and_backward(hip, case):
    with rc.bwd.switch(case["env"]):
        sweep(_backward_call(case))


@pytest.mark.parametrize("name", rc.INTO_CASES, ids=[n.replace(" ", "_") for n in rc.INTO_CASES])
def test_backward_into_the_callers_tensors(hip, name):
    case = rc.case_named(name)
    with rc.bwd.switch(case["env"]):
        sweep(_backward_call(case, into=True))


# ---- the fused forward on a plan built from the shifted batch -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plan_graphs(F, big):
    from gnn_fpga_amd import HitGraphBatch, synth
    if big:
        graphs = [synth.layered_graph(33000, 200000, F, seed=70)]
    else:
        graphs = [synth.layered_graph(900, 6000, F, seed=70 + i) for i in range(3)]
        graphs.append(synth.layered_graph(5, 4, F, n_layers=2, seed=9))
    return HitGraphBatch.from_graphs(graphs)


def _plan_weights(case):
    from gnn_fpga_amd.model import SegmentClassifier
    torch.manual_seed(3 * case["D"] + case["T"])
    model = SegmentClassifier(input_dim=case["F"], hidden_dim=case["D"], n_iters=case["T"])
    return [t.detach().contiguous() for t in model.effective_weights()]


@pytest.mark.parametrize("case", rc.fwd.CASES, ids=[rc.case_id(c) for c in rc.fwd.CASES])
def test_plan_build_and_fused_forward(hip, case):
    """rc.fwd.build_inputs / run_inputs restated over shifted arrays: the plan is built from the shifted batch, the
    forward runs on shifted weights into a guarded `out=` on a guarded `workspace=`."""
    F, D, T = case["F"], case["D"], case["T"]
    hb, hw = _plan_graphs(F, case["big"]), _plan_weights(case)

    def call(S):
        b = shift_batch(hb, S)
        w = S([t.cuda() for t in hw])
        plan = b.build_plan(D, case["limits"])              # gnn_plan_build_sizes_graphs / _fill on the shifted arrays
        with rc.fwd._switch(case["env"]):
            if case["train"]:
                twin = b.level_ordered(D)
                assert twin._fused is plan
                return list(hip.segclf_forward_train_fused(twin, w, F, D, T))
            flags = 0
            if case["xp"]:
                assert hip.exp_product_bound(w, F, D, plan.x_absmax) <= 60.0
                flags |= hip.GNN_FLAG_EXP_PRODUCT
            if case["bf16"]:
                flags |= hip.GNN_FLAG_BF16_MLP
            ws = S.empty(hip.plan_workspace_bytes(plan.n_pad, plan.n_segments, F, D), dtype=torch.uint8)
            first = hip.segclf_forward_plan(plan, w, F, D, T, out=S.empty(plan.n_segments), workspace=ws, flags=flags)
            params = hip.params_struct(w, F, D, flags)
            second = hip.segclf_forward_plan(plan, w, F, D, T, flags=flags, params=params)
            return [first, second]
    got = sweep(call)
    if not case["train"]:
        assert torch.equal(got[0], got[1])


# ---- the per-module forwards, the list builder and the dense adapter ----------------------------------------------
def _host_weights(F, D, T=T_FWD):
    from gnn_fpga_amd.model import SegmentClassifier
    torch.manual_seed(7 * D + F)
    m = SegmentClassifier(input_dim=F, hidden_dim=D, n_iters=T)
    w = [t.detach().contiguous() for t in m.effective_weights()]
    g = torch.Generator().manual_seed(11 * D + F)
    return w, 0.3 * torch.randn(1, F + D, generator=g), torch.randn(1, generator=g)


@pytest.mark.parametrize("F,D", FWD_SHAPES, ids=["%dx%d" % s for s in FWD_SHAPES])
def test_per_module_forwards(hip, F, D):
    hw, hWo, hbo = _host_weights(F, D)
    host = _cached_host_batch(F)
    trace = (F, D) == (3, 8)
    ldh = hip.h_stride(F, D)

    def call(S):
        b = shift_batch(host, S)
        w, Wo, bo = S([t.cuda() for t in hw]), S(hWo.cuda()), S(hbo.cuda())
        parts = hip.csr_build(b.src, b.dst, b.n_hits)
        need = hip.workspace_bytes(b.n_hits, b.n_segments, F, D)
        out = hip.segclf_forward(b, w, F, D, T_FWD, out=S.empty(b.n_segments),
                                 workspace=S.empty(need, dtype=torch.uint8))
        traced = hip.segclf_forward(b, w, F, D, T_FWD, trace=True) if trace else None
        y = hip.nodeclf_forward(b, w, Wo, bo, F, D, T_FWD, workspace=S.empty(need, dtype=torch.uint8), trace=trace)
        H = hip.input_fwd(b.X, w[0], w[1])
        e = hip.edge_fwd(S(H), b.src, b.dst, *w[2:6], F, D)
        Hn = hip.node_fwd(S(H), S(e), b, *w[6:10], F, D)
        if not isinstance(S.mode, str):                     # the rows the kernels store 16 bytes at a time: off the grid
            assert H.data_ptr() % 16 == Hn.data_ptr() % 16 == 4 * S.mode
        return [parts, out, traced, y, H, e, Hn]

    plain = sweep(call)
    _assert_lists(plain[:7], host.src.numpy(), host.dst.numpy(), host.n_hits)
    H = plain[-3]
    assert H.shape == (host.n_hits, ldh) and not bool(torch.isnan(H).any())
    assert bool((H[:, F + D:] == 0).all())


@pytest.mark.parametrize("F,D", EVENT_SHAPES, ids=["%dx%d" % s for s in EVENT_SHAPES])
def test_one_launch_forward(hip, F, D):
    hw, _, _ = _host_weights(F, D)
    host = _cached_host_batch(F, False)

    def call(S):
        b = shift_batch(host, S)
        w = S([t.cuda() for t in hw])
        fresh = hip.segclf_forward_events(b, b.event_layout(), w, F, D, T_FWD, out=S.empty(b.n_segments))
        b.in_ptr                                            # the batch's lists (gnn_csr_build), then the same call
        listed = hip.segclf_forward_events(b, b.event_layout(), w, F, D, T_FWD, out=S.empty(b.n_segments),
                                           params=hip.params_struct(w, F, D))
        return [fresh, listed]

    fresh, listed = sweep(call)
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
    src, dst, flags = sweep(lambda S: hip.dense_to_index(S(Rid), S(Rod)))
    assert np.array_equal(_np(src), want.src.numpy()) and np.array_equal(_np(dst), want.dst.numpy())
    assert int(flags.item()) == 0


# ---- the loss -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want_grad", [True, False], ids=["grad", "no_grad"])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 100003])
def test_bce_loss(hip, n, want_grad):
    g = torch.Generator().manual_seed(n)
    e = torch.rand(n, generator=g)
    y = (torch.rand(n, generator=g) < 0.3).float()
    for k, (v, t) in enumerate(((0.0, 0.0), (0.0, 1.0), (1.0, 0.0), (1.0, 1.0))):    # the clamps' edges
        if n:
            at = (k * (n - 1)) // 3
            e[at], y[at] = v, t
    ed, yd = e.cuda(), y.cuda()
    for scale in (1.0 / max(n, 1), 1.0):                    # "mean", "sum"
        got = sweep(lambda S: hip.bce_loss(S(ed), S(yd), scale, want_grad=want_grad), shifts=n > 0)
        assert got[0].shape == (1,) and bool(torch.isfinite(got[0]).all()) and len(got) == 1 + want_grad


# ---- the plan builder's two calls, array for array against plan.SellPlan ------------------------------------------
@pytest.mark.parametrize("mode", sorted(PLAN_MODES))
@pytest.mark.parametrize("case", PLAN_CASES)
def test_plan_builder(hip, case, mode):
    from gnn_fpga_amd.plan import SellPlan
    from gnn_fpga_amd.plan_hip import HipSellPlan
    from test_plan import _same_plan
    from test_plan_hip import case_batch
    hb, F, D, lim_over = case_batch(case)
    lim = hip.plan_limits(F, D)
    lim.update(lim_over)
    host = SellPlan(hb, lim)

    def call(S):
        dev = HipSellPlan(shift_batch(hb, S), lim, debug=True)              # gnn_plan_build_sizes[_graphs] / _fill
        _same_plan(host, dev)                                               # every array, in every run
        return [getattr(dev, k) for k in dev._TENSORS] + list(dev._dbg)

    with _env(**dict({"GNN_PLAN_GRAPH_LOCAL": None, "GNN_PLAN_SCATTER_LISTS": None}, **PLAN_MODES[mode])):
        sweep(call)


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
    ed, yd, sd = _dev(e), _dev(y), _dev(src)
    spd = None if sp is None else _dev(sp)

    def call(S):
        counts = S.empty((len(thresholds) + 1, 2), dtype=torch.int64).zero_()  # the contract: zeroed
        hist = S.empty((2, n_bins), dtype=torch.int64).zero_()
        status = S.empty(1, dtype=torch.int32).zero_()
        pg = S.empty((sp.size - 1, len(thresholds) + 1, 2), dtype=torch.int64) if per_graph else None
        hip.segment_metrics_update(S(ed), S(yd), S(sd), thresholds, key_shift, counts, hist, status, S(spd), pg)
        return [counts, hist, status, pg]

    got = sweep(call, allocates=False)                      # (no workspace, and the counters are the caller's)
    assert int(got[2].item()) == spec["status"]
    assert np.array_equal(_np(got[0]), spec["counts"]) and np.array_equal(_np(got[1]), spec["hist"])
    if per_graph:
        assert np.array_equal(_np(got[3]), spec["per_graph"])


# ---- track candidates, their matching and their fit ---------------------------------------------------------------
def _tracks_call(host_batch, scores, threshold, mode, min_hits, pid):
    from tracks_cases import assert_match_equal, assert_tracks_equal, match_spec, spec_of
    from gnn_fpga_amd import build_tracks
    spec = spec_of(host_batch, scores, threshold, mode, min_hits)
    sd = scores.cuda() if torch.is_tensor(scores) else _dev(np.asarray(scores, np.float32))
    pd = _dev(np.asarray(pid, np.int64))

    def call(S):
        tracks = build_tracks(shift_batch(host_batch, S), S(sd), threshold, mode, min_hits)
        assert_tracks_equal(tracks, spec)
        outs = [tracks.track_of_hit, tracks.root_of_hit, tracks._sizes]
        if not spec["status"]:
            m = tracks.match(S(pd))                                         # gnn_track_build_lists, gnn_track_match
            assert_match_equal(m, match_spec(tracks, pid))
            outs += [tracks.track_ptr, tracks.track_hits, tracks.track_graph, tracks.graph_track_ptr,
                     m.majority_particle, m.majority_hits, m.particle_hits, m.matched, m.counts]
        return outs
    return call


def _track_cases():
    from tracks_cases import HAND
    return ["hand:" + k for k in sorted(HAND)] + [0, 1, 255, 256, 257, "barrel"]


TRACK_CASES = _track_cases()


@pytest.mark.parametrize("mode", ("components", "best"))
@pytest.mark.parametrize("which", TRACK_CASES, ids=[str(c).replace(":", "_") for c in TRACK_CASES])
def test_tracks(hip, which, mode):
    if which == "barrel":
        from tracks_cases import barrel_batch
        batch, e, pid = barrel_batch((40, 40, 2, 1, 3), torch.device("cuda", torch.cuda.current_device()))
        pid, thr, mh = _np(pid), 0.5, 3
    elif isinstance(which, str):
        from tracks_cases import hand_batch
        batch, e, thr, mh = hand_batch(which[5:])
        pid = np.arange(batch.n_hits, dtype=np.int64) // 2 - 1
    else:
        from test_gpu_tracks import random_batch
        batch, e = random_batch(which, which // 2 + (3 if which else 0), seed=which)
        pid, thr, mh = np.random.default_rng(3).integers(-2, 40, size=which), 0.3, 2
    sweep(_tracks_call(batch, e, thr, mode, mh, pid), shifts=batch.n_hits > 0)


@pytest.mark.parametrize("name", ["lengths", "mixed", "three_hits_257"])
def test_track_fit(hip, name):
    from gnn_fpga_amd.tracks import fit_tracks_numpy
    from track_fit_cases import KEYS, STATUS_CASES, assert_fit_equal, lengths_case, three_hit_tracks
    case = {"lengths": lengths_case, "mixed": lambda: STATUS_CASES["mixed"],
            "three_hits_257": lambda: three_hit_tracks(257)}[name]()
    ptr, hits, x, y, z, max_hits, _ = case
    ptr, hits = np.asarray(ptr, np.int32), np.asarray(hits, np.int32)
    cols = [np.asarray(v, np.float64) for v in (x, y, z)]
    d = [_dev(v) for v in [ptr, hits] + cols]
    got = sweep(lambda S: hip.track_fit(*(S(t) for t in d), max_hits))
    assert_fit_equal(dict(zip(KEYS, got)), fit_tracks_numpy(ptr, hits, *cols, max_hits))


# ---- the graph-convolution classifiers ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["segments", "hits"])
def test_gcn(hip, kind):
    """The adjacency, x, the model's parameters (one flat buffer, lead k) and the compressed lists (re-seated between
    gnn_gcn_compress_* and the model) shifted; the kept layers and the upstream gradient re-seated before the
    backward through _lib."""
    from gnn_fpga_amd.autograd import _gcn_net, gcn_forward_layers
    from gnn_fpga_amd.gcn import SparseAdjacency, compress_adjacency
    X, A, y, make = _gcn_case(kind)
    torch.manual_seed(3)
    proto = make().cuda().train()
    x, a = torch.from_numpy(X).float().cuda(), torch.from_numpy(A).float().cuda()
    wgt = torch.linspace(0.5, 1.5, y.size, device="cuda").view(y.shape)

    def call(S):
        model = copy.deepcopy(proto)
        shift_params(model, S.next_k(torch.float32))
        made = compress_adjacency(S(a))                                     # gnn_gcn_compress_count / _fill
        adj = SparseAdjacency(*(S(t) for t in _toy_adj(made)))
        xs = S(x)
        model.zero_grad(set_to_none=True)
        logits = model(xs, adj)                                             # gnn_gcn_forward, H_all kept
        (logits * wgt).sum().backward()                                     # gnn_gcn_backward
        grads = [p.grad.clone() for p in model.parameters()]
        _, layers = gcn_forward_layers(model, xs, adj)
        w = [p.detach() for p in model.parameters()]
        net = _gcn_net(model, w)
        out, H_all = hip.gcn_forward(adj, net, xs, train=True)
        flat = hip.gcn_backward(adj, net, xs, S(H_all), S(wgt.contiguous()))
        return [_toy_adj(made), logits.detach(), grads, layers, out, flat]

    got = sweep(call)
    assert np.array_equal(_np(got[0]), (_np(a) != 0).sum(axis=2))           # the lists' counts against the dense matrix


def test_gcn_layers_of_unequal_width(hip):
    from gnn_fpga_amd import synth
    from gnn_fpga_amd.autograd import _gcn_net
    from gnn_fpga_amd.gcn import GCRNBinaryClassifier, compress_adjacency
    X, A, _ = synth.toy_hit_graphs(3, seed=11, norm="row")
    dims = [5, 7, 3]
    torch.manual_seed(4)
    proto = GCRNBinaryClassifier(3, dims).cuda()
    x, adj = torch.from_numpy(X).float().cuda(), compress_adjacency(torch.from_numpy(A).float().cuda())
    go = torch.linspace(0.5, 1.5, X.shape[0] * X.shape[1], device="cuda").view(X.shape[0], X.shape[1])

    def call(S):
        model = copy.deepcopy(proto)
        shift_params(model, S.next_k(torch.float32))
        net = _gcn_net(model, [p.detach() for p in model.parameters()])
        xs = S(x)
        out, H_all = hip.gcn_forward(adj, net, xs, train=True)
        grads = hip.gcn_backward(adj, net, xs, S(H_all), S(go))
        kept = H_all.clone()
        for l, d in enumerate(dims):                        # columns past a layer's own width: documented unspecified
            kept[:, l, :, d:] = 0
        return [out, kept, grads]
    sweep(call)


# ---- the graph builder, the cut study and the layer census --------------------------------------------------------
def _columns_on_device(cols):
    return [_dev(c) for c in cols[:5]]


@pytest.mark.parametrize("edges", [False, True], ids=["two_events", "empty_and_one_layer_events"])
@pytest.mark.parametrize("sectors", [1, 2])
def test_graph_build(hip, sectors, edges):
    from gnn_fpga_amd.graph_build import build_graphs
    cols = _barrel_columns(edges)
    d = _columns_on_device(cols)
    host = build_graphs(cols.r, cols.phi, cols.z, cols.layer, BARREL_PAIRS, particle_id=cols.particle_id,
                        event_ptr=cols.event_ptr, n_phi_sectors=sectors)

    def call(S):
        r, phi, z, layer, pid = (S(t) for t in d)
        b = build_graphs(r, phi, z, layer, BARREL_PAIRS, particle_id=pid, event_ptr=cols.event_ptr,
                         n_phi_sectors=sectors)                             # gnn_graph_build_sizes / _fill
        assert np.array_equal(b.hit_ptr, host.hit_ptr) and np.array_equal(b.seg_ptr, host.seg_ptr)
        return [b.X, b.src, b.dst, b.y, b.hit_index]

    X, src, dst, y, hit_index = sweep(call)
    assert _np(X).tobytes() == host.X.numpy().tobytes() and _np(y).tobytes() == host.y.numpy().tobytes()
    assert np.array_equal(_np(src), host.src.numpy()) and np.array_equal(_np(dst), host.dst.numpy())
    assert np.array_equal(_np(hit_index), host.hit_index.numpy()) and host.n_segments > 0


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

    def call(S):
        r, phi, z, layer, pid = (S(t) for t in d)
        s = study_segment_cuts(r, phi, z, layer, BARREL_PAIRS, pid, **kw)                           # gnn_cut_study
        c = count_layer_transitions(r, layer, pid, event_ptr=cols.event_ptr, n_layers=10)
        many = count_layer_transitions(r, layer, pid, event_ptr=cols.event_ptr, n_layers=70)
        return [s.counts, c, many]

    counts, c, many = sweep(call)
    assert np.array_equal(_np(counts), host.counts.numpy()) and int(host.counts.sum()) > 0
    assert np.array_equal(_np(c), census.numpy()) and int(census.sum()) > 0
    assert np.array_equal(_np(many)[:10, :10], census.numpy()) and int(many.sum()) == int(census.sum())


# ---- the toy notebooks' graph builders ----------------------------------------------------------------------------
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
    xd, yd = _dev(x), _dev(y)
    W = expected_width("hits", L, T, norm)

    def call(S):
        got = toy_graphs.build_toy_hit_graphs(S(xd), S(yd), det_r=det_r, seed_size=seed_size, norm=norm)
        check_hits(got, *want, W)                                           # bit for bit, in every run
        return [got.X, got.y0, got.n_isolated] + _toy_adj(got.adj)
    sweep(call)


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
    xd, yd = _dev(x), _dev(y)

    def call(S):
        got = toy_graphs.build_toy_segment_graphs(S(xd), S(yd), det_r=det_r, **kw)
        check_segments(got, *want, expected_width("seg", L, T), "offset_arrays %s" % source)
        return [got.X, got.y] + _toy_adj(got.adj)[:3]
    sweep(call)


# ---- the four detector graph builders: the smallest fixture of each golden directory and a seeded synthetic input -
def _selection(sel):
    return [getattr(sel, k) for k in ("r", "phi", "z", "layer", "particle_id", "hit_id", "row")]


def _shift_tables(S, tables):
    return [{k: (v if k == "event_ptr" else S(v)) for k, v in tb.items()} for tb in tables]


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
        host_phi = np.arctan2(ev["hits"]["y"], ev["hits"]["x"])
        kw = dict(pt_min=0.5)
        spec = select_hits(ev["hits"], ev["truth"], ev["particles"], phi=host_phi, **kw)
        assert len(spec) > 0 and np.any(np.diff(spec.event_ptr) == 0)
        tables, phi = sf.to_device(ev, dev), torch.from_numpy(host_phi).to(dev)
        verify = lambda sel: sf.assert_same(sel, spec)                      # noqa: E731

    def call(S):
        tb = _shift_tables(S, tables)
        sel = select_hits(*tb, phi=S(phi), **kw)                            # gnn_select_hits_sizes / _fill
        verify(sel)
        own_phi = select_hits(*tb, **kw)                                    # phi by the device's atan2f
        return [_selection(sel), _selection(own_phi)]
    sweep(call)


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
        cols = [ev.r, ev.phi, ev.z, ev.layer, ev.particle_id]
        ep = np.array([ev.event_ptr[0], ev.event_ptr[1], ev.event_ptr[1], ev.event_ptr[2]], dtype=np.int64)
        kw = dict(n_layer_hits=5, n_seed_layers=3)
        host = build_hit_samples(*cols, event_ptr=ep, **kw)
        assert len(host) > 0
        verify = lambda s: _compare(cols, ep, host, s, 10, 5)               # noqa: E731  (near-tie swaps only)
    d = [_dev(c) for c in cols]

    def call(S):
        s = build_hit_samples(*(S(t) for t in d), event_ptr=ep, **kw)       # gnn_hit_samples_sizes / _fill
        verify(s)
        return [s.batch.X, s.batch.src, s.batch.dst, s.y, s.hit_index, s.keys]
    sweep(call)


@pytest.mark.parametrize("source", ["fixture", "synthetic"])
def test_event_graphs(hip, source):
    import event_graphs_fixtures as ef
    from gnn_fpga_amd import build_event_graphs, synth
    from test_gpu_event_graphs import _same
    if source == "fixture":
        f = ef.load(_smallest("event_graphs"))
        d = [_dev(f[k]) for k in ef.COLS]
        build = lambda cols: ef.build(f, cols=cols)                         # noqa: E731
        verify = lambda g: ef.assert_equals_reference(g, f)                 # noqa: E731
    else:                               # four events and an empty one after the first
        ev = synth.acts_events(4, 20, 40, seed=231)
        ep = np.concatenate([ev.event_ptr[:2], ev.event_ptr[1:]]).astype(np.int64)
        host = build_event_graphs(*ev[:6], ep)
        assert len(host) > 0 and host.batch.n_segments > 0
        d = [_dev(c) for c in ev[:6]]
        build = lambda cols: build_event_graphs(*cols, ep)                  # noqa: E731
        verify = lambda g: _same(g, host)                                   # noqa: E731

    def call(S):
        g = build([S(t) for t in d])                                        # gnn_event_graphs_sizes / _fill
        verify(g)
        b = g.batch
        return [b.X, b.src, b.dst, b.y, g.event_index, g.hit_index, g.layer]
    sweep(call)


@pytest.mark.parametrize("layout", ["flat", "padded"])
@pytest.mark.parametrize("source", ["fixture", "synthetic"])
def test_muon_graphs(hip, source, layout):
    from gnn_fpga_amd import build_muon_graphs, synth
    from test_gpu_muon_graph import _host, assert_same
    from test_muon_graph_host import assert_matches_case, load_case
    if source == "fixture":
        case = load_case(_smallest("muon_graph"))
        mu, pu, vpt, veta, start, muon_only = case[:6]
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
        vpt, veta = dd["vp_pt"][:43], dd["vp_eta"][:43]
        case = None
    want = build_muon_graphs(mu, pu, vpt, veta, entry_start=start, muon_only=muon_only, layout=layout)
    mud, pud = ({k: _dev(v) for k, v in t.items()} for t in (mu, pu))
    vpd = [_dev(vpt), _dev(veta)]

    def call(S):
        args = ({k: S(v) for k, v in mud.items()}, {k: S(v) for k, v in pud.items()}, S(vpd[0]), S(vpd[1]))
        res = build_muon_graphs(*args, entry_start=start, muon_only=muon_only, layout=layout)   # gnn_muon_graph_*
        got = _host(res)
        assert_same(got, want)                                              # the specification, bit for bit
        if case is not None and layout == "flat":
            assert_matches_case(got, case)                                  # and the reference's graphs
        b = res.batch
        return [b.X, b.src, b.dst, b.y, res.entry, res.pt, res.eta, res.written, res.vp_missing, res.hit_source,
                res.hit_row, res.present, res.n_hits, res.n_segments]
    sweep(call)


# ---- the two product paths that make such views -------------------------------------------------------------------
STORE_HITS = (40, 41, 42, 43, 44, 45)       # windows of two graphs start at hit 0, 40, 81, 123, 166: 0, 0, 1, 3, 2 mod 4
WINDOW = 2
INFERENCE = {"per_module": dict(use_plan=False, use_events=False), "one_launch": dict(use_plan=True, use_events=True),
             "fused_plan": dict(use_plan=True, use_events=False)}
TRAINING = {"events": dict(use_events=True, level_order_training=False),
            "pass": dict(use_events=False, level_order_training=False),
            "twin": dict(use_events=False, level_order_training=True)}


@functools.lru_cache(maxsize=None)
def _store_graphs():
    from gnn_fpga_amd import synth
    graphs = []
    for i, n in enumerate(STORE_HITS):
        g = synth.layered_graph(n, 3 * n + i, 3, n_layers=4, seed=400 + i)
        graphs.append(synth.HitGraph(g.X, g.src, g.dst, (np.arange(g.src.shape[0]) % 3 == 0).astype(np.float32)))
    return graphs


def _step(model, batch, settings):
    for k, v in settings.items():
        setattr(model, k, v)
    model.train()
    model.zero_grad(set_to_none=True)
    e = model(batch)
    (e * torch.linspace(0.5, 1.5, e.numel(), device=e.device).view_as(e)).sum().backward()
    return [e.detach().clone()] + [p.grad.clone() for p in model.parameters()], model._route.kind


def _infer(model, batch, settings):
    for k, v in settings.items():
        setattr(model, k, v)
    model.eval()
    with torch.no_grad():
        return model(batch).clone(), model._route.kind


def test_store_windows(hip, monkeypatch):
    """Every window of a device GraphStore of ragged F = 3 graphs - X a view 12 * hit_ptr[j] bytes into the store's -
    through the three inference routes and one training step per training route: the bits of the same window
    rebuilt from fresh tensors.  (call_route.TWIN_MIN_HITS is a speed threshold: lowered here so that windows of 80
    hits train on their level-ordered twin, as the recorder's 2700-hit training case does.)"""
    from gnn_fpga_amd import HitGraphBatch, call_route
    monkeypatch.setattr(call_route, "TWIN_MIN_HITS", 0)
    from gnn_fpga_amd.batcher import GraphStore
    from gnn_fpga_amd.model import SegmentClassifier
    graphs = _store_graphs()
    store = GraphStore(graphs, "cuda")
    torch.manual_seed(23)
    proto = SegmentClassifier(input_dim=3, hidden_dim=8, n_iters=2).cuda()
    seen, routes = set(), set()
    for j in range(len(graphs) - WINDOW + 1):
        make = {"window": lambda: store.batch(j, WINDOW, layout="flat")[0],
                "fresh": lambda: HitGraphBatch.from_graphs(graphs[j:j + WINDOW]).cuda()}
        w = make["window"]()
        assert w.X.data_ptr() == store.X.data_ptr() + 12 * int(store.hit_ptr[j])
        seen.add(w.X.data_ptr() % 16)
        f = make["fresh"]()
        S = Shift(MODES[4 + j % 4])         # the window's runs: the binding's own outputs at mixed offsets as well
        assert f.X.data_ptr() % 16 == 0 and torch.equal(w.X, f.X) and torch.equal(w.src, f.src)
        for name, settings in INFERENCE.items():
            a, ra = _infer(copy.deepcopy(proto), make["fresh"](), settings)
            with shifted_alloc(S):
                b, rb = _infer(copy.deepcopy(proto), make["window"](), settings)
            assert ra == rb == {"per_module": "per_module", "one_launch": "events", "fused_plan": "plan"}[name]
            routes.add(ra)
            _assert_same([a], [b], "window %d, inference %s (%s)" % (j, name, ra))
        for name, settings in TRAINING.items():
            a, ra = _step(copy.deepcopy(proto), make["fresh"](), settings)
            with shifted_alloc(S):
                b, rb = _step(copy.deepcopy(proto), make["window"](), settings)
            assert ra == rb == name, (name, ra, rb)
            routes.add(ra)
            _assert_same(a, b, "window %d, training %s (%s)" % (j, name, ra))
        assert S.allocated > 0 and S.guards_intact() == []
    assert seen == {0, 4, 8, 12}, seen                      # the windows' X cover all four residues
    assert routes == {"per_module", "events", "plan", "pass", "twin"}, routes


FLAT_SHAPES = [(3, 8), (11, 16), (3, 32), (3, 64)]
_PLAIN = {}


def _flat_routes(D):
    routes = {k: dict(MODEL_ROUTES[k], mlp_bf16=False) for k in ("per_module", "plan", "events")}
    if D >= 32:
        routes["plan_bf16"] = dict(MODEL_ROUTES["plan"], mlp_bf16=True)
    return routes


def _flat_run(F, D, k):
    """Inference on every route, one autograd step + Adam and one GradBucket.step + Adam of the (F, D) model; `k` None:
    its parameters where torch put them (and a GradBucket as the package makes it), else shift_params(model, k)."""
    from gnn_fpga_amd.loss import BCELoss
    from gnn_fpga_amd.model import SegmentClassifier
    from gnn_fpga_amd.shard import GradBucket
    torch.manual_seed(31 * D + F)
    model = SegmentClassifier(input_dim=F, hidden_dim=D, n_iters=2).cuda()
    if k is None:
        bucket = GradBucket(model.parameters())
    else:
        _, bucket = shift_params(model, k, grads=True)
        # Win .. b2 hold a multiple of 4 floats plus b2's one: they start k floats past the grid, W3 .. b4 k + 1.
        # So W3, b3, W4, b4 are off the grid at k = 0, 1, 2; at k = 3 they are ON it (225 + 3 = 4 * 57) and the
        # first six, b1 among them - which the wide kernels also read 16 bytes at a time -, are 12 bytes off it
        res = [p.data_ptr() % 16 for p in model.parameters()]
        assert res == [4 * k % 16] * 6 + [4 * (k + 1) % 16] * 4, (k, res)
        assert all(res[6:]) if k < 3 else (not any(res[6:]) and all(res[:6]))
        assert [p.grad.data_ptr() % 16 for p in model.parameters()] == res
    big, small = _cached_host_batch(F), _cached_host_batch(F, False)
    outs, routes = [], []
    for name, settings in _flat_routes(D).items():
        for hb in (big, small):
            e, r = _infer(model, shift_batch(hb, 0), settings)
            outs.append(e)
            routes.append((name, r))
    model.mlp_bf16 = False
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    b = shift_batch(big, 0)
    # the autograd step: the gradients are accumulated into the bucket's zeroed views
    model.use_events, model.level_order_training = False, False
    model.train()
    bucket.zero()
    e = model(b)
    loss = BCELoss(reduction="sum")(e, b.y)
    loss.backward()
    outs += [e.detach().clone(), loss.detach().clone()] + [p.grad.clone() for p in model.parameters()]
    opt.step()
    outs += [p.detach().clone() for p in model.parameters()]
    # GradBucket.step: forward, loss and backward without an autograd graph, adding into the bucket's views
    mean = bucket.step(model, b, b.y)
    outs += [mean.clone()] + [p.grad.clone() for p in model.parameters()]
    opt.step()
    outs += [p.detach().clone() for p in model.parameters()]
    torch.cuda.synchronize()
    return outs, routes


@pytest.mark.parametrize("k", [0, 1, 2, 3])
@pytest.mark.parametrize("F,D", FLAT_SHAPES, ids=["%dx%d" % s for s in FLAT_SHAPES])
def test_flat_parameters(hip, F, D, k):
    """A model whose parameters (and gradients) live packed in one flat buffer after k leading floats: scores on
    every inference route, the loss, every gradient and the parameters after an Adam step - by autograd and by
    GradBucket.step - have the bits of the same model with its parameters where torch put them.  `_flat_run` first
    proves from data_ptr() which parameters are off the grid: W3, b3, W4, b4 at k = 0, 1, 2 (they start k + 1 floats
    past it) and Win .. b2 at k = 3, where 225 + 3 floats put W3 .. b4 back ON the grid - no lead has all ten off it."""
    if (F, D) not in _PLAIN:
        _PLAIN[(F, D)] = _flat_run(F, D, None)              # once per shape, left unchanged
    want, want_routes = _PLAIN[(F, D)]
    S = Shift(k)
    with shifted_alloc(S):                  # kept layers, gradients' scratch, workspaces of _lib: k floats off too
        got, routes = _flat_run(F, D, k)
    assert S.allocated > 0 and S.guards_intact() == []
    assert routes == want_routes
    _assert_same(want, got, "%dx%d, parameters packed after %d floats, against the plain model" % (F, D, k))


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_flat_parameters_node_classifier(hip, k):
    from gnn_fpga_amd.model import NodeClassifier

    def run(k):
        torch.manual_seed(77)
        model = NodeClassifier(input_dim=3, hidden_dim=8, n_iters=2).cuda()
        if k is not None:
            shift_params(model, k)
        b = shift_batch(_cached_host_batch(3), 0)
        model.eval()
        with torch.no_grad():
            outs = [model(b).clone()]
        model.train()
        y = model(b)
        (y * torch.linspace(0.5, 1.5, y.numel(), device=y.device)).sum().backward()
        return outs + [y.detach().clone()] + [p.grad.clone() for p in model.parameters()]
    if "nodeclf" not in _PLAIN:
        _PLAIN["nodeclf"] = run(None)
    _assert_same(_PLAIN["nodeclf"], run(k), "NodeClassifier, parameters packed after %d floats" % k)
