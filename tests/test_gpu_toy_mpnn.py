"""GPU checks of the toy MPNN notebook's classifiers (gnn_fpga_amd/toy_mpnn.py, csrc/iter_events.hip) against fp64.

Bounds (tests/toy_mpnn_fp64.py): scores and every stored pass's e_t / H_t within 1e-5 absolute of the fp64 values -
the project's score bound -; the loss and EVERY gradient tensor separately within max(4 x the reference's own fp32
error, 5e-6) of the fp64 value, relative to that tensor's largest fp64 entry (with default init the gradients of the
early iterations at T = 10 are 1e-7 of the largest gradient: a global bound would see nothing of them).  For a
fixture the reference's own error is its ref_err_*; for synthetic inputs it is the distance of the restatement run in
fp32 on the CPU, the largest over eight segment orders (`reference_error`).  Every figure is printed before it is asserted (run with -s to see them)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import toy_mpnn_fp64 as ref
from gnn_fpga_amd import HitGraphBatch, ToySegmentClassifier, build_toy_mpnn_graphs, synth
from gnn_fpga_amd import sort_toy_tracks
from gnn_fpga_amd.call_route import EVENTS_MAX_GRAPHS
from toy_mpnn_cases import (check_abs, check_graphs, check_rel, model_of, random_graph, random_params,  # noqa: F401
                            reference_error, train_step)

pytestmark = pytest.mark.gpu
_FIX = {}


def fixture(case):
    if case not in _FIX:
        _FIX[case] = ref.Fixture(case)
    return _FIX[case]


def index_batch(X, src, dst, y, hit_ptr, seg_ptr, dense_shape=None):
    return HitGraphBatch(np.asarray(X, np.float32).reshape(-1, X.shape[-1]), src, dst, y=np.asarray(y).reshape(-1),
                         hit_ptr=hit_ptr, seg_ptr=seg_ptr, dense_shape=dense_shape).to("cuda")


def fixture_inputs(fx, form):
    if form == "dense":
        return [torch.from_numpy(fx[k]).cuda() for k in ("X", "Ri", "Ro")]
    return index_batch(fx["X"], fx["src"], fx["dst"], fx["y"], np.arange(fx.B + 1) * fx.N, np.arange(fx.B + 1) * fx.E,
                       (fx.B, fx.N, fx.E))


# ---- the reference's fixtures: both routes, both input forms -----------------------------------------------------------
# (the dense matrices are stored for the padded case only)
FIXTURE_RUNS = [(c, r, f) for c in ref.CASES for r in ("iter_events", "per_module")
                for f in (("index", "dense") if "ragged" in c else ("index",))]


@pytest.mark.parametrize("case,route,form", FIXTURE_RUNS)
def test_fixture(hip, case, route, form):
    fx = fixture(case)
    m = model_of(fx.params, fx.F, fx.D, fx.T, fx.shared, events=route == "iter_events")
    inp = fixture_inputs(fx, form)
    y = torch.from_numpy(fx["y"]).cuda()
    C = fx.F + fx.D
    bad = []
    with torch.no_grad():
        e, et, Ht = m.eval()(inp, trace=True)
        assert m._route.kind == route
        plain = m(inp)
    assert tuple(e.shape) == (fx.B, fx.E) and tuple(et.shape) == (fx.T + 1, fx.B * fx.E)
    assert tuple(Ht.shape) == (fx.T + 1, fx.B * fx.N, C)
    bad += check_abs("scores", e.cpu().numpy(), fx["e64_%d" % fx.T])
    for t in range(fx.T + 1):
        bad += check_abs("e_%d" % t, et[t].cpu().numpy(), fx["e64_%d" % t].reshape(-1))
    for t in fx.h_passes():
        bad += check_abs("H_%d" % t, Ht[t].cpu().numpy(), fx["H64_%d" % t].reshape(-1, C))
    out, loss, grads = train_step(m, inp, y)
    assert m._route.kind == route
    assert torch.equal(out, plain.reshape(-1)), "inference scores differ from the training forward's"
    assert torch.equal(out, e.reshape(-1)), "traced scores differ from the training forward's"
    bad += check_rel("loss", loss, float(fx["loss64"]), float(fx["ref_err_loss"]))
    assert list(grads) == fx.keys
    for k in fx.keys:
        bad += check_rel("grad " + k, grads[k], fx.grad64[k], fx.ref_err_grad[k])
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", ["a_unshared_f2_d32_t10_b4", "f_unshared_f11_d8_t2_ragged", "g_shared_f2_d32_t10_b4"])
def test_two_runs_give_the_same_bits(hip, case):
    fx = fixture(case)
    m = model_of(fx.params, fx.F, fx.D, fx.T, fx.shared)
    y = torch.from_numpy(fx["y"]).cuda()
    runs = [train_step(m, fixture_inputs(fx, "index"), y) for _ in range(2)]
    assert m._route.kind == "iter_events"
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    for k in fx.keys:
        assert np.array_equal(runs[0][2][k].view(np.uint32), runs[1][2][k].view(np.uint32)), k


def test_adam_step_changes_every_tensor(hip):
    fx = fixture("a_unshared_f2_d32_t10_b4")
    m = model_of(fx.params, fx.F, fx.D, fx.T, fx.shared)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    opt = torch.optim.Adam(m.parameters())
    out = m.train()(fixture_inputs(fx, "index"))
    nn.BCELoss()(out, torch.from_numpy(fx["y"]).cuda()).backward()
    opt.step()
    assert m._route.kind == "iter_events" and len(before) == 86
    same = [k for k, v in m.state_dict().items() if torch.equal(v, before[k])]
    assert not same, "unchanged after an Adam step: %s" % same
    with torch.no_grad():           # the stepped parameters are what the next call reads
        again = m.eval()(fixture_inputs(fx, "index"))
    assert not torch.equal(again, out.detach())


# ---- size edges, against the restatement -------------------------------------------------------------------------------
def _nt_forward(D):
    return 64 * (16 if D >= 32 else 8 if D >= 8 else 4)         # csrc/iter_events.hip ItFwd::NT; the backward runs 256


@pytest.mark.parametrize("D", [8, 32])
def test_segment_count_edges(hip, D):
    """Graphs of 0, 1, NT - 1, NT and NT + 1 segments for both kernels' workgroup sizes, graphs of 1 and 2 hits, a hit
    with no segment: one batch, the one-launch route."""
    rng = np.random.default_rng(100 + D)
    nt = _nt_forward(D)
    counts = [0, 1, 255, 256, 257, nt - 1, nt, nt + 1]
    graphs = [random_graph(rng, 30, ns, 2) for ns in counts] + [random_graph(rng, 1, 0, 2), random_graph(rng, 2, 1, 2)]
    check_graphs(hip, graphs, 2, D, 2, "iter_events", "iter_events", seed=D)


@pytest.mark.parametrize("D", [8, 32])
def test_hit_count_edges(hip, D):
    """Graphs of 1, 2, 63, 64 and 65 hits.  At hidden_dim 32 the backward's LDS ends near 49 hits: training falls back."""
    rng = np.random.default_rng(200 + D)
    graphs = [random_graph(rng, nh, min(3 * nh, 150), 2) for nh in (1, 2, 63, 64, 65)]
    fits = hip.iter_events_supported(2, D, 65, 150, True)
    assert fits == (D == 8)
    check_graphs(hip, graphs, 2, D, 2, "iter_events", "iter_events" if fits else "per_module", seed=D + 1)


@pytest.mark.parametrize("D", [8, 32])
def test_one_graph(hip, D):
    rng = np.random.default_rng(300 + D)
    check_graphs(hip, [random_graph(rng, 25, 70, 2)], 2, D, 3, "iter_events", "iter_events", seed=D + 2)


@pytest.mark.parametrize("D", [8, 32])
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("T,route", [(16, "iter_events"), (17, "per_module")])
def test_iteration_limit(hip, T, route, shared, D):
    """All GNN_ITER_MAX slots of the by-value parameter table, and one iteration more than it holds."""
    assert hip.GNN_ITER_MAX == 16
    rng = np.random.default_rng(400 + T + D)
    check_graphs(hip, [random_graph(rng, 12, 30, 2) for _ in range(3)], 2, D, T, route, route, shared=shared, seed=T + D)


@pytest.mark.parametrize("D", [8, 32])
def test_one_hit_over_the_limit(hip, D):
    """The largest graph the one-launch backward takes at (2, D) with 40 segments - the kernel's LDS carving against
    gnn_iter_events_supported's arithmetic, at the last size that passes it - and one hit more."""
    top = max(h for h in range(1, 400) if hip.iter_events_supported(2, D, h, 40, True))
    assert not hip.iter_events_supported(2, D, top + 1, 40, True)
    print("  hidden_dim %d: the backward takes %d hits with 40 segments" % (D, top))
    rng = np.random.default_rng(500 + D)
    check_graphs(hip, [random_graph(rng, top, 40, 2), random_graph(rng, 9, 20, 2)], 2, D, 1, "iter_events", "iter_events",
                 seed=D)
    more = [random_graph(rng, top + 1, 40, 2), random_graph(rng, 9, 20, 2)]
    fwd = "iter_events" if hip.iter_events_supported(2, D, top + 1, 40, False) else "per_module"
    check_graphs(hip, more, 2, D, 1, fwd, "per_module", seed=D)


@pytest.mark.parametrize("D", [8, 32])
def test_more_graphs_than_the_one_launch_route_takes(hip, D):
    rng = np.random.default_rng(600 + D)
    graphs = [random_graph(rng, 3, 2, 2, lone=False) for _ in range(EVENTS_MAX_GRAPHS + 1)]
    check_graphs(hip, graphs, 2, D, 1, "per_module", "per_module", seed=D)


# ---- the notebook's data cells -----------------------------------------------------------------------------------------
def test_build_toy_mpnn_graphs_equals_its_specification(hip):
    tracks = synth.toy_tracks(5, 4, seed=3)
    hx, hy = sort_toy_tracks(torch.from_numpy(tracks).cuda())
    g = build_toy_mpnn_graphs(hx, hy)
    X, src, dst, y = synth.toy_mpnn_graphs_from_hits(hx.cpu().numpy(), hy.cpu().numpy())
    b = g.batch
    assert (b.n_graphs, b.n_hits, b.n_segments) == (5, 200, 720) and b.event_layout() is not None
    assert (b.event_layout().max_hits, b.event_layout().max_segments) == (40, 144)
    assert np.array_equal(b.X.cpu().numpy().view(np.uint32), X.reshape(-1, 2).view(np.uint32))
    off = (np.arange(5) * 40)[:, None]
    assert np.array_equal(b.src.cpu().numpy(), (src[None] + off).reshape(-1))
    assert np.array_equal(b.dst.cpu().numpy(), (dst[None] + off).reshape(-1))
    assert np.array_equal(g.y.cpu().numpy(), y.reshape(-1)) and g.y is b.y
    want = HitGraphBatch(X.reshape(-1, 2), b.src.cpu().numpy(), b.dst.cpu().numpy()).to("cuda")     # gnn_csr_build's lists
    for name in ("in_ptr", "in_eid", "in_nbr", "out_ptr", "out_eid", "out_nbr"):
        assert torch.equal(getattr(b, name), getattr(want, name)), name
    m = ToySegmentClassifier(2, 8, 2).cuda()
    with torch.no_grad():
        e = m(b)
    assert m._route.kind == "iter_events" and tuple(e.shape) == (720,)
