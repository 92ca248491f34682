"""GPU training and inference at detector scale against an fp64 reference (oracle/index_torch.py: index form,
torch autograd, float64 on the CPU).

Every other gradient test at detector size compares one HIP path with another that shares its machinery
(k_grad_fold's row chunks, the partial-row tables, the list walks of k_seg_bwd4 / k_seg_bwdW, kOuterCap chunks).
Here every route is checked against the truth on the graph families of fp64_graphs.py - hubs of degree 1 ... 4097
(the 4- and 16-lane list walks at and past their strides), a 70 000-segment hit (the torch plan builder), ragged
batches, padded segments, small events with hubs (the one-launch kernels) and the mu200 shape (3, 64, 6).

Training cases check scores at TOL, the loss at 1e-6 (relative for a summed loss) and all ten gradients with
golden_util.assert_grad_close at the unchanged GRAD_REL / GRAD_ABS, and assert that the route they are named for
ran (kernel names from _lib.profile):

  pass        caller's order, per-pass kernels       level_order_training = False    k_seg_bwd4 / k_seg_bwdW, no k_edge_tw
  twin        level-ordered twin + fused forward     level_order_training = True     k_edge_tw (D <= 8, (11, 16))
  twin_pp     twin with the per-pass training fwd    + GNN_NO_FUSED_TRAIN=1          a twin, no k_edge_tw
  events      one-launch event kernels               use_events = True, D <= 16      k_event_bwd

GNN_TEST_RECORD=<file> receives every comparison's worst error and max|reference|.
"""
import numpy as np
import pytest
import torch

import fp64_graphs
from golden_util import assert_grad_close
from gnn_fpga_amd import HitGraphBatch
from oracle import index_c, index_torch
from oracle.dense_torch import KEYS

pytestmark = pytest.mark.gpu

TOL = 1e-5          # edge scores (north_star), as in test_gpu_parity
LOSS_TOL = 1e-6
FP32_PRECONDITION = 2.5e-6     # exp-product cases: the fp32 CPU oracle itself must lie this close to fp64


def _record(what, err, scale):
    import os
    rec = os.environ.get("GNN_TEST_RECORD")
    if rec:
        with open(rec, "a") as f:
            f.write("%s\t%.3e\t%.3e\t%.3e\n" % (what, err, scale, err / scale if scale else 0.0))


def _bounds(case, route):
    """(score bound, gradient rel bound) of one training (case, route): FP32_LIMIT's where listed, else TOL / GRAD_REL."""
    from golden_util import GRAD_REL
    tol, rel, _ = FP32_LIMIT.get((tuple(case[:4]), route), (None, None, None))
    return (tol or TOL), (rel or GRAD_REL)


def _assert_scores(got, ref, what, tol=TOL):
    got = np.asarray(got.detach().cpu().numpy() if hasattr(got, "detach") else got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    _record(what, err, float(np.abs(ref).max()) if ref.size else 0.0)
    assert err < tol, (what, err)
    return err


def _batch(fam):
    return HitGraphBatch(fam.X, fam.src, fam.dst, y=fam.y, hit_ptr=fam.hit_ptr, seg_ptr=fam.seg_ptr).cuda()


def _masks(F, D, seed):
    g = torch.Generator().manual_seed(seed)
    C = F + D
    return dict(masks_e=[(torch.rand(D, 2 * C, generator=g) < 0.7).float(), (torch.rand(1, D, generator=g) < 0.8).float()],
                masks_n=[(torch.rand(D, 3 * C, generator=g) < 0.7).float(), (torch.rand(D, D, generator=g) < 0.8).float()])


def _model(F, D, T, seed, masked=False):
    """A CPU SegmentClassifier (default init from `seed`), its fp64 parameters and masks for the oracle."""
    from gnn_fpga_amd.model import SegmentClassifier
    torch.manual_seed(seed)
    m = SegmentClassifier(input_dim=F, hidden_dim=D, n_iters=T, **(_masks(F, D, seed) if masked else {}))
    params = {k: v.detach().double().clone() for k, v in m.state_dict().items()}
    masks = None
    if masked:
        masks = {k + ".weight": getattr(m, k.split(".")[0]).network[int(k.split(".")[-1])].mask.double()
                 for k in ("edge_network.network.0", "edge_network.network.2", "node_network.network.0",
                           "node_network.network.2")}
    return m, params, masks


def _loss_fn(kind, dev=True):
    from gnn_fpga_amd.loss import BCELoss
    if kind == "torch":
        return torch.nn.BCELoss()
    if not dev:
        return torch.nn.BCELoss(reduction="mean" if kind == "fused_mean" else "sum")
    return BCELoss(reduction="mean" if kind == "fused_mean" else "sum")


# ---- fp64 references, shared across routes (module scope) ------------------------------------------------------
class _Refs:
    def __init__(self):
        self.train = {}
        self.fwd = {}

    def training(self, case):
        key = case[:7]
        if key not in self.train:
            fam_name, F, D, T, loss, masked, seed = key
            fam = fp64_graphs.family(fam_name, F)
            _, params, masks = _model(F, D, T, seed, masked)
            p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
            e = index_torch.segment_classifier(fam.X, fam.src, fam.dst, p, T, masks)
            lo = _loss_fn(loss, dev=False)(e, torch.from_numpy(fam.y).double())
            lo.backward()
            grads = {k: (p[k].grad.numpy() if p[k].grad is not None else np.zeros(p[k].shape)) for k in KEYS}
            self.train[key] = (e.detach().numpy(), lo.item(), grads)
        return self.train[key]

    def forward(self, fam_name, F, D, T, seed, params=None, tag=""):
        key = (fam_name, F, D, T, seed, tag)
        if key not in self.fwd:
            fam = fp64_graphs.family(fam_name, F)
            if params is None:
                params = _model(F, D, T, seed)[1]
            p = {k: v.numpy() for k, v in params.items()}
            self.fwd[key] = index_c.segment_classifier(fam.X, fam.src, fam.dst, p, T, f64=True).astype(np.float64)
        return self.fwd[key]


@pytest.fixture(scope="module")
def refs():
    return _Refs()


# ---- training -----------------------------------------------------------------------------------------------------
# (family, F, D, T, loss, masked, weight seed, routes, what it is there for)
ALL = ("pass", "twin", "twin_pp")
WIDE = ("pass", "twin_pp")         # no fused training forward: choose_route declines D > 16 and D = 16 with F <= 4
TRAIN_CASES = [
    ("c3x4", 3, 8, 3, "torch", False, 1, ALL, "the headline shape; 1 % padded segments scattered through the order"),
    ("c3x4", 2, 4, 1, "fused_mean", False, 2, ALL, "narrowest shape, one iteration"),
    ("c3x4", 11, 16, 3, "fused_sum", False, 3, ALL, "F = 11, D = 16: the widest fused training forward, summed loss"),
    ("c3x4", 3, 32, 1, "torch", False, 4, WIDE, "16 lanes per hit (k_seg_bwdW) at c3 x 4"),
    ("c3x4", 2, 16, 0, "fused_mean", False, 5, WIDE, "T = 0: input network + one edge pass"),
    ("hubs", 2, 8, 3, "fused_mean", False, 6, ALL, "hub lists of degree 1 ... 4097 on the 4-lane walk"),
    ("hubs", 3, 4, 3, "fused_sum", False, 7, ALL, "D = 4 on the hub lists"),
    ("hubs", 11, 4, 0, "torch", False, 8, ALL, "F = 11, T = 0 on the hubs"),
    ("hubs", 11, 8, 3, "fused_mean", False, 9, ALL, "F = 11, D = 8 on the hub lists"),
    ("hubs", 3, 16, 1, "torch", False, 10, WIDE, "D = 16 on the hub lists"),
    ("hubs", 2, 32, 3, "fused_mean", False, 11, WIDE, "k_seg_bwdW walks the hub lists (F = 2)"),
    ("hubs", 3, 64, 3, "fused_sum", False, 12, WIDE, "k_seg_bwdW at D = 64 on the hub lists"),
    ("hubs", 3, 8, 3, "torch", True, 13, ("twin",), "masked model (effective weights) on the twin"),
    ("c3", 3, 64, 3, "torch", False, 14, ("pass",), "D = 64 on one c3 graph (below the twin's 20 000 hits)"),
    ("c3", 2, 32, 1, "fused_mean", False, 15, ("pass",), "D = 32 on one c3 graph"),
    ("superhub", 3, 8, 2, "torch", False, 16, ALL, "a 70 000-segment hit: the torch plan builder behind the twin"),
    ("ragged", 3, 8, 3, "fused_mean", False, 17, ALL, "1-hit, 2-hit, empty and all-padded graphs + 200 small ones"),
    ("ragged", 11, 16, 2, "fused_sum", False, 18, ALL, "the ragged batch at F = 11, D = 16 (fused forward too)"),
    ("events", 11, 8, 3, "torch", False, 19, ("events", "pass"), "300 events with hubs of up to 1200 segments"),
    ("events", 11, 16, 2, "fused_mean", False, 20, ("events", "pass"), "one-launch kernels at D = 16"),
    ("events", 11, 4, 1, "fused_sum", False, 21, ("events",), "one-launch kernels at D = 4"),
    ("mu200", 3, 64, 6, "fused_mean", False, 22, WIDE, "the mu200 notebook's (3, 64, 6) at 500 k segments"),
]
# (case, route) pairs at the limit of fp32, with their own bounds: {((family, F, D, T), route): (score bound or None,
# gradient rel bound or None, GPU error measured on MI355X with GNN_TEST_RECORD)}.  Where the scores' or the gradients'
# largest entry is small against the terms it is summed from (the hubs' saturated tanh, the events' complete bipartite
# layers), the fp32 result depends on the summation order, and the caller's order is just one order.  Each bound is at
# most 2.5 x the measured GPU error and at most 2.5 x the worst error of the fp32 CPU oracle (index_torch in float32)
# over five orders of the same segments: tests/test_fp32_limit_host.py recomputes the latter and checks both.
# Every pair not listed keeps TOL and golden_util.GRAD_REL.
FP32_LIMIT = {
    (("events", 11, 8, 3), "events"): (None, 8.4e-5, (1.32e-7, 3.53e-5)),     # fp32 oracle over orders: 7.4e-5
    (("events", 11, 8, 3), "pass"): (None, 8.4e-5, (1.32e-7, 3.51e-5)),
    (("events", 11, 16, 2), "events"): (None, 4.9e-5, (1.14e-7, 2.05e-5)),    # 3.8e-5
    (("events", 11, 16, 2), "pass"): (None, 4.9e-5, (1.14e-7, 2.05e-5)),
    (("hubs", 2, 8, 3), "pass"): (None, 1.0e-4, (1.96e-7, 4.20e-5)),          # 8.1e-5
    (("hubs", 2, 8, 3), "twin_pp"): (None, 2.0e-4, (3.63e-7, 1.06e-4)),
    (("hubs", 2, 32, 3), "pass"): (None, 1.8e-3, (5.52e-7, 7.89e-4)),         # 1.09e-3
    (("hubs", 2, 32, 3), "twin_pp"): (None, 2.7e-3, (1.77e-6, 1.39e-3)),
    (("hubs", 3, 64, 3), "pass"): (None, 2.4e-4, (1.62e-7, 1.00e-4)),         # 1.55e-4
    (("hubs", 3, 64, 3), "twin_pp"): (None, 1.8e-4, (1.47e-7, 7.64e-5)),
    (("hubs", 11, 8, 3), "pass"): (None, 2.0e-4, (1.06e-7, 8.45e-5)),         # 2.5e-4
    (("hubs", 11, 8, 3), "twin_pp"): (None, 2.9e-4, (1.27e-7, 1.21e-4)),
}
# The same for the sub-module checks: {(D, order): {quantity: (rel bound, measured GPU error / max|fp64|)}}.  The
# 4097-hub's sums of random rows make grad e (through tanh' of the node network's hidden layer) order-dependent.
SUBMODULE_FP32_LIMIT = {
    (8, "twin"): {"grad e": (7.5e-6, 6.43e-6)},       # fp32 oracle over orders: 3.05e-6
}
TRAIN_PARAMS = [pytest.param(c, r, id="%s-F%d-D%d-T%d-%s%s-%s" % (c[0], c[1], c[2], c[3], c[4], "-masked" if c[5] else "", r))
                for c in TRAIN_CASES for r in c[7]]


@pytest.mark.parametrize("case,route", TRAIN_PARAMS)
def test_training_step_against_fp64(hip, refs, case, route, monkeypatch):
    """One training step (forward, loss, backward) of the case's family and shape on `route`, against autograd through
    oracle.index_torch in fp64: scores at TOL, loss at 1e-6, all ten gradients at golden_util's bound.  The case's
    last field says which kernel / degree / shape it is there for; the route is asserted from the kernel names."""
    fam_name, F, D, T, loss_kind, masked, seed, _, why = case
    fam = fp64_graphs.family(fam_name, F)
    m, _, _ = _model(F, D, T, seed, masked)
    m = m.cuda().train()
    m.use_events = route == "events"
    m.level_order_training = route in ("twin", "twin_pp")
    if route == "twin_pp":
        monkeypatch.setenv("GNN_NO_FUSED_TRAIN", "1")
    b = _batch(fam)
    y = b.y.cuda()
    m.zero_grad()
    with hip.profile(2048) as prof:
        out = m(b)
        loss = _loss_fn(loss_kind)(out, y)
        loss.backward()
        torch.cuda.synchronize()
    names = {k for k, _ in prof.records}
    # the route ran
    twin = getattr(b, "_twin", None)
    if route == "events":
        assert "k_event_bwd" in names, (why, sorted(names))
    else:
        assert "k_event_bwd" not in names and "k_event" not in names, (why, sorted(names))
        if T > 0:
            assert ("k_seg_bwdW" if D >= 32 else "k_seg_bwd4") in names, (why, sorted(names))
    if route == "twin":
        assert twin is not None and twin is not b, why
        assert "k_edge_tw" in names, (why, sorted(names))
    else:
        assert "k_edge_tw" not in names, (why, sorted(names))
    if route == "twin_pp":
        assert twin is not None and twin is not b, why
    if route == "pass":
        assert twin is None, why
    if fam_name == "superhub" and route != "pass":
        from gnn_fpga_amd.plan_device import DeviceSellPlan
        assert isinstance(b.plan, DeviceSellPlan)          # >= 65536 segments at one hit: the torch builder
    # against fp64
    e_ref, l_ref, g_ref = refs.training(case)
    tag = "train %s F%d D%d T%d %s%s %s" % (fam_name, F, D, T, loss_kind, " masked" if masked else "", route)
    tol, rel = _bounds(case, route)
    _assert_scores(out, e_ref, tag + " scores", tol=tol)
    err = abs(loss.item() - l_ref)
    _record(tag + " loss", err, abs(l_ref))
    assert err < LOSS_TOL * max(1.0, abs(l_ref)), (tag, loss.item(), l_ref)
    for k, p in m.named_parameters():
        assert_grad_close(p.grad, g_ref[k], tag + " " + k, rel=rel)


# ---- the sub-modules at hub degrees -------------------------------------------------------------------------------
def submodule_inputs(fam, C, D):
    """Seeded fp64 inputs of the sub-module checks: H [N, C], e [E] and the weights of a linear loss on e and H'."""
    g = torch.Generator().manual_seed(D)
    H0 = torch.rand(fam.X.shape[0], C, generator=g, dtype=torch.float64) * 2 - 1
    e0 = torch.rand(fam.src.shape[0], generator=g, dtype=torch.float64)
    wE = torch.rand(fam.src.shape[0], generator=g, dtype=torch.float64)
    wN = torch.rand(fam.X.shape[0], D, generator=g, dtype=torch.float64)
    return H0, e0, wE, wN


@pytest.mark.parametrize("order", ["caller", "twin"])
@pytest.mark.parametrize("D", [8, 32])
def test_submodules_at_hub_degrees(hip, D, order):
    """EdgeNetwork / NodeNetwork called directly with gradients (gnn_edge_bwd: k_edge_bwd, gnn_node_bwd: k_node_bwd) on
    the hubs graph against oracle.index_torch's edge_network / node_network in fp64: values at TOL, the gradients of
    H, e and the four weights of each at golden_util's bound.  order = "twin": the same inputs on the level-ordered
    twin (plan hit ids, dummy rows, segments sorted by end hit), results mapped back - a twin-only error in a
    full-model case shows here as one pass."""
    F = 3
    fam = fp64_graphs.hubs(F)
    m, params, _ = _model(F, D, 1, 30 + D)
    m = m.cuda()
    b = _batch(fam)
    C = F + D
    H0, e0, wE, wN = submodule_inputs(fam, C, D)
    dev = torch.device("cuda:0")
    hits = torch.arange(fam.X.shape[0], device=dev)             # caller's hit i is row hits[i] of the batch run
    segs = torch.arange(fam.src.shape[0], device=dev)           # caller's segment j is entry segs[j]
    run = b
    if order == "twin":
        run = b.level_ordered(D)
        assert run is not b
        perm = b.plan.perm.to(torch.int64)
        new_ids = torch.nonzero(perm >= 0).reshape(-1)
        hits = torch.empty_like(hits)
        hits[perm[new_ids]] = new_ids
        segs = run.seg_rank
    n_run = run.n_hits

    def scatter_rows(A):                                        # caller's rows -> the batch run's rows (dummies 0)
        out = torch.zeros((n_run,) + tuple(A.shape[1:]), dtype=torch.float32, device=dev)
        out[hits] = A.float().to(dev)
        return out

    def scatter_segs(a):
        out = torch.empty(a.shape[0], dtype=torch.float32, device=dev)
        out[segs] = a.float().to(dev)
        return out

    Hg = scatter_rows(H0).requires_grad_(True)
    eg = scatter_segs(e0).requires_grad_(True)
    with hip.profile(256) as prof:
        e_gpu = m.edge_network(Hg, run)
        n_gpu = m.node_network(Hg, eg, run)
        ((e_gpu * scatter_segs(wE)).sum() + (n_gpu * scatter_rows(wN)).sum()).backward()
        torch.cuda.synchronize()
    names = {k for k, _ in prof.records}
    assert "k_edge_bwd" in names and "k_node_bwd" in names, sorted(names)
    # fp64
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    Hr = H0.clone().requires_grad_(True)
    er = e0.clone().requires_grad_(True)
    e_ref = index_torch.edge_network(Hr, fam.src, fam.dst, p)
    n_ref = index_torch.node_network(Hr, er, fam.src, fam.dst, p)
    ((e_ref * wE).sum() + (n_ref * wN).sum()).backward()
    tag = "submodule hubs D%d %s " % (D, order)
    _assert_scores(e_gpu[segs], e_ref.detach().numpy(), tag + "edge_network")
    _assert_scores(n_gpu[hits], n_ref.detach().numpy(), tag + "node_network")
    assert_grad_close(Hg.grad[hits], Hr.grad, tag + "grad H")
    lim = SUBMODULE_FP32_LIMIT.get((D, order), {})
    assert_grad_close(eg.grad[segs], er.grad, tag + "grad e", **({"rel": lim["grad e"][0]} if "grad e" in lim else {}))
    for prefix, mod in (("edge_network.", m.edge_network), ("node_network.", m.node_network)):
        for k, q in mod.named_parameters():
            assert_grad_close(q.grad, p[prefix + k].grad, tag + prefix + k)


# ---- inference on the same graphs ---------------------------------------------------------------------------------
INFER = [("hubs", 3, 8, 3), ("hubs", 11, 16, 2), ("hubs", 3, 32, 2), ("hubs", 3, 64, 2),
         ("superhub", 3, 8, 2), ("superhub", 3, 32, 2), ("superhub", 3, 64, 1),
         ("c3x4", 3, 8, 3), ("c3x4", 2, 4, 2), ("c3x4", 3, 32, 2), ("c3x4", 3, 64, 2)]


@pytest.mark.parametrize("route", ["modules", "plan"])
@pytest.mark.parametrize("fam_name,F,D,T", INFER)
def test_inference_against_fp64(hip, refs, fam_name, F, D, T, route):
    """Inference scores against index_c in fp64 at TOL: the first forward's per-module kernels (route "modules") and
    the fused plan (route "plan": k_iter / k_iter2 at D <= 16, k_iter_wx - the exact wide iteration, from 32 768
    padded hits on - at D = 32 / 64; on superhub the plan of the torch builder)."""
    fam = fp64_graphs.family(fam_name, F)
    m = _model(F, D, T, 40 + D + T)[0].cuda().eval()
    m.use_events = False
    m.use_plan = route == "plan"
    b = _batch(fam)
    with torch.no_grad(), hip.profile(512) as prof:
        e = m(b)
        torch.cuda.synchronize()
    names = {k for k, _ in prof.records}
    if route == "plan":
        assert b.plan is not None and b.plan.hidden_dim == D
        if D >= 32:
            assert "k_iter_wx" in names, sorted(names)
        if fam_name == "superhub":
            from gnn_fpga_amd.plan_device import DeviceSellPlan
            assert isinstance(b.plan, DeviceSellPlan)
    else:
        assert b.plan is None and not any(k.startswith("k_iter") for k in names), sorted(names)
        assert any(k.startswith("k_node") for k in names), sorted(names)
    ref = refs.forward(fam_name, F, D, T, 40 + D + T)
    _assert_scores(e, ref, "inference %s F%d D%d T%d %s" % (fam_name, F, D, T, route))


@pytest.mark.parametrize("D,T", [(8, 3), (16, 2), (4, 1)])
def test_event_inference_against_fp64(hip, refs, D, T):
    """The one-launch inference kernel (k_event) on the events family, hubs of up to 1200 segments included."""
    fam = fp64_graphs.events(11)
    m = _model(11, D, T, 50 + D)[0].cuda().eval()
    b = _batch(fam)
    with torch.no_grad(), hip.profile(64) as prof:
        e = m(b)
        torch.cuda.synchronize()
    assert "k_event" in {k for k, _ in prof.records}
    _assert_scores(e, refs.forward("events", 11, D, T, 50 + D), "inference events F11 D%d T%d k_event" % (D, T))


def test_tolerance_sees_a_dropped_hub_entry(hip, refs):
    """The bound can see a real error: the fp64 reference of the hubs graph with ONE segment removed from the
    1000-degree hub's in-list lies more than 10 x TOL from the GPU scores (every other segment compared), while the
    true reference lies within TOL.  A kernel that drops a list entry at that degree cannot pass (measured on the
    CPU: 5e-3 at default init, T = 2)."""
    F, D, T = 3, 8, 2
    fam = fp64_graphs.hubs(F)
    hub = fam.info["in_hub"][1000]
    j = int(np.flatnonzero(fam.dst == hub)[0])
    keep = np.ones(fam.src.shape[0], bool)
    keep[j] = False
    m, params, _ = _model(F, D, T, 60)
    m = m.cuda().eval()
    m.use_events = False
    b = _batch(fam)
    p = {k: v.numpy() for k, v in params.items()}
    ref = index_c.segment_classifier(fam.X, fam.src, fam.dst, p, T, f64=True).astype(np.float64)
    dropped = index_c.segment_classifier(fam.X, fam.src[keep], fam.dst[keep], p, T, f64=True).astype(np.float64)
    for use_plan in (False, True):
        m.use_plan = use_plan
        with torch.no_grad():
            e = m(b).cpu().numpy().astype(np.float64)
        _assert_scores(e, ref, "dropped-entry check: true reference (plan=%s)" % use_plan)
        miss = float(np.abs(e[keep] - dropped).max())
        _record("dropped-entry check: distance to the wrong reference (plan=%s)" % use_plan, miss, 1.0)
        assert miss > 10 * TOL, miss


# ---- the exp-product fast path near the edge of its range ---------------------------------------------------------
def _edge_case_weights(hip, b, F, D, T, seed, target):
    """Model weights with the edge network's first layer scaled (bisection on the GPU bound) so that
    _lib.exp_product_bound lies at `target` (+-1)."""
    m, params, _ = _model(F, D, T, seed)
    m = m.cuda().eval()
    W1 = m.edge_network.network[0].weight
    W1_0 = W1.detach().clone()
    plan = b.build_plan(D)

    def bound(s):
        with torch.no_grad():
            W1.copy_(W1_0 * s)
        return hip.exp_product_bound(m.effective_weights(), F, D, plan.x_absmax)

    lo, hi = 1.0, 1.0
    while bound(hi) < target:
        hi *= 2.0
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        if bound(mid) < target:
            lo = mid
        else:
            hi = mid
        if abs(bound(mid) - target) < 1.0:
            break
    bd = bound(mid)
    assert abs(bd - target) < 1.0, bd
    params = {k: v.detach().double().cpu() for k, v in m.state_dict().items()}
    return m, params, bd


def _with_extremes(fam):
    """Some hits at the extremes of the feature range (|X| = 1: x_absmax = 1 for every feature)."""
    X = fam.X.copy()
    X[::997] = np.where(np.arange(X.shape[1]) % 2 == 0, 1.0, -1.0)
    return fp64_graphs.Family(X, fam.src, fam.dst, fam.y, fam.hit_ptr, fam.seg_ptr, fam.info)


XP_CASES = [(f, D) for f in ("c3x4", "hubs") for D in (4, 8, 16, 32, 64)]


@pytest.mark.parametrize("side", ["fast path, bound ~ 52", "exact path, bound ~ 61"])
@pytest.mark.parametrize("fam_name,D", XP_CASES)
def test_exp_product_near_the_edge_of_its_range(hip, fam_name, D, side):
    """GNN_FLAG_EXP_PRODUCT (2^P' * 2^Q' in the fused kernels) with weights that put _lib.exp_product_bound at 52
    (inside its proven range, <= 60: the fast path must be taken) and at 61 (just outside: the exact path), on c3x4
    and hubs at every width (all fused widths honour the flag), against index_c in fp64 at TOL.  Precondition: the
    fp32 CPU oracle lies within 2.5e-6 of fp64 (large first-layer weights could make the network itself
    ill-conditioned in fp32; then the case says so instead of widening TOL)."""
    F, T = 3, 2
    fast = side.startswith("fast")
    fam = _with_extremes(fp64_graphs.family(fam_name, F))
    b = _batch(fam)
    for seed in (70 + D, 170 + D, 270 + D):       # the precondition picks the seed (CPU only), never the bound
        m, params, bd = _edge_case_weights(hip, b, F, D, T, seed, 52.0 if fast else 61.0)
        p = {k: v.numpy() for k, v in params.items()}
        ref = index_c.segment_classifier(fam.X, fam.src, fam.dst, p, T, f64=True).astype(np.float64)
        ref32 = index_c.segment_classifier(fam.X, fam.src, fam.dst, p, T, f64=False)
        cond = float(np.abs(ref32 - ref).max())
        _record("exp-product %s %s D%d seed %d: fp32 oracle vs fp64" % (side, fam_name, D, seed), cond,
                float(np.abs(ref).max()))
        if cond < FP32_PRECONDITION:
            break
    assert cond < FP32_PRECONDITION, ("fp32 itself drifts at these weights for every seed tried", cond)
    assert (bd <= 60.0) == fast
    m.use_events, m.use_plan = False, True
    with torch.no_grad(), hip.profile(512) as prof:
        e = m(b)
        torch.cuda.synchronize()
    assert m._xp_cache[1] == (hip.GNN_FLAG_EXP_PRODUCT if fast else 0)
    if D >= 32:
        assert "k_iter_wx" in {k for k, _ in prof.records}
    _assert_scores(e, ref, "exp-product %s %s F%d D%d T%d (bound %.1f)" % (side, fam_name, F, D, T, bd))
