"""Derived state of batches and plans on the GPU ("Declared fields, derived state"): after
`with_features` to other features, `with_features` back, and a device round trip, a batch that has been through a model
call gives the bits a freshly built batch of the same arrays gives - on the one-launch route, the plan route and the
twin route (there: scores and the ten gradients of one training step) - and what had to be made again was made again.
Shapes are the smallest that reach each route: 3 graphs of 40 hits / 150 segments, one 600-hit graph, one graph just
past call_route.TWIN_MIN_HITS."""
import pytest
import torch

from gnn_fpga_amd import HitGraphBatch, call_route, synth
from gnn_fpga_amd.loss import BCELoss
from gnn_fpga_amd.model import SegmentClassifier

pytestmark = pytest.mark.gpu

ROUTES = ("events", "plan", "twin")
_GRAPHS = {}


def _graphs(route):
    if route not in _GRAPHS:
        _GRAPHS[route] = {"events": lambda: [synth.layered_graph(40, 150, 3, seed=30 + s) for s in range(3)],
                          "plan": lambda: [synth.layered_graph(600, 3000, 3, seed=31)],
                          "twin": lambda: [synth.layered_graph(21000, 60000, 3, seed=32)]}[route]()
    return _GRAPHS[route]


def _model(route, device="cuda"):
    torch.manual_seed(5)
    m = SegmentClassifier(input_dim=3, hidden_dim=8, n_iters=2).to(device)
    m.use_events = route == "events"
    if route == "twin":
        m.level_order_training = True
        return m.train()
    return m.eval()


def _built(route, device="cuda"):
    b = HitGraphBatch.from_graphs(_graphs(route)).to(device)
    assert route != "twin" or b.n_hits >= call_route.TWIN_MIN_HITS
    b.hit_index = torch.arange(b.n_hits, device=device)          # what a graph builder leaves on its batches
    return b


def _fresh(b, X=None):
    """A batch nobody has seen, from the arrays `b` holds (X: other features), on b's device."""
    X = b.X if X is None else X
    return HitGraphBatch(X.cpu().numpy(), b.src.cpu().numpy(), b.dst.cpu().numpy(), y=b.y.cpu().numpy(),
                         hit_ptr=b.hit_ptr, seg_ptr=b.seg_ptr).to(b.device)


def _run(route, m, b):
    """One call on `route` -> [scores] (twin: + the ten gradients of one training step)."""
    if route != "twin":
        with torch.no_grad():
            out = [m(b).clone()]
    else:
        m.zero_grad()
        e = m(b)
        BCELoss(reduction="sum")(e, b.y).backward()
        out = [e.detach().clone()] + [p.grad.detach().clone() for p in m.parameters()]
        assert len(out) == 11
    assert m._route.kind == route, m._route.kind
    return out


def _assert_bits(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.device == w.device and torch.equal(g, w), "%s: tensor %d differs by %g" % (
            what, i, float((g - w).abs().max()))


def _seen(route, m, b):
    """Everything a call leaves on a batch is there: lists, structs, layout pointers, plan / twin."""
    out = _run(route, m, b)
    b.in_ptr
    if route == "events":
        _run(route, m, b)                                         # (now on the struct with the lists)
        assert b.derived("features", "gstruct") is not None and b.derived("device", "layout") is not None
    elif route == "plan":
        assert b.plan.derived("features", "struct") is not None and b.plan.derived("features", "xp")[0] is m
    else:
        twin = b.derived("features", "twin")
        assert twin is not b and twin.hit_index is None and twin.seg_order is not None
        assert twin.derived("device", "n_valid") == b.n_segments and twin.derived("features", "gstruct") is not None
    return out


def _made_again(route, m, before, after, old):
    """`after` (which has run) holds none of the feature-dependent objects `before` held (`old`: taken before)."""
    if route == "plan":
        xp = after.plan.derived("features", "xp")
        assert xp is not None and xp[0] is m and xp is not old["xp"]
        assert after.plan.derived("features", "struct") is not old["struct"]
    if route == "twin":
        twin = after.derived("features", "twin")
        assert twin is not None and twin is not after and twin is not old["twin"]
    if route == "events":
        assert after.derived("features", "gstruct") is not old["gstruct"]


def _old(route, b):
    return {"xp": b.plan and b.plan.derived("features", "xp"), "struct": b.plan and b.plan.derived("features", "struct"),
            "twin": b.derived("features", "twin"), "gstruct": b.derived("features", "gstruct")}


@pytest.mark.parametrize("route", ROUTES)
def test_with_features_and_back(hip, route):
    m, b = _model(route), _built(route)
    first = _seen(route, m, b)
    old, lists = _old(route, b), b.derived("device", "csr")
    torch.manual_seed(9)
    X2 = (b.X * 0.5 + 0.1 * torch.randn_like(b.X)).contiguous()
    b2 = b.with_features(X2)
    assert b2.hit_index is b.hit_index and b2._derived["features"] == {} and b2.derived("device", "csr") is lists
    got = _run(route, m, b2)
    _assert_bits(got, _run(route, m, _fresh(b, X2)), "other features")
    assert not torch.equal(got[0], first[0])
    _made_again(route, m, b, b2, old)
    b3 = b2.with_features(b.X.clone())
    got = _run(route, m, b3)
    _assert_bits(got, first, "the first features again, against the first call")
    _assert_bits(got, _run(route, m, _fresh(b)), "the first features again")
    _made_again(route, m, b2, b3, _old(route, b2))
    _assert_bits(_run(route, m, b), first, "the batch the copies were made from")      # untouched by its copies


@pytest.fixture
def layout_checks(monkeypatch):
    """How often a batch's event layout was worked out on the host."""
    calls, real = [], HitGraphBatch._event_sizes
    monkeypatch.setattr(HitGraphBatch, "_event_sizes", lambda batch: calls.append(batch) or real(batch))
    return calls


@pytest.mark.parametrize("route", ROUTES)
def test_device_round_trip(hip, route, layout_checks):
    m, b = _model(route), _built(route)
    first = _seen(route, m, b)
    b.event_layout()
    old, event = _old(route, b), b.derived("host", "event")
    assert event is not None and bool(event) == (route == "events") and layout_checks == [b]
    assert b.to("cpu") is b and not b.X.is_cuda
    assert b._derived["features"] == {} and set(b._derived["device"]) <= {"csr", "csr_status"}
    assert not b.derived("device", "csr")[0].is_cuda
    b.cuda()
    assert b.derived("device", "csr")[0].is_cuda and b.derived("host", "event") is event       # not computed again
    got = _run(route, m, b)
    _assert_bits(got, first, "after cpu -> cuda, against the first call")
    _assert_bits(got, _run(route, m, _fresh(b)), "after cpu -> cuda")
    _made_again(route, m, b, b, old)
    b.event_layout()
    assert b.derived("host", "event") is event and sum(c is b for c in layout_checks) == 1


@pytest.mark.parametrize("route", ROUTES)
def test_move_to_a_second_device(hip, route):
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU visible")
    m, b = _model(route), _built(route)
    _seen(route, m, b)
    b.event_layout()
    old, event = _old(route, b), b.derived("host", "event")
    b.to("cuda:1")
    m.to("cuda:1")
    got = _run(route, m, b)
    assert got[0].device == torch.device("cuda:1") and b.derived("host", "event") is event
    _assert_bits(got, _run(route, m, _fresh(b)), "on the second device")
    _made_again(route, m, b, b, old)
