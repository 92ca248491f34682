"""gnn_fpga_amd/call_route.py without a GPU: both decision tables ("Which route a model call takes")
row by row and on both sides of every boundary, the wrappers on stub batches (plain objects: the wrappers need no device
tensors), the two per-batch counters, and the two constants' single place in the sources."""
import os
import re
import types

import pytest

from gnn_fpga_amd import HitGraphBatch, call_route as cr, synth
from gnn_fpga_amd.hitgraph import _EventLayout
from gnn_fpga_amd.model import SegmentClassifier

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lay(h, s):
    return _EventLayout([0, h], [0, s])


class StubBatch:
    """What the wrappers read of a batch, with call counts."""

    def __init__(self, n_graphs=1, n_hits=100, n_segments=500, layout=None, plan_dim=None, twin="new", twin_attrs=()):
        self.n_graphs, self.n_hits, self.n_segments = n_graphs, n_hits, n_segments
        self.plan = None if plan_dim is None else types.SimpleNamespace(hidden_dim=plan_dim)
        self._layout, self._twin_kind, self._twin_attrs = layout, twin, dict(twin_attrs)
        self._fused = self._fused_dim = None
        self.kept = {}
        self.calls = {"event_layout": 0, "build_plan": 0, "level_ordered": 0}

    def derived(self, kind, name, make=None):
        assert make is None
        return self.kept.get((kind, name))

    def remember(self, kind, name, value):
        self.kept[kind, name] = value

    def event_layout(self):
        self.calls["event_layout"] += 1
        return self._layout

    def build_plan(self, D):
        self.calls["build_plan"] += 1
        if self.plan is None or self.plan.hidden_dim != D:
            self.plan = types.SimpleNamespace(hidden_dim=D, n_pad=self.n_hits + 12, n_segments=self.n_segments)
        return self.plan

    def level_ordered(self, D):
        self.calls["level_ordered"] += 1
        if self.derived("features", "twin") is None:
            if self._twin_kind == "self":
                self.remember("features", "twin", self)
            else:
                plan = self.build_plan(D)
                attrs = dict(n_hits=plan.n_pad, n_segments=plan.n_segments, _fused=plan, _fused_dim=D)
                attrs.update(self._twin_attrs)
                self.remember("features", "twin", types.SimpleNamespace(**attrs))
        return self.derived("features", "twin")


def model(F=3, D=8, **knobs):
    m = SegmentClassifier(input_dim=F, hidden_dim=D, n_iters=2)
    for k, v in knobs.items():
        setattr(m, k, v)
    return m


# ---- inference -------------------------------------------------------------------------------------------------------
def inference(F=3, D=8, trace=False, use_events=True, use_plan="auto", max_segments=4_000_000, n_graphs=1,
              n_segments=500, layout=None, plan_dim=None, seen=0):
    return cr.choose_inference(F, D, trace, use_events, use_plan, max_segments, n_graphs, n_segments, layout, plan_dim, seen)


def test_inference_events_row():
    small = lay(150, 1200)
    assert inference(layout=small) == ("events", False)
    assert inference(layout=small, n_graphs=1024).kind == "events"
    assert inference(layout=small, n_graphs=1025, use_plan=False).kind == "per_module"
    assert inference(layout=lay(150, 1201), use_plan=False).kind == "per_module"
    assert inference(layout=small, use_events=False, use_plan=False).kind == "per_module"
    assert inference(layout=None, use_plan=False).kind == "per_module"
    assert inference(D=16, layout=lay(100, 250)).kind == "events"
    assert inference(D=32, layout=lay(100, 250), use_plan=True).kind == "plan"           # wide: never the one-launch kernels
    assert inference(F=5, D=7, layout=small, use_plan=True).kind == "per_module"         # no kernel: nothing is preferred


@pytest.mark.parametrize("use_plan,kind,bump", [(False, "per_module", False), (True, "plan", False),
                                                ("auto", "per_module", True)])
def test_inference_use_plan(use_plan, kind, bump):
    assert inference(use_plan=use_plan) == (kind, bump)
    assert inference(use_plan=use_plan, trace=True) == ("per_module", False)
    assert inference(use_plan=use_plan, trace=True, layout=lay(40, 150)) == ("per_module", False)


def test_inference_auto():
    assert inference(plan_dim=8) == ("plan", False)                  # carries a plan of this width: counter untouched
    assert inference(plan_dim=4) == ("per_module", True)             # ... of another width: as if it had none
    assert inference(seen=0) == ("per_module", True)
    assert inference(seen=1) == ("plan", True)
    for D, limit in ((8, 2000), (32, 1000), (64, 300)):              # first_forward_max_segments = 2000
        assert cr.first_forward_limit(2000, D) == limit
        assert inference(D=D, max_segments=2000, n_segments=limit) == ("per_module", True)
        assert inference(D=D, max_segments=2000, n_segments=limit + 1) == ("plan", True)


def test_inference_route_on_stub_batches():
    m = model(use_plan="auto", first_forward_max_segments=2000)
    b = StubBatch(n_segments=2000)
    kinds = [cr.inference_route(m, b, 8).kind for _ in range(3)]
    assert kinds == ["per_module", "plan", "plan"] and m._route.kind == "plan"
    assert b.derived("host", "forwards") == 2                                          # (the third call found the plan: no bump)
    assert b.calls == {"event_layout": 3, "build_plan": 2, "level_ordered": 0}
    big = StubBatch(n_segments=2001)
    r = cr.inference_route(m, big, 8)
    assert r.kind == "plan" and r.plan is big.plan and r.batch is big and big.derived("host", "forwards") == 1
    ev = StubBatch(n_graphs=8, layout=lay(40, 150))
    r = cr.inference_route(m, ev, 8)
    assert r == ("events", ev._layout, None, ev) and ev.derived("host", "forwards") is None and ev.calls["event_layout"] == 1
    many = StubBatch(n_graphs=1025, layout=lay(40, 150))
    assert cr.inference_route(m, many, 8).kind == "per_module" and many.calls["event_layout"] == 0
    # the width the kernels run at decides, not the module's
    assert cr.inference_route(model(D=32, use_plan=False), StubBatch(layout=lay(40, 150)), 16).kind == "events"


@pytest.mark.parametrize("use_events", [False, True])
@pytest.mark.parametrize("use_plan", [False, True, "auto"])
def test_trace_is_per_module_whatever_the_knobs(use_events, use_plan):
    m = model(use_events=use_events, use_plan=use_plan)
    b = StubBatch(layout=lay(40, 150), plan_dim=8)
    r = cr.inference_route(m, b, 8, trace=True)
    assert r == ("per_module", None, None, b) and b.derived("host", "forwards") is None
    assert b.calls == {"event_layout": 0, "build_plan": 0, "level_ordered": 0}


def test_with_features_carries_the_forward_count():
    m = model(use_events=False, use_plan="auto")
    b = HitGraphBatch.from_graphs([synth.layered_graph(30, 50, 3, seed=0)])
    assert cr.inference_route(m, b, 8).kind == "per_module" and b._forwards == 1
    b2 = b.with_features(b.X + 1)
    assert b2._forwards == 1 and cr.inference_route(m, b2, 8).kind == "plan" and b2.plan is not None


# ---- training --------------------------------------------------------------------------------------------------------
def training(F=3, D=8, use_events=True, policy="auto", n_graphs=1, n_hits=20000, layout=None, has_twin=False, uses=0, **kw):
    return cr.choose_training(F, D, use_events, policy, n_graphs, n_hits, layout, has_twin, uses, **kw)


def test_training_events_row():
    small = lay(150, 1200)
    for n_graphs, kind in ((0, "pass"), (1, "events"), (1024, "events"), (1025, "pass")):
        assert training(n_graphs=n_graphs, layout=small, n_hits=100) == (kind, False)
    assert training(layout=small, uses=1) == ("events", False)                   # an events decision bumps nothing
    assert training(layout=small, use_events=False, n_hits=100).kind == "pass"
    assert training(layout=lay(150, 1201), n_hits=100).kind == "pass"
    assert training(D=32, layout=lay(40, 144), n_hits=100).kind == "pass"


def test_training_twin_rows():
    assert training(policy=True, n_hits=19999) == ("pass", False)
    assert training(policy=True, n_hits=20000) == ("twin", False)
    assert training(policy=False, n_hits=20000) == ("pass", False)
    assert training(policy="auto", uses=0) == ("pass", True)
    assert training(policy="auto", uses=1) == ("twin", True)
    assert training(policy="auto", uses=0, has_twin=True) == ("twin", False)
    assert training(policy="auto", n_hits=19999) == ("pass", False)
    assert training(policy=True, twin_differs=False) == ("pass", False)
    assert training(policy=True, fused=False) == ("twin_pp", False)
    assert training(policy="auto", uses=1, fused=False) == ("twin_pp", True)


def test_training_route_on_stub_batches():
    m = model(level_order_training="auto")
    b = StubBatch(n_hits=20000, n_segments=90000)
    routes = [cr.training_route(m, b) for _ in range(3)]
    assert [r.kind for r in routes] == ["pass", "twin", "twin"] and b.derived("host", "train_uses") == 2
    twin = b.derived("features", "twin")
    assert routes[0].batch is b and routes[1].batch is twin and routes[2].batch is twin and m._route.kind == "twin"
    assert b.calls == {"event_layout": 3, "build_plan": 1, "level_ordered": 2}
    assert cr.training_route(model(level_order_training=True), StubBatch(n_hits=19999)).kind == "pass"
    own = StubBatch(n_hits=20000, twin="self")                       # nothing to gain: level_ordered returns the batch
    r = cr.training_route(model(level_order_training=True), own)
    assert r.kind == "pass" and r.batch is own and own.calls["level_ordered"] == 1 and own.derived("host", "train_uses") is None
    ev = StubBatch(n_graphs=8, n_hits=30000, layout=lay(40, 150))
    r = cr.training_route(m, ev)
    assert r == ("events", ev._layout, None, ev) and ev.derived("host", "train_uses") is None and ev.calls["level_ordered"] == 0


@pytest.mark.parametrize("broken", ["_fused", "_fused_dim", "env", "n_hits", "n_segments", None])
def test_each_condition_of_the_fused_training_forward(broken, monkeypatch):
    m = model(level_order_training=True)
    attrs = {"_fused": None, "_fused_dim": 4, "n_hits": 7, "n_segments": 7}
    b = StubBatch(n_hits=20000, twin_attrs={broken: attrs[broken]} if broken in attrs else {})
    if broken == "env":
        monkeypatch.setenv("GNN_NO_FUSED_TRAIN", "1")
    r = cr.training_route(m, b)
    assert r.kind == ("twin" if broken is None else "twin_pp") and r.batch is b.derived("features", "twin") and r.batch is not b


@pytest.mark.parametrize("F,D,kind", [(3, 8, "twin"), (11, 16, "twin"), (3, 32, "twin_pp"), (3, 64, "twin_pp"),
                                      (3, 16, "twin_pp"), (5, 7, "twin_pp")])
def test_the_library_says_which_shapes_have_a_fused_training_forward(F, D, kind):
    """gnn_plan_route's answer (choose_route in csrc/sell_pipeline.hip), not a list in Python; (5, 7): no fused kernels."""
    assert cr.training_route(model(F, D, level_order_training=True), StubBatch(n_hits=20000)).kind == kind


def test_the_model_keeps_the_kind_and_not_the_batch():
    """A model that kept its last batch (with the plan and the twin: tens of GB at detector scale) would hold their memory
    as long as it lives - and, through the plan's exp-product cache, which points at the model, in a reference cycle
    that `del batch, model` does not free."""
    import weakref
    m = model(level_order_training=True)
    for training in (False, True):
        b = StubBatch(n_hits=20000)
        r = cr.training_route(m, b) if training else cr.inference_route(m, b, 8)
        assert m._route.kind == r.kind and r.batch is not None and m._route[1:] == (None, None, None)
        alive = weakref.ref(b)
        del b, r
        assert alive() is None


def test_the_model_drops_its_last_route_when_copied():
    import copy
    m = model()
    cr.inference_route(m, StubBatch(), 8)
    assert m._route is not None and copy.deepcopy(m)._route is None and m.__getstate__()["_route"] is None


# ---- the sources -----------------------------------------------------------------------------------------------------
def test_each_constant_is_written_once():
    """The 1024-graph bound and the 20000-hit threshold used to be spelled out in model.py, autograd.py and shard.py.  Now
    20000 occurs once in the whole package, and 1024 once in the modules that decide or run a model call (elsewhere in
    the package the same number is a bin count, a chunk size and a workspace length: other quantities)."""
    pkg = os.path.join(REPO, "gnn-fpga_amd")
    src = {fn: open(os.path.join(pkg, fn)).read() for fn in os.listdir(pkg) if fn.endswith(".py")}
    count = lambda word, files: {fn: n for fn in files for n in [len(re.findall(r"\b%s\b" % word, src[fn]))] if n}
    assert count("20000", src) == {"call_route.py": 1}
    assert count("1024", ("call_route.py", "model.py", "autograd.py", "shard.py", "hitgraph.py")) == {"call_route.py": 1}
    found = {fn: text.count("events_preferred(") for fn, text in src.items() if "events_preferred(" in text}
    assert found == {"_lib.py": 1, "call_route.py": 2}, found           # its definition and the two choose_* functions
