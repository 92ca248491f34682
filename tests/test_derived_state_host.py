"""HitGraphBatch and SellPlan without a GPU: every field is declared, derived state sits in the stores that `to`,
`with_features` and `forget` treat as DESIGN.md section 3 says."""
import numpy as np
import pytest
import torch

from gnn_fpga_amd import HitGraphBatch, call_route as cr, synth
from gnn_fpga_amd.model import SegmentClassifier
from gnn_fpga_amd.plan import SellPlan

FIELDS = [k for k in HitGraphBatch.__slots__ if k != "__weakref__"]
G = synth.layered_graph(60, 200, 3, seed=5)


def _dense(g):
    n, e = g.X.shape[0], g.src.shape[0]
    Ri, Ro = np.zeros((1, n, e), np.float32), np.zeros((1, n, e), np.float32)
    Ri[0, g.dst, np.arange(e)] = 1
    Ro[0, g.src, np.arange(e)] = 1
    return g.X[None], Ri, Ro


def _sparse(g):
    e = np.arange(g.src.shape[0])
    oi, oo = np.argsort(g.dst, kind="stable"), np.argsort(g.src, kind="stable")
    return g.X, g.dst[oi], e[oi], g.src[oo], e[oo]


def _npz(g, tmp_path):
    X, Ri_rows, Ri_cols, Ro_rows, Ro_cols = _sparse(g)
    fn = str(tmp_path / "g.npz")
    np.savez(fn, X=X, Ri_rows=Ri_rows, Ri_cols=Ri_cols, Ro_rows=Ro_rows, Ro_cols=Ro_cols, y=g.y)
    return fn


CONSTRUCTORS = {
    "init": lambda tmp: HitGraphBatch(G.X, G.src, G.dst, y=G.y),
    "from_graphs": lambda tmp: HitGraphBatch.from_graphs([G, G]),
    "from_graphs_padded": lambda tmp: HitGraphBatch.from_graphs([G, synth.layered_graph(30, 50, 3, seed=1)], pad_segments=True),
    "from_dense": lambda tmp: HitGraphBatch.from_dense(*_dense(G)),
    "from_sparse_arrays": lambda tmp: HitGraphBatch.from_sparse_arrays(*_sparse(G), y=G.y),
    "from_npz": lambda tmp: HitGraphBatch.from_npz(_npz(G, tmp)),
    "device_arrays": lambda tmp: HitGraphBatch._from_device_arrays(
        torch.from_numpy(G.X), torch.from_numpy(G.src.astype(np.int32)), torch.from_numpy(G.dst.astype(np.int32)), None,
        [0, G.X.shape[0]], [0, G.src.shape[0]]),
}


def _state(b):
    """Every declared field but the stores, and the stores' entries by name."""
    plain = {k: getattr(b, k) for k in FIELDS if k != "_derived"}
    return plain, {kind: sorted(map(str, store)) for kind, store in b._derived.items()}


def _same(a, b):
    if torch.is_tensor(a) or isinstance(a, np.ndarray):
        return type(a) is type(b) and a.shape == b.shape and bool((a == b).all())
    return a is b or a == b


@pytest.mark.parametrize("how", sorted(CONSTRUCTORS))
def test_every_field_is_declared_and_set(how, tmp_path):
    b = CONSTRUCTORS[how](tmp_path)
    for k in FIELDS:
        getattr(b, k)                                   # no AttributeError
    assert not hasattr(b, "__dict__")
    with pytest.raises(AttributeError):
        b._gstruct = None                               # what a module would have invented before
    with pytest.raises(AttributeError):
        b.anything = 1
    assert b.seg_order is None and b.seg_rank is None and b._fused is None and b._fused_dim is None
    assert b.plan is None and b.hit_index is None and b.validate_csr is False
    assert sorted(b._derived) == ["device", "features", "host"] and b._derived["features"] == {}
    assert b.derived("host", "forwards") is None and b.derived("features", "twin") is None
    brought = how in ("from_sparse_arrays", "from_npz")
    assert (b.derived("device", "csr") is not None) == brought
    b.in_ptr
    assert len(b.derived("device", "csr")) == 6


@pytest.mark.parametrize("how", sorted(CONSTRUCTORS))
def test_forget_gives_the_constructors_state(how, tmp_path):
    b, fresh = CONSTRUCTORS[how](tmp_path), CONSTRUCTORS[how](tmp_path)
    brought = how in ("from_sparse_arrays", "from_npz")          # (lists the caller brought are rebuilt from src / dst)
    lists = [getattr(fresh, n).clone() for n in HitGraphBatch._CSR_NAMES]
    m = SegmentClassifier(input_dim=3, hidden_dim=8, n_iters=1)
    m.use_plan, m.use_events = "auto", False
    cr.inference_route(m, b, 8)
    cr.inference_route(m, b, 8)                                  # the second call builds the plan
    b.event_layout()
    assert b.plan is not None and b.derived("host", "forwards") == 2 and b.derived("host", "event") is not None
    b.in_ptr, b.level_ordered(8), b.derived("device", "mine", lambda batch: batch.n_hits)
    assert b.derived("device", "mine") == b.n_hits and b.derived("features", "twin") is b        # CPU: nothing to gain
    assert b.forget() is b
    fresh = CONSTRUCTORS[how](tmp_path)
    (plain, stores), (want, want_stores) = _state(b), _state(fresh)
    assert all(_same(plain[k], want[k]) for k in plain), [k for k in plain if not _same(plain[k], want[k])]
    assert stores == ({"host": [], "device": [], "features": []} if brought else want_stores)
    assert all(torch.equal(getattr(b, n), w) for n, w in zip(HitGraphBatch._CSR_NAMES, lists))


def test_with_features_shares_structure_and_starts_features_empty():
    b = HitGraphBatch.from_graphs([G, G])
    b.hit_index = torch.arange(b.n_hits)
    m = SegmentClassifier(input_dim=3, hidden_dim=8, n_iters=1)
    m.use_plan, m.use_events = "auto", False
    cr.inference_route(m, b, 8)
    b.in_ptr, b.event_layout(), b.build_plan(8), b.level_ordered(8)
    b.remember("features", "gstruct", object())
    b2 = b.with_features(b.X * 2)
    assert b2 is not b and b2.src is b.src and b2.dst is b.dst and b2.hit_index is b.hit_index
    assert b2._derived["features"] == {} and b._derived["features"] != {}
    assert b2._derived["device"] is b._derived["device"] and b2.derived("device", "csr") is b.derived("device", "csr")
    assert b2.derived("device", "layout") is b.derived("device", "layout")
    assert b2._derived["host"] == b._derived["host"] and b2._derived["host"] is not b._derived["host"]
    assert b2.derived("host", "event") is b.derived("host", "event") and b2.derived("host", "forwards") == 1
    assert b2.plan is not b.plan and b2.plan.hidden_dim == 8 and b2.plan.src is b.plan.src
    b2.plan = None
    assert cr.inference_route(m, b2, 8).kind == "plan" and b2.derived("host", "forwards") == 2      # a bump on the copy
    assert b.derived("host", "forwards") == 1
    b.remember("host", "train_uses", 3)
    assert b2.derived("host", "train_uses") is None
    # a device move empties what points into the old device's memory and keeps the host part
    event = b.derived("host", "event")
    b.remember("features", "gstruct", object())
    b.to("cpu")
    assert b._derived["features"] == {} and sorted(b._derived["device"]) == ["csr"]
    assert b.derived("host", "event") is event and b.derived("host", "forwards") == 1
    assert b2.derived("device", "layout") is not None              # the copy's stores are its own


def test_plan_stores():
    b = HitGraphBatch.from_graphs([G, G])
    plan = b.build_plan(8)
    assert isinstance(plan, SellPlan) and plan.hidden_dim == 8
    assert plan._derived == {"structure": {}, "features": {}}
    plan.remember("features", "struct", object())
    plan.remember("features", "xp", (None, 0, 0))
    plan.remember("structure", ("ws_need", 3, 8), 1234)
    p2 = plan.with_features(b.X + 1)
    rows = plan.derived("structure", "feature_rows")
    assert rows is not None and p2.derived("structure", "feature_rows") is rows
    assert p2.derived("structure", ("ws_need", 3, 8)) == 1234 and p2._derived["structure"] is plan._derived["structure"]
    assert p2.derived("features", "struct") is None and p2.derived("features", "xp") is None
    assert plan.derived("features", "xp") == (None, 0, 0) and p2.hidden_dim == 8
    assert p2.in_nbr is plan.in_nbr and p2.X is not plan.X
    p2.to("cpu")
    assert p2._derived == {"structure": {}, "features": {}} and plan.derived("structure", "feature_rows") is rows
