"""The call route (gnn_fpga_amd/call_route.py) on the GPU: the kind a model call records (`model._route`) and the
kernels that ran agree, for every kind; the "auto" policies step through their kinds; and a `twin_pp` step allocates
no more than the per-pass step plus the twin.  Shapes are the smallest at which each rule can go wrong: 8 muon graphs
(one-launch kernels), 600 hits (below every threshold), 21 000 hits (just past TWIN_MIN_HITS).

Kernel names as in test_gpu_fp64_reference.py: k_event / k_event_bwd the one-launch kernels, k_edge_tw the fused
training forward's last pass (`twin` only), k_iter* the fused tile pipeline, k_node the per-module node pass.
"""
import pytest
import torch

from gnn_fpga_amd import HitGraphBatch, synth
from gnn_fpga_amd.model import SegmentClassifier

pytestmark = pytest.mark.gpu

FUSED = {"k_iter", "k_iter2", "k_iter_w", "k_iter_wx"}


def _assert_kind(m, kind):
    assert m._route.kind == kind, (m._route.kind, kind)


def _batch(what):
    if what == "muon":              # events: F = 11
        graphs = [synth.muon_graph(s) for s in range(8)]
    elif what == "small":           # below every threshold
        graphs = [synth.layered_graph(300, 1500, 3, seed=s) for s in range(2)]
    elif what == "twin":            # 21 000 hits: just past the twin's threshold
        graphs = [synth.layered_graph(7000, 40000, 3, seed=10 + s) for s in range(3)]
    else:                           # "wide": the D = 32 twin
        graphs = [synth.layered_graph(10500, 50000, 3, seed=20 + s) for s in range(2)]
    return HitGraphBatch.from_graphs(graphs).cuda()


def _model(F, D, T, train, **knobs):
    torch.manual_seed(3)
    m = SegmentClassifier(input_dim=F, hidden_dim=D, n_iters=T).cuda()
    m.train() if train else m.eval()
    for k, v in knobs.items():
        setattr(m, k, v)
    return m


def _call(hip, m, b, train):
    """One model call (training: with its backward) -> the names of the kernels that ran."""
    with hip.profile(512) as prof:
        if train:
            m.zero_grad()
            m(b).sum().backward()
        else:
            with torch.no_grad():
                m(b)
        torch.cuda.synchronize()
    return {k for k, _ in prof.records}


def test_inference_events(hip):
    m = _model(11, 8, 3, False, use_events=True)
    names = _call(hip, m, _batch("muon"), False)
    _assert_kind(m, "events")
    assert "k_event" in names and not names & FUSED and "k_node" not in names, sorted(names)


def test_inference_plan(hip):
    m = _model(3, 8, 3, False, use_events=False, use_plan=True)
    b = _batch("small")
    names = _call(hip, m, b, False)
    _assert_kind(m, "plan")
    assert names & FUSED and "k_event" not in names and "k_node" not in names, sorted(names)
    assert b.plan is not None


def test_inference_per_module(hip):
    m = _model(3, 8, 3, False, use_events=False, use_plan=False)
    b = _batch("small")
    names = _call(hip, m, b, False)
    _assert_kind(m, "per_module")
    assert {"k_input", "k_edge", "k_node"} <= names and not names & FUSED and "k_event" not in names, sorted(names)
    assert b.plan is None


def test_inference_auto_goes_from_per_module_to_plan(hip):
    m = _model(3, 8, 3, False, use_events=False, use_plan="auto")
    b = _batch("small")
    first = _call(hip, m, b, False)
    _assert_kind(m, "per_module")
    second = _call(hip, m, b, False)
    _assert_kind(m, "plan")
    assert "k_node" in first and not first & FUSED, sorted(first)
    assert second & FUSED and "k_node" not in second, sorted(second)


def test_training_events(hip):
    m = _model(11, 8, 3, True, use_events=True)
    b = _batch("muon")
    names = _call(hip, m, b, True)
    _assert_kind(m, "events")
    assert {"k_event", "k_event_bwd"} <= names and "k_edge_tw" not in names, sorted(names)
    assert getattr(b, "_twin", None) is None


def test_training_pass(hip):
    m = _model(3, 8, 3, True, use_events=False, level_order_training=True)      # 600 hits: no twin at any policy
    b = _batch("small")
    names = _call(hip, m, b, True)
    _assert_kind(m, "pass")
    assert getattr(b, "_twin", None) is None
    assert "k_seg_bwd4" in names and "k_edge_tw" not in names and "k_event_bwd" not in names, sorted(names)


def test_training_twin(hip):
    m = _model(3, 8, 2, True, use_events=False, level_order_training=True)
    b = _batch("twin")
    assert b.n_hits == 21000
    names = _call(hip, m, b, True)
    _assert_kind(m, "twin")
    assert getattr(b, "_twin", None) is not None and b._twin is not b
    assert "k_edge_tw" in names and "k_seg_bwd4" in names and "k_event_bwd" not in names, sorted(names)


@pytest.mark.parametrize("why", ["GNN_NO_FUSED_TRAIN", "hidden_dim 32"])
def test_training_twin_per_module_forward(hip, why, monkeypatch):
    if why == "GNN_NO_FUSED_TRAIN":
        monkeypatch.setenv("GNN_NO_FUSED_TRAIN", "1")
        m, b = _model(3, 8, 2, True, use_events=False, level_order_training=True), _batch("twin")
    else:
        m, b = _model(3, 32, 1, True, use_events=False, level_order_training=True), _batch("wide")
    names = _call(hip, m, b, True)
    _assert_kind(m, "twin_pp")
    assert getattr(b, "_twin", None) is not None and b._twin is not b
    assert "k_edge_tw" not in names and not names & FUSED and names & {"k_node", "k_node_walkW"}, sorted(names)
    assert ("k_seg_bwdW" if m.hidden_dim >= 32 else "k_seg_bwd4") in names, sorted(names)


def test_training_auto_goes_from_pass_to_twin(hip):
    m = _model(3, 8, 2, True, use_events=False)
    assert m.level_order_training == "auto"
    b = _batch("twin")
    first = _call(hip, m, b, True)
    _assert_kind(m, "pass")
    assert getattr(b, "_twin", None) is None and "k_edge_tw" not in first, sorted(first)
    second = _call(hip, m, b, True)
    _assert_kind(m, "twin")
    assert b._twin is not b and "k_edge_tw" in second, sorted(second)
    third = _call(hip, m, b, True)
    _assert_kind(m, "twin")
    assert "k_edge_tw" in third and "k_event_bwd" not in third, sorted(third)


def test_a_model_does_not_keep_its_last_batch_alive(hip):
    """The plan's exp-product cache points at the model; a model that pointed back at its last batch would make a cycle
    that holds the batch's, the plan's and the twin's device memory until a garbage collection."""
    import weakref
    m = _model(3, 8, 2, False, use_events=False, use_plan=True)
    b = _batch("small")
    _call(hip, m, b, False)
    assert b.plan._xp[0] is m
    m.train()
    m.level_order_training = True
    t = _batch("twin")
    _call(hip, m, t, True)
    alive = [weakref.ref(b), weakref.ref(b.plan), weakref.ref(t)]
    m.zero_grad()
    del b, t
    # (the twin, and the plan it holds as `_fused`, wait for a collection as before: a twin is its own `_twin`)
    assert [r() for r in alive] == [None] * 3
    _assert_kind(m, "twin")


def _tensor_bytes(obj):
    seen, total = set(), 0
    for v in [getattr(obj, k) for k in obj.__slots__ if k != "__weakref__"] + list(obj._csr or ()):
        if torch.is_tensor(v) and v.is_cuda and v.data_ptr() not in seen:
            seen.add(v.data_ptr())
            total += v.numel() * v.element_size()
    return total


def test_twin_pp_step_allocates_no_more_than_the_pass_step_plus_the_twin(hip):
    """A `twin_pp` training step (forward + backward, D = 32, T = 1, 2 x (10 500 hits, 50 000 segments)) against the same
    step with level_order_training = False: torch.cuda.max_memory_allocated() above the level the step starts at.  Both
    batches have made one step before (plan, twin and segment lists exist), so the two steps differ by the twin's
    numbering - more hit rows (n_pad), two gathers between the segment orders - which the twin's own tensors bound.
    Measured on MI355X: twin_pp 69 403 136 bytes, pass 68 976 128, the twin's tensors 4 823 372.  The commit before the
    route was decided ahead of the call passes this too (69 360 640 against 68 912 128): it allocated the fused training
    forward's e_all / H_all / Q_all / e_out and workspace, was told GNN_ERR_UNSUPPORTED and dropped them BEFORE the
    per-module forward allocated its own, and the step's peak lies in the backward - the waste was allocator traffic
    and host time on every step, not peak memory."""
    def peak(level_order):
        m = _model(3, 32, 1, True, use_events=False, level_order_training=level_order)
        b = _batch("wide")

        def step():
            m.zero_grad()
            m(b).sum().backward()
            torch.cuda.synchronize()
        step()
        torch.cuda.reset_peak_memory_stats()
        start = torch.cuda.memory_allocated()
        step()
        return torch.cuda.max_memory_allocated() - start, b

    pass_peak, _ = peak(False)
    twin_peak, b = peak(True)
    assert b._twin is not None and b._twin is not b
    twin_bytes = _tensor_bytes(b._twin)
    print("twin_pp step peak %d bytes, pass step peak %d bytes, the twin's tensors %d bytes"
          % (twin_peak, pass_peak, twin_bytes))
    assert twin_peak <= pass_peak + twin_bytes, (twin_peak, pass_peak, twin_bytes)
