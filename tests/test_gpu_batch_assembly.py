"""Batch assembly ON THE DEVICE against the restatement of tests/batch_cases.py, and what the kernels make of the
batches: `GraphStore(..., device="cuda")` window by window (tensors and the lists of gnn_csr_build), the reference's
own tail window (tests/golden/batchgen_sector_tail.npz: n_samples = 5 of six graphs) scored from a list and from a
device store, and one epoch of training - tail window included - fed by either, bit for bit, with the first step's
gradients against fp64 autograd.  Malformed graphs are refused on the host: nothing of them reaches a kernel."""
import numpy as np
import pytest
import torch

import gnn_fpga_amd
from batch_cases import LAYOUTS, MALFORMED, MUON, RAGGED, assemble, assert_batch_equal, windows
from gnn_fpga_amd import HitGraphBatch
from gnn_fpga_amd.batcher import GraphStore, merge_graphs
from golden_util import assert_grad_close
from oracle import index_c, index_torch
from test_batcher_host import _fx, _sparse_graphs
from test_gpu_formats import TOL, _model

pytestmark = pytest.mark.gpu


def _device_windows(store, layout):
    compared = 0
    for j in range(7):
        for k in range(1, 9):
            got = store.batch(j, k, layout)
            assert_batch_equal(got, assemble(RAGGED, j, k, layout), device="cuda")
            b = got[0]
            # gnn_csr_build's lists: all n_segments entries (the list, then -1), and no malformed endpoint seen
            assert b.in_eid.numel() == b.n_segments and b.out_nbr.numel() == b.n_segments
            assert int(b.derived("device", "csr_status").item()) == 0
            compared += 1
    return compared


def test_device_store_every_window_equals_the_restatement(hip):
    """j in 0..6, batch_size in 1..8, both layouts: 2 x 56 = 112 windows of a store built from the list."""
    store = GraphStore(RAGGED, device="cuda")
    assert all(t.is_cuda for t in (store.X, store.src, store.dst, store.y))
    compared = {layout: _device_windows(store, layout) for layout in LAYOUTS}
    assert compared == {"padded": 56, "flat": 56} and sum(compared.values()) == 112


def test_store_of_a_device_batch_every_window_equals_the_restatement(hip):
    """The same 112 windows of GraphStore.from_batch on a batch that lives on the device."""
    whole = HitGraphBatch.from_graphs(RAGGED).cuda()
    store = GraphStore.from_batch(whole)
    assert store.device.type == "cuda" and store.src.is_cuda
    compared = {layout: _device_windows(store, layout) for layout in LAYOUTS}
    assert compared == {"padded": 56, "flat": 56} and sum(compared.values()) == 112
    assert_batch_equal((whole, whole.y), assemble(RAGGED, 0, 7, "flat"), device="cuda")      # (left as it was)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_tail_fixture_scores_from_a_list_and_from_a_device_store(hip, layout):
    """The reference's three batches of n_samples = 5, batch_size = 2 over six graphs - the third is graphs[4:6] -
    scored by both kernel routes: scores and loss at test_gpu_formats' bounds, the two feeds the same bits."""
    from gnn_fpga_amd.loss import BCELoss
    d = _fx("batchgen_sector_tail")
    graphs = _sparse_graphs(d)
    assert (len(graphs), int(d["n_samples"]), int(d["batch_size"]), int(d["n_batches"])) == (6, 5, 2, 3)
    kw = dict(n_samples=5, batch_size=2, layout=layout)
    feeds = (gnn_fpga_amd.batch_generator(graphs, device="cuda", **kw),
             gnn_fpga_amd.batch_generator(GraphStore(graphs, device="cuda"), **kw))
    m = _model(d, 3).eval()
    for b in range(3):
        ref = d["b%d.scores" % b]
        items = [next(gen) for gen in feeds]
        outs = []
        for batch, y in items:
            assert batch.X.is_cuda and y.is_cuda and batch.n_graphs == 2
            for events in (True, False):
                m.use_events = events
                with torch.no_grad():
                    out = m(batch)
                outs.append(out)
                if layout == "padded":
                    assert tuple(out.shape) == ref.shape
                    assert np.abs(out.cpu().numpy() - ref).max() < TOL
                    assert abs(BCELoss()(out, y).item() - float(d["b%d.loss" % b])) < 1e-6
                    assert np.array_equal(y.cpu().numpy(), d["b%d.y" % b])
                else:
                    counts = np.diff(batch.seg_ptr)
                    want = np.concatenate([ref[i, :c] for i, c in enumerate(counts)])
                    assert np.abs(out.cpu().numpy() - want).max() < TOL
        assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3])


def _epoch(graphs, from_store, F, D, T, use_events):
    """Three steps of zero_grad / forward / BCELoss / backward / Adam over n_samples = 5, batch_size = 2."""
    from gnn_fpga_amd.loss import BCELoss
    from gnn_fpga_amd.model import SegmentClassifier
    torch.manual_seed(9)
    m = SegmentClassifier(input_dim=F, hidden_dim=D, n_iters=T).cuda().train()
    m.use_events = use_events
    start = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    opt = torch.optim.Adam(m.parameters(), lr=0.02)
    if from_store:
        gen = gnn_fpga_amd.batch_generator(GraphStore(graphs, device="cuda"), n_samples=5, batch_size=2)
    else:
        gen = gnn_fpga_amd.batch_generator(graphs, n_samples=5, batch_size=2, device="cuda")
    steps, kinds, first_grads = [], [], None
    for step in range(3):
        batch, y = next(gen)
        m.zero_grad()
        out = m(batch)
        loss = BCELoss()(out, y)
        loss.backward()
        kinds.append(m._route.kind)
        if step == 0:
            first_grads = {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()}
        opt.step()
        steps.append((loss.detach().cpu().clone(), [p.detach().cpu().clone() for p in m.parameters()]))
    return start, steps, kinds, first_grads


@pytest.mark.parametrize("name,F,D,T,use_events,kind", [("ragged", 3, 8, 2, False, "pass"),
                                                        ("muon", 11, 8, 3, True, "events")])
def test_one_epoch_of_training_fed_by_a_list_and_by_a_device_store(hip, name, F, D, T, use_events, kind):
    """The same arrays through the same kernels in fixed summation orders: after every step the loss and all ten
    parameters are EQUAL between the two feeds; the first step's gradients against fp64 autograd through
    oracle.index_torch on the restated first window (the mean over all B x E_max entries, padded ones included)."""
    graphs = RAGGED[:6] if name == "ragged" else MUON
    assert len(graphs) == 6 and windows(5, 2) == [0, 2, 4]
    start, steps_l, kinds_l, grads_l = _epoch(graphs, False, F, D, T, use_events)
    start_s, steps_s, kinds_s, grads_s = _epoch(graphs, True, F, D, T, use_events)
    assert all(torch.equal(start[k], start_s[k]) for k in start)
    assert kinds_l == kinds_s == [kind] * 3
    for step, ((loss_l, params_l), (loss_s, params_s)) in enumerate(zip(steps_l, steps_s)):
        assert torch.equal(loss_l, loss_s), (step, loss_l.item(), loss_s.item())
        assert len(params_l) == 10 and all(torch.equal(a, c) for a, c in zip(params_l, params_s)), step
    want = assemble(graphs, 0, 2, "padded")
    p = {k: v.double().requires_grad_(True) for k, v in start.items()}
    e = index_torch.segment_classifier(want.X, want.src, want.dst, p, T)
    ref_loss = torch.nn.functional.binary_cross_entropy(e, torch.from_numpy(want.y).double())
    ref_loss.backward()
    assert abs(steps_l[0][0].item() - ref_loss.item()) < 1e-6
    assert set(grads_l) == set(p) and len(p) == 10
    for k in p:
        assert_grad_close(grads_l[k], p[k].grad, "batch assembly %s, list feed, %s" % (name, k))
        assert_grad_close(grads_s[k], p[k].grad, "batch assembly %s, store feed, %s" % (name, k))


def test_refusals_reach_no_kernel(hip):
    """Malformed graphs are refused on the host - by a device store before anything is uploaded or launched, by
    from_graphs also when it builds in pinned memory - and a valid window scores as the oracle says afterwards."""
    from gnn_fpga_amd.model import SegmentClassifier
    with hip.profile(64) as prof:
        for name in sorted(MALFORMED):
            graphs = [RAGGED[3], RAGGED[0], MALFORMED[name](RAGGED[4]), RAGGED[5]]
            with pytest.raises(ValueError, match=r"graph 2\b"):
                GraphStore(graphs, device="cuda")
            for layout in LAYOUTS:
                with pytest.raises(ValueError, match=r"graph 2\b"):
                    HitGraphBatch.from_graphs(graphs, pad_segments=layout == "padded", pin_memory=True)
                with pytest.raises(ValueError, match=r"graph 2\b"):
                    next(gnn_fpga_amd.batch_generator(graphs, n_samples=4, batch_size=4, layout=layout, device="cuda"))
        torch.cuda.synchronize()
    assert prof.records == []
    torch.manual_seed(2)
    m = SegmentClassifier(input_dim=3, hidden_dim=8, n_iters=2).cuda().eval()
    m.use_events = False
    params = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    batch, y = GraphStore(RAGGED, device="cuda").batch(2, 4, "flat")
    ref, _ = merge_graphs(RAGGED[2:6], "flat")
    with torch.no_grad():
        out = m(batch)
    want = index_c.segment_classifier(ref.X.numpy(), ref.src.numpy(), ref.dst.numpy(), params, 2)
    assert out.shape == (batch.n_segments,) and np.abs(out.cpu().numpy() - want).max() < TOL
