"""The reference's own training harness holding the drop-in, pinned by what that harness did with it
(tests/golden/estimator/, written by oracle/gen_golden.py --only-estimator, which runs gnn/estimator.py and
gnn/estimator_maskedlinear.py UNMODIFIED on the drop-in).  gnn/estimator.py:22-47 (constructor: optimizer over
model.parameters(), printed parameter count), :54-55 (the weight lists its L1 penalty walks), :62-78 (checkpoint
save / load of state_dict + optimizer).  The forward itself needs a GPU (no CPU path): on CPU tensors the step
must fail loudly, not fall back."""
import io
import os

import numpy as np
import pytest
import torch

from golden_util import GOLDEN

EST = os.path.join(GOLDEN, "estimator")


def _prefixed(d, prefix):
    return {k[len(prefix):]: torch.from_numpy(d[k]) for k in d.files if k.startswith(prefix)}


def test_reference_estimator_holds_the_dropin(tmp_path):
    from gnn_fpga_amd import HitGraphBatch, synth
    from gnn_fpga_amd._lib import GnnHipError
    from gnn_fpga_amd.model import SegmentClassifier
    fx = np.load(os.path.join(EST, "ref_estimator_d8.npz"))
    torch.manual_seed(0)
    m = SegmentClassifier(input_dim=3, hidden_dim=8, n_iters=2)
    # what the reference's constructor printed and built around the drop-in: "Parameters: 569" (the notebooks'
    # count, F=3, D=8) and an optimizer over all ten tensors
    assert int(fx["printed_parameters"]) == 569 == sum(p.numel() for p in m.parameters())
    assert int(fx["optimizer_params"]) == 10 == len(list(m.parameters()))
    opt = torch.optim.Adam(m.parameters())
    # the lists training_step builds for its L1 penalty (estimator.py:54-55)
    node_w = [l.weight for l in m.node_network.network if hasattr(l, "weight")]
    edge_w = [l.weight for l in m.edge_network.network if hasattr(l, "weight")]
    assert [tuple(w.shape) for w in node_w] == [(8, 33), (8, 8)]
    assert [tuple(w.shape) for w in edge_w] == [(8, 22), (1, 8)]
    # same state_dict keys / shapes as the reference's own model
    ref_sd = _prefixed(fx, "sd/")
    assert {k: tuple(v.shape) for k, v in ref_sd.items()} == {k: tuple(v.shape) for k, v in m.state_dict().items()}
    # a checkpoint the reference's save_checkpoint wrote (its model + the optimizer it built around the drop-in)
    # loads the way its load_checkpoint loads it (estimator.py:73-78)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(1.0)
    ck = torch.load(os.path.join(EST, "checkpoint.pt"), weights_only=True)
    m.load_state_dict(ck["state_dict"])
    opt.load_state_dict(ck["optimizer"])
    for k, v in ref_sd.items():
        assert torch.equal(m.state_dict()[k], v), k
    assert ck["train_losses"] == [0.6] and ck["valid_losses"] == [0.5]
    # and the drop-in's own state round-trips through the same checkpoint layout
    fn = str(tmp_path / "checkpoint.pt")
    torch.save({"epoch": 1, "state_dict": m.state_dict(), "optimizer": opt.state_dict()}, fn)
    torch.manual_seed(5)
    again = SegmentClassifier(input_dim=3, hidden_dim=8, n_iters=2)
    again.load_state_dict(torch.load(fn, weights_only=True)["state_dict"])
    assert all(torch.equal(a, b) for a, b in zip(m.parameters(), again.parameters()))
    # no CPU path: the step raises instead of silently computing somewhere else
    g = synth.layered_graph(30, 60, 3, seed=0)
    X, Ri, Ro = (torch.from_numpy(a)[None] for a in synth.to_dense(g))
    with pytest.raises(GnnHipError):
        m([X, Ri, Ro])
    with pytest.raises(GnnHipError):
        m(HitGraphBatch.from_graphs([g]))


def test_reference_pruning_estimator_deep_copies_and_reloads_the_dropin():
    """gnn/estimator_maskedlinear.py:82-101 `load_weights` (the pruning notebooks' retraining step) deep-copies the
    model, loads a checkpoint into the copy and assigns `weight.data = W * mask` layer by layer.  The drop-in must
    survive that AFTER it has run a forward - its caches then hold a ctypes struct of device pointers, which neither
    pickles nor deep-copies (simulated here: the test needs no GPU) - and must see the replaced `.data`.  The
    weights that load_weights left in this drop-in are the fixture's `after/`."""
    import copy
    from gnn_fpga_amd import _lib
    from gnn_fpga_amd.model import SegmentClassifier
    fx = np.load(os.path.join(EST, "ref_load_weights_d8.npz"))
    D = 8
    me = [torch.from_numpy(fx["me0"]), torch.from_numpy(fx["me1"])]
    mn = [torch.from_numpy(fx["mn0"]), torch.from_numpy(fx["mn1"])]
    torch.manual_seed(1)
    m = SegmentClassifier(input_dim=3, hidden_dim=D, n_iters=2, masks_e=me, masks_n=mn)
    layers = {"edge_network.network.0": m.edge_network.network[0], "edge_network.network.2": m.edge_network.network[2],
              "node_network.network.0": m.node_network.network[0], "node_network.network.2": m.node_network.network[2]}
    assert all(hasattr(l, "mask_flag") and hasattr(l, "mask") for l in layers.values())   # what load_weights reads
    # what a forward on the GPU leaves behind
    key = m._param_key()
    m._w_cache = (key, [p.detach() for p in m.parameters()], _lib.GnnParams(), D, None)
    m._xp_cache = (key, 0)
    c = copy.deepcopy(m)
    assert c._w_cache is None and c._xp_cache is None and m._w_cache is not None
    assert all(torch.equal(a, b) and a.data_ptr() != b.data_ptr() for a, b in zip(m.parameters(), c.parameters()))
    # the copy takes the dense checkpoint; the masked layers of the model take the copy's weights times their masks
    dense, after = _prefixed(fx, "dense/"), _prefixed(fx, "after/")
    c.load_state_dict(dense)
    for name, layer in layers.items():
        w = getattr(c, name.split(".")[0]).network[int(name[-1])].weight.data
        layer.weight.data = w * layer.mask.data if layer.mask_flag else w
        assert torch.equal(layer.weight.data, after[name + ".weight"]), name     # what load_weights left
    assert m._param_key() != key                      # the replaced .data is seen: the cached weights are rebuilt
    # torch.save(model) / torch.load of the whole module, as notebooks do, drops the caches too
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    again = torch.load(buf, weights_only=False)       # (a file this test wrote itself)
    assert again._w_cache is None and all(torch.equal(a, b) for a, b in zip(m.parameters(), again.parameters()))
