"""Host checks of the hit classifier (gnn/MPNN_HitClassifier.ipynb): the drop-in module tree against the
reference's fixtures, the new C ABI entry points and shapes, the fp64 restatement the GPU tests use, and the
synthetic samples.  No GPU needed."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import nodeclf_fp64 as ref64
from gnn_fpga_amd import HitGraphBatch, _lib, synth
from gnn_fpga_amd.model import NodeClassifier

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "node_classifier")
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, "*.npz")))


def test_fixtures_present():
    assert {"d8_t0_b2", "d8_t1_b4", "d16_t3_b8", "d64_t7_b32", "d8_t2_b4_l1", "d8_t2_b6_padded"} <= set(CASES)


@pytest.mark.parametrize("case", CASES)
def test_module_tree_matches_the_reference(case):
    fx = ref64.fixture(os.path.join(GOLD, case + ".npz"))
    D, T = int(fx["hidden_dim"]), int(fx["n_iters"])
    m = NodeClassifier(input_dim=4, hidden_dim=D, n_iters=T)
    assert list(m.state_dict().keys()) == list(fx["keys"]) == ref64.KEYS
    for k, v in m.state_dict().items():
        assert tuple(v.shape) == fx["params"][k].shape, k
    m.load_state_dict({k: torch.from_numpy(v) for k, v in fx["params"].items()})
    # the lists gnn/estimator.py training_step builds for its l1 term
    node_w = [l.weight for l in m.node_network.network if hasattr(l, "weight")]
    edge_w = [l.weight for l in m.edge_network.network if hasattr(l, "weight")]
    assert [list(w.shape) for w in node_w] == fx["node_weight_shapes"].tolist()
    assert [list(w.shape) for w in edge_w] == fx["edge_weight_shapes"].tolist()


def test_notebook_configuration_parameter_count():
    m = NodeClassifier(input_dim=4, hidden_dim=64, n_iters=7)
    assert sum(p.numel() for p in m.parameters()) == 26502
    assert len(m.state_dict()) == 12


def test_cpu_tensors_raise():
    s = synth.hit_classifier_samples(2, seed=0)
    m = NodeClassifier(input_dim=4, hidden_dim=8, n_iters=1)
    dense = [torch.from_numpy(s.X), torch.from_numpy(s.Ri.astype(np.float32)), torch.from_numpy(s.Ro.astype(np.float32))]
    with torch.no_grad(), pytest.raises(RuntimeError):
        m(dense)
    with pytest.raises(RuntimeError):                                    # training forward too
        m(HitGraphBatch.from_dense(*dense))


def test_new_entry_points_and_shapes():
    lib = _lib.load()
    for name in ("gnn_nodeclf_forward", "gnn_nodeclf_forward_train", "gnn_nodeclf_backward"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    for D in (8, 16, 32, 64):
        assert lib.gnn_shape_supported(4, D) == 1
        assert lib.gnn_h_stride(4, D) == 4 + D                           # C == LDH: no pad column
    assert lib.gnn_abi_version() == 7
    g, p, gr = _lib.GnnGraph(), _lib.GnnParams(), _lib.GnnGrads()
    p.F, p.D = 4, 8
    bad = _lib.GNN_ERR_BADARG
    assert lib.gnn_nodeclf_forward(None, ctypes.byref(p), None, None, 1, None, None, None, 0, None) == bad
    assert lib.gnn_nodeclf_forward(ctypes.byref(g), ctypes.byref(p), None, None, 1, None, None, None, 0, None) == bad
    assert lib.gnn_nodeclf_forward_train(ctypes.byref(g), None, None, None, 1, None, None, None, None, None, 0,
                                         None) == bad
    assert lib.gnn_nodeclf_backward(ctypes.byref(g), ctypes.byref(p), None, None, 1, None, None, None, None, None,
                                    ctypes.byref(gr), None, None, None, 0, None) == bad
    assert b"nodeclf" in lib.gnn_last_error()


@pytest.mark.parametrize("case", CASES)
def test_fp64_restatement_reproduces_the_reference(case):
    fx = ref64.fixture(os.path.join(GOLD, case + ".npz"))
    B, N, T = int(fx["B"]), int(fx["N"]), int(fx["n_iters"])
    y, H = ref64.forward(fx["X"], fx["src"], fx["dst"], fx["params"], T)
    assert np.abs(y.reshape(B, N) - fx["scores"]).max() < 2e-6
    D = int(fx["hidden_dim"])
    for t in range(1, T + 1):
        if "H%d" % t in fx:
            assert np.abs(H[t, :, :D].reshape(B, N, D) - fx["H%d" % t]).max() < 2e-6
    loss, grads, _ = ref64.training_step(fx["X"], fx["src"], fx["dst"], fx["params"], T, fx["y"], float(fx["l1"]))
    assert abs(loss - float(fx["loss"])) < 1e-5
    for k in ref64.KEYS:
        r = fx["grads"][k]
        assert np.abs(grads[k] - r).max() <= 1e-6 + 1e-4 * np.abs(r).max(), k


def test_synthetic_samples_have_the_notebook_structure():
    s = synth.hit_classifier_samples(5, seed=3)
    assert s.X.shape == (5, 50, 4) and s.X.dtype == np.float32
    assert s.Ri.shape == s.Ro.shape == (5, 50, 225) and s.y.shape == (5, 50)
    layers = np.repeat(np.arange(10), 5)
    assert np.all(layers[s.dst] - layers[s.src] == 1)                    # Ro = inner hit, Ri = outer hit
    adj = np.stack(np.where((layers[None, :] - layers[:, None]) == 1), axis=1)
    assert np.array_equal(adj[:, 0], s.src) and np.array_equal(adj[:, 1], s.dst)
    assert np.all(s.Ri.sum(axis=1) == 1) and np.all(s.Ro.sum(axis=1) == 1)
    assert np.all(s.y.reshape(5, 10, 5).sum(axis=2) == 1)                # one true hit per layer
    seed = layers < 3
    assert np.array_equal(s.X[:, seed, 3], s.y[:, seed]) and np.all(s.X[:, ~seed, 3] == 0)
    assert np.all(s.X[:, 0, 1] == 0)                                     # phi centred on the first true hit
    b = synth.hit_classifier_samples(5, seed=3)
    assert np.array_equal(s.X, b.X) and np.array_equal(s.y, b.y)
