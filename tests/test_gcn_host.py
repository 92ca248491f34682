"""Host checks of the graph-convolution classifiers (gnn/GCN_Seg_Toy2D.ipynb, gnn/GCN_Toy2D.ipynb): the module tree
against the reference's fixtures, the fp64 restatement the GPU tests use, the seeded toy inputs, the C ABI's new entry
points and the build's resource remarks.  No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch

import gcn_fp64 as ref
import gnn_fpga_amd
from gnn_fpga_amd import _lib, synth
from gnn_fpga_amd.gcn import (GCNBinaryClassifier, GCRNBinaryClassifier, GraphConv, GraphConvSelfInt, SparseAdjacency,
                              compress_adjacency)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ref.fixture_names()
EXPECTED = {"seg_gcn_selfint_16x5_b4", "seg_gcn_graphconv_16x5_b2", "seg_gcn_selfint_32_64_32_b2",
            "hits_gcrn_selfint_8x12_b8", "hits_gcrn_graphconv_8_12_16_b3", "hits_gcrn_selfint_32_64x5_32_b2",
            "hits_kw_gcn_graphconv_8x3_b3", "hits_gcn_selfint_8_8_b1", "hits_gcn_8_b2"}


@pytest.fixture(scope="module")
def fixtures():
    return {c: ref.load_fixture(c) for c in CASES}


def package_model(d):
    cls = GCRNBinaryClassifier if d["kind"] == "gcrn" else GCNBinaryClassifier
    return ref.fixture_model(d, cls, gc_type=GraphConvSelfInt if d["conv"] == "selfint" else GraphConv)


def test_fixtures_present():
    assert EXPECTED <= set(CASES)


def test_fixtures_have_live_units(fixtures):
    """No fixture hides errors behind dead units: the logits span at least 0.05 and every graph-convolution layer of
    the kept activations has between 20 % and 90 % positive outputs."""
    for c, d in fixtures.items():
        assert float(d["logits64"].max() - d["logits64"].min()) >= 0.05, c
        for l in range(1, len(d["hidden_dims"])):
            if "h64_%d" % l in d:
                assert 0.2 <= float((d["h64_%d" % l] > 0).mean()) <= 0.9, (c, l)


@pytest.mark.parametrize("case", sorted(EXPECTED))
def test_module_tree_matches_the_reference(fixtures, case):
    d = fixtures[case]
    m = package_model(d)                                         # (load_state_dict is strict: the keys match)
    assert list(m.state_dict().keys()) == [str(k) for k in d["keys"]]
    for k, v in m.state_dict().items():
        assert tuple(v.shape) == d["param/" + k].shape, k
    kinds = {type(gc) for gc in m.gc_layers}
    assert kinds <= {GraphConvSelfInt if d["conv"] == "selfint" else GraphConv}
    assert [n for n, _ in m.named_children()] == ["feature_extractor", "gc_layers", "classifier"]


def test_notebook_configuration_parameter_count():
    m = GCNBinaryClassifier(5, [16] * 5)
    assert sum(p.numel() for p in m.parameters()) == 2225
    keys = list(m.state_dict())
    assert keys[:2] == ["feature_extractor.weight", "feature_extractor.bias"]
    assert keys[2:5] == ["gc_layers.0.node_mod.weight", "gc_layers.0.node_mod.bias", "gc_layers.0.neighbor_mod.weight"]
    assert keys[-2:] == ["classifier.weight", "classifier.bias"]
    g = GCRNBinaryClassifier(3, [8] * 12, gc_type=GraphConv)
    assert list(g.state_dict())[2:4] == ["gc_layers.0.linear.weight", "gc_layers.0.linear.bias"]
    assert g.gc_layers[0].linear.weight.shape == (8, 11)


def test_exports():
    for n in ("GraphConv", "GraphConvSelfInt", "GCNBinaryClassifier", "GCRNBinaryClassifier", "SparseAdjacency",
              "compress_adjacency"):
        assert hasattr(gnn_fpga_amd, n), n
    from gnn_fpga_amd import model
    assert model.GCNBinaryClassifier is GCNBinaryClassifier and model.GCRNBinaryClassifier is GCRNBinaryClassifier


@pytest.mark.parametrize("case", sorted(EXPECTED))
def test_fp64_restatement_reproduces_the_reference(fixtures, case):
    d = fixtures[case]
    r = ref.run(ref.fixture_model(d), d["X"], d["A"], d["y"], torch.float64)
    assert ref.rel_err(r["logits"], d["logits64"]) <= 1e-12
    assert abs(r["loss"] - float(d["loss64"])) <= 1e-12 * abs(float(d["loss64"]))
    for k in d["keys"]:
        assert ref.rel_err(r["grads"][str(k)], d["grad64/" + str(k)]) <= 1e-12, k
    for l in range(len(d["hidden_dims"])):
        if "h64_%d" % l in d:
            assert ref.rel_err(r["h"][l], d["h64_%d" % l]) <= 1e-12, l


@pytest.mark.parametrize("case", sorted(EXPECTED))
def test_fp32_restatement_within_the_reference_error(fixtures, case):
    """The fp32 restatement is as far from fp64 as the reference's fp32 run was (the bound the GPU tests use)."""
    d = fixtures[case]
    r = ref.run(ref.fixture_model(d), d["X"], d["A"], d["y"], torch.float32)
    assert ref.rel_err(r["logits"], d["logits64"]) <= ref.bound(d["ref_err_logits"])
    assert ref.rel_err(r["logits"], d["logits"]) <= max(float(d["ref_err_logits"]), ref.ULP16)


def test_bound_floor():
    assert ref.bound(0.0) == pytest.approx(9.5367e-7, rel=1e-3) and ref.bound(1e-6) == 4e-6


def test_toy_segment_graphs():
    X, A, y = synth.toy_segment_graphs(3, seed=4)
    assert X.shape == (3, 225, 5) and A.shape == (3, 225, 225) and y.shape == (3, 225)
    assert X.dtype == A.dtype == y.dtype == np.float32
    assert int((A != 0).sum(axis=-1).max()) <= 10 and int((A != 0).sum(axis=-2).max()) <= 10
    assert np.isfinite(A).all() and A.max() <= 1.0 and A.min() >= 0.0
    assert set(np.unique(y)) <= {0.0, 1.0} and y.sum(axis=1).tolist() == [45.0] * 3     # 5 tracks x 9 true segments
    np.testing.assert_array_equal(X[:, :, 4], (X[:, :, 1] - X[:, :, 0]) / (X[:, :, 3] - X[:, :, 2]))
    # a true segment pair (same track, consecutive) has equal slopes: weight ~1
    X2, A2, y2 = synth.toy_segment_graphs(3, seed=4)
    np.testing.assert_array_equal(A, A2)


def test_segment_adjacency_is_the_triple_loop():
    """Cell 12 of the segment notebook, spelled out on one small event, against the index comparison."""
    X, A, y = synth.toy_segment_graphs(1, seed=2, n_tracks=2)
    T, L = 2, 10
    S = T * T * (L - 1)
    assert A.shape == (1, S, S)
    seg = [(l * T + a, (l + 1) * T + b) for l in range(L - 1) for a in range(T) for b in range(T)]
    adj = np.zeros((S, S), bool)
    for i in range(S):
        for j in range(i, S):
            if seg[i][1] == seg[j][0]:
                adj[i, j] = adj[j, i] = True
    slope = X[0, :, 4]
    kern = np.exp(-((slope[None, :] - slope[:, None]) ** 2) / np.float32(2 * 0.01 ** 2))
    np.testing.assert_array_equal(A[0], np.where(adj, kern, 0).astype(np.float32))


def test_toy_hit_graphs():
    for norm in (None, "row", "kw"):
        X, A, y = synth.toy_hit_graphs(16, seed=3, norm=norm)
        assert X.shape == (16, 40, 3) and A.shape == (16, 40, 40) and y.shape == (16, 40)
        assert np.isfinite(A).all()
        if norm is None:
            assert set(np.unique(A)) <= {0.0, 1.0} and np.array_equal(A, A.transpose(0, 2, 1))
        if norm == "row":
            s = A.sum(axis=-1)
            assert np.all((np.abs(s - 1) < 1e-6) | (s == 0))                 # a hit with no neighbour: a zero row
            assert not np.array_equal(A, A.transpose(0, 2, 1))               # the "row" norm is not symmetric
            assert np.array_equal(A != 0, (A != 0).transpose(0, 2, 1))
        if norm == "kw":
            assert np.all(np.diagonal(A, axis1=1, axis2=2) > 0)
            np.testing.assert_allclose(A, A.transpose(0, 2, 1), rtol=1e-6)
    assert y.sum(axis=1).tolist() == [10.0] * 16                             # track 0 has one hit per layer
    assert np.array_equal(X[:, :12, 2], y[:, :12]) and not X[:, 12:, 2].any()
    with pytest.raises(ValueError):
        synth.toy_hit_graphs(1, norm="col")


def test_cpu_tensors_raise():
    X, A, y = synth.toy_hit_graphs(2, seed=0)
    m = GCRNBinaryClassifier(3, [8, 8])
    with pytest.raises(RuntimeError):
        m(torch.from_numpy(X), torch.from_numpy(A))
    with torch.no_grad(), pytest.raises(RuntimeError):
        m.eval()(torch.from_numpy(X), torch.from_numpy(A))
    with pytest.raises(RuntimeError):
        compress_adjacency(torch.from_numpy(A))
    with pytest.raises(RuntimeError):
        GraphConvSelfInt(3, 4)(torch.from_numpy(X), torch.from_numpy(A))
    with pytest.raises(TypeError):
        GCNBinaryClassifier(3, [8, 8], gc_type=torch.nn.Linear)


def test_sparse_adjacency_slices_are_views():
    B, N, W = 6, 5, 3
    z = lambda *s: torch.zeros(*s, dtype=torch.int32)                        # noqa: E731
    adj = SparseAdjacency(z(B, N), z(B, N, W), z(B, N, W).float(), z(B, N), z(B, N, W), z(B, N, W).float())
    assert len(adj) == 6 and adj.n_nodes == 5 and adj.width == 3 and adj.shape == (6, 5, 5)
    s = adj[2:4]
    assert len(s) == 2 and s.width == 3
    assert s.row_idx.data_ptr() == adj.row_idx[2].data_ptr() and s.row_idx.is_contiguous()
    assert s.col_val.data_ptr() == adj.col_val[2].data_ptr()
    assert len(adj[4:100]) == 2
    with pytest.raises(TypeError):
        adj[0]
    with pytest.raises(TypeError):
        adj[::2]


def test_new_entry_points_and_abi():
    lib = _lib.load()
    hdr = open(os.path.join(REPO, "include", "gnn_hip.h")).read()
    names = ("gnn_gcn_supported", "gnn_gcn_compress_count", "gnn_gcn_compress_fill", "gnn_gcn_forward",
             "gnn_gcn_backward_workspace_bytes", "gnn_gcn_backward")
    for n in names:
        assert re.search(r"\b%s\(" % n, hdr) and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert lib.gnn_abi_version() == 7 and _lib.GNN_ABI_VERSION == 7 and "#define GNN_ABI_VERSION 7" in hdr
    assert "GCN_Seg_Toy2D.ipynb cell 20" in hdr and "GCN_Toy2D.ipynb cell 11" in hdr and "cell 14" in hdr
    assert "#define GNN_GCN_MAX_LAYERS %d" % _lib.GNN_GCN_MAX_LAYERS in hdr
    bad = _lib.GNN_ERR_BADARG
    assert lib.gnn_gcn_forward(None, None, None, None, None, None) == bad
    assert lib.gnn_gcn_backward(None, None, None, None, None, None, None, 0, None) == bad
    assert lib.gnn_gcn_compress_count(None, 1, 0, None, None, None, None) == bad
    assert lib.gnn_gcn_compress_fill(None, 1, 4, 0, None, None, None, None, None) == bad
    assert b"gcn" in lib.gnn_last_error()
    assert lib.gnn_gcn_backward_workspace_bytes(32, 2225) >= 32 * 2225 * 4


def test_supported_shapes():
    ok = _lib.gcn_supported
    assert ok(225, 5, 16, 10) and ok(40, 3, 8, 40)                           # the two notebook configurations
    assert ok(40, 3, 64, 40) and ok(225, 5, 64, 10)                          # the wide ones
    assert ok(1, 3, 8, 1) and ok(257, 3, 64, 257) and ok(65, 3, 12, 65)
    assert not ok(600, 3, 64, 10)
    msg = _lib.load().gnn_last_error().decode()
    assert "LDS" in msg and "163840" in msg
    with pytest.raises(RuntimeError, match="163840"):
        _lib.gcn_require(600, 3, 64, 10)
    assert not ok(40, 3, 512, 10) and "256" in _lib.load().gnn_last_error().decode()
    assert not ok(0, 3, 8, 0) and not ok(40, 0, 8, 4) and not ok(40, 3, 8, 41)


def test_net_struct_offsets_follow_the_parameter_order(monkeypatch):
    """The flat gradient the backward writes is cut by numel in module parameter order (autograd._Gcn.backward)."""
    from gnn_fpga_amd import autograd
    for m in (GCNBinaryClassifier(5, [16] * 5), GCRNBinaryClassifier(3, [8, 12, 16], gc_type=GraphConv),
              GCNBinaryClassifier(3, [8])):
        names = [n for n, _ in m.named_parameters()]
        params = [p.detach() for p in m.parameters()]
        # (the struct needs device pointers; the offsets are checked on a stand-in that records them)
        offs, off = {}, 0
        for n, p in zip(names, params):
            offs[n], off = off, off + p.numel()
        monkeypatch.setattr(_lib, "_dev", lambda t, dtype, what: 1)
        s = autograd._gcn_net(m, params)
        assert s.n_params == off == sum(p.numel() for p in params)
        assert (s.off_f, s.off_bf) == (offs["feature_extractor.weight"], offs["feature_extractor.bias"])
        assert (s.off_c, s.off_bc) == (offs["classifier.weight"], offs["classifier.bias"])
        for l, gc in enumerate(m.gc_layers):
            if isinstance(gc, GraphConvSelfInt):
                assert s.off_n[l] == offs["gc_layers.%d.node_mod.weight" % l]
                assert s.off_b[l] == offs["gc_layers.%d.node_mod.bias" % l]
                assert s.off_g[l] == offs["gc_layers.%d.neighbor_mod.weight" % l]
            else:
                assert s.off_g[l] == offs["gc_layers.%d.linear.weight" % l]
                assert s.off_b[l] == offs["gc_layers.%d.linear.bias" % l]
        assert list(s.dims[:s.n_dims]) == m.hidden_dims and s.max_width == max(m.hidden_dims)
    deep = GCNBinaryClassifier(3, [4] * 18)
    with pytest.raises(RuntimeError, match="at most 16"):
        autograd._gcn_net(deep, [p.detach() for p in deep.parameters()])


def test_gcn_is_a_build_unit():
    mk = open(os.path.join(REPO, "gnn-fpga_amd", "csrc", "Makefile")).read()
    units = re.search(r"^UNITS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    assert "gcn" in units and os.path.exists(os.path.join(REPO, "gnn-fpga_amd", "csrc", "gcn.hip"))


def test_kernel_resource_remarks():
    path = os.path.join(REPO, "build", "gcn.remarks")
    if not os.path.exists(path):
        pytest.fail("build/gcn.remarks is missing: build the library first")
    txt = open(path).read()
    kernels = set(re.findall(r"Function Name: \S*?(k_gcn_[a-z]+)", txt))
    assert {"k_gcn_rows", "k_gcn_cols", "k_gcn_fwd", "k_gcn_bwd", "k_gcn_reduce"} <= kernels, kernels
    # the one-launch kernels keep their working set in registers and LDS: no scratch
    for blk in txt.split("Function Name: ")[1:]:
        if "k_gcn_" in blk.split("\n", 1)[0]:
            assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", blk), blk.split("\n", 1)[0]
