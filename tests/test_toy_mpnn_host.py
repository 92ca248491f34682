"""gnn_fpga_amd/toy_mpnn.py and include/gnn_hip_iter.h without a GPU: the module trees against the reference's fixtures,
the fp64 restatement the GPU tests lean on against the same fixtures, the numpy specification of the data cells, the
second ABI table, argument refusals, the route rule, and the power of the fixtures to see a mis-wired weight set."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import toy_mpnn_fp64 as ref
from gnn_fpga_amd import (HitGraphBatch, ToySegmentClassifier, ToySegmentClassifier2, _lib, build_toy_mpnn_graphs,
                          call_route as cr, synth, toy_mpnn)
from gnn_fpga_amd.hitgraph import _EventLayout

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_FIX = {}


def fixture(case):
    if case not in _FIX:
        _FIX[case] = ref.Fixture(case)
    return _FIX[case]


# ---- module trees ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.CASES)
def test_state_dict_equals_the_reference(case):
    fx = fixture(case)
    m = (ToySegmentClassifier2 if fx.shared else ToySegmentClassifier)(fx.F, fx.D, fx.T)
    sd = m.state_dict()
    assert list(sd) == fx.keys
    assert all(tuple(sd[k].shape) == fx.params[k].shape for k in fx.keys)
    assert sum(p.numel() for p in m.parameters()) == sum(v.size for v in fx.params.values())
    assert len(fx.keys) == (10 if fx.shared else 6 + 8 * fx.T)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in fx.params.items()})        # a checkpoint loads


def test_parameter_counts_of_the_notebook():
    assert toy_mpnn.SegmentClassifier is ToySegmentClassifier and toy_mpnn.SegmentClassifier2 is ToySegmentClassifier2
    m = ToySegmentClassifier(2, 32, 10)
    assert len(m.state_dict()) == 86 and sum(p.numel() for p in m.parameters()) == 68267
    assert [n for n, _ in m.named_children()] == ["input_network", "edge_networks", "node_networks", "output_network"]
    assert len(m.edge_networks) == len(m.node_networks) == 10
    m2 = ToySegmentClassifier2(2, 32, 10)
    assert len(m2.state_dict()) == 10 and sum(p.numel() for p in m2.parameters()) == 6689
    assert [n for n, _ in m2.named_children()] == ["input_network", "edge_network", "node_network"]
    for cls in (ToySegmentClassifier, ToySegmentClassifier2):
        assert cls().n_iters == 3 and cls().hidden_dim == 8 and cls().input_dim == 2
        with pytest.raises(NotImplementedError):
            cls(hidden_activation=nn.ReLU)


def test_no_cpu_path():
    g = synth.toy2d_graph(0)
    for cls in (ToySegmentClassifier, ToySegmentClassifier2):
        with torch.no_grad(), pytest.raises(RuntimeError):
            cls(2, 8, 1)(HitGraphBatch.from_graphs([g]))
    with pytest.raises(RuntimeError):
        build_toy_mpnn_graphs(torch.zeros(2, 40), torch.zeros(2, 40, dtype=torch.int64))


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.CASES)
def test_restatement_reproduces_the_fixture(case):
    fx = fixture(case)
    got = ref.run(fx.params, fx["X"], fx["src"], fx["dst"], fx["y"], fx.T)
    C = fx.F + fx.D
    for t in range(fx.T + 1):
        assert np.abs(got["e"][t] - fx["e64_%d" % t].reshape(-1)).max() <= 1e-12, t
    assert fx.h_passes() and fx.h_passes()[-1] == fx.T
    for t in fx.h_passes():
        assert np.abs(got["H"][t] - fx["H64_%d" % t].reshape(-1, C)).max() <= 1e-12, t
    assert abs(got["loss"] - float(fx["loss64"])) <= 1e-12
    for k in fx.keys:
        assert np.abs(got["grads"][k] - fx.grad64[k]).max() <= 1e-12, k
    # what the GPU tests compare with: the stored fp32 run is as far from fp64 as its ref_err_* says
    assert ref.rel_err(fx["scores"], fx["e64_%d" % fx.T]) == float(fx["ref_err_scores"])
    for k in fx.keys:
        assert ref.rel_err(fx["grad/" + k], fx.grad64[k]) == fx.ref_err_grad[k]


def test_fixture_files_stay_small():
    for f in os.listdir(ref.GOLDEN):
        assert os.path.getsize(os.path.join(ref.GOLDEN, f)) <= 1 << 20, f


def test_padded_case_pins_the_padding_rule():
    fx = fixture("f_unshared_f11_d8_t2_ragged")
    Ri, Ro, src, dst = fx["Ri"], fx["Ro"], fx["src"].reshape(fx.B, fx.E), fx["dst"].reshape(fx.B, fx.E)
    n_seg = (src >= 0).sum(axis=1)
    assert len(set(n_seg)) >= 4 and 1 in n_seg and 0 in n_seg                 # ragged, one segment, none
    assert np.array_equal(src < 0, Ro.sum(axis=1) == 0) and np.array_equal(src < 0, dst < 0)
    used = np.zeros((fx.B, fx.N), bool)
    for b in range(fx.B):
        used[b, src[b][src[b] >= 0] - b * fx.N] = used[b, dst[b][dst[b] >= 0] - b * fx.N] = True
    real = np.abs(fx["X"]).sum(axis=2) > 0
    assert (real & ~used).any(axis=1).sum() >= 3                              # isolated hits among the real ones
    # a padded segment scores sigmoid(W2 tanh(b1) + b2) of the network that scores it: pass t's, then output_network's
    p = fx.params
    for t, pre in enumerate(["edge_networks.0", "edge_networks.1", "output_network"]):
        z = np.tanh(p[pre + ".network.0.bias"].astype(np.float64))
        want = 1 / (1 + np.exp(-(p[pre + ".network.2.weight"].astype(np.float64) @ z + p[pre + ".network.2.bias"])))
        assert np.abs(fx["e64_%d" % t].reshape(fx.B, fx.E)[src < 0] - want).max() <= 1e-12


# ---- the data cells ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in ref.CASES if "ragged" not in c])
def test_specification_equals_the_notebook_cells(case):
    """synth.toy_mpnn_graphs_from_hits against what cells 8, 11 and 12 produced (kept in the fixture), element for
    element: X = [x, r], the np.where(d == 1) segment order, the labels."""
    fx = fixture(case)
    hit_x = fx["X"][:, :, 0]
    X, src, dst, y = synth.toy_mpnn_graphs_from_hits(hit_x, fx["hit_y"], det_r=np.arange(10.0))
    assert X.dtype == np.float32 and np.array_equal(X, fx["X"])
    off = (np.arange(fx.B) * fx.N)[:, None]
    assert np.array_equal((src[None] + off).reshape(-1), fx["src"]) and np.array_equal((dst[None] + off).reshape(-1), fx["dst"])
    assert y.dtype == np.float32 and np.array_equal(y, fx["y"])
    assert src.shape == (144,) and np.array_equal(src, np.sort(src))           # np.where's row-major order


def test_segment_order_of_other_shapes():
    src, dst = synth.toy_mpnn_segments(3, 2)
    assert src.tolist() == [0, 0, 1, 1, 2, 2, 3, 3] and dst.tolist() == [2, 3, 2, 3, 4, 5, 4, 5]
    lay = np.repeat(np.arange(5), 3)
    i, j = np.where(lay[None, :] - lay[:, None] == 1)                          # cell 11
    s, d = synth.toy_mpnn_segments(5, 3)
    assert np.array_equal(s, i) and np.array_equal(d, j)


# ---- the second ABI table ----------------------------------------------------------------------------------------------
def _declared():
    text = open(os.path.join(REPO, "include", "gnn_hip_iter.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gnn_iter_[a-z0-9_]+)\s*\(", text)))


def test_header_binding_and_library_export_the_same_names():
    names = _declared()
    assert len(names) == 7 and sorted(_lib.ITER_SIGNATURES) == names
    assert not set(_lib.ITER_SIGNATURES) & set(_lib.SIGNATURES)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), n
    src = open(os.path.join(REPO, "gnn-fpga_amd", "csrc", "iter_events.hip")).read()
    assert sorted(set(re.findall(r"^(?:int|size_t|int64_t) (gnn_iter_[a-z0-9_]+)\(", src, flags=re.M))) == names
    hdr = open(os.path.join(REPO, "include", "gnn_hip_iter.h")).read()
    assert int(re.search(r"#define GNN_ITER_MAX (\d+)", hdr).group(1)) == _lib.GNN_ITER_MAX == 16
    assert _lib.load().gnn_abi_version() == 7
    # every declaration cites the notebook cell it replaces
    for block in re.findall(r"/\*(.*?)\*/\s*(?:int|size_t|int64_t) gnn_iter_", hdr, flags=re.S):
        assert "cell" in block, block[:60]
    # the struct the kernels take by value is the one the binding fills
    assert ctypes.sizeof(_lib.GnnIterParams) == 2 * 8 + (2 * 16 + 1) * 4 * 8 + 4 * 4


def test_sizes_without_a_gpu():
    lib = _lib.load()
    assert lib.gnn_iter_grad_floats(2, 32, 10, 0) == 68267 and lib.gnn_iter_grad_floats(2, 32, 10, 1) == 6689
    assert lib.gnn_iter_grad_floats(11, 8, 0, 0) == 8 * 11 + 8 + (8 * 38 + 8 + 8 + 1)
    assert lib.gnn_iter_grad_floats(2, 32, 17, 0) == 0 and lib.gnn_iter_grad_floats(5, 7, 1, 0) == 0
    assert lib.gnn_iter_backward_workspace_bytes(32, 2, 32, 10) == 32 * 68267 * 4 + 256
    assert lib.gnn_iter_backward_workspace_bytes(0, 2, 32, 10) == 68267 * 4 + 256
    assert lib.gnn_iter_backward_workspace_bytes(-1, 2, 32, 10) == 0
    assert lib.gnn_iter_input_bwd_workspace_bytes(1025, 2, 32) == 2 * 96 * 4 + 256
    # the notebook's event fits both kernels at its width; LDS decides the rest
    assert _lib.iter_events_supported(2, 32, 40, 144, False) and _lib.iter_events_supported(2, 32, 40, 144, True)
    assert _lib.iter_events_supported(2, 32, 65, 150, False) and not _lib.iter_events_supported(2, 32, 65, 150, True)
    assert _lib.iter_events_supported(11, 8, 60, 300, True) and not _lib.iter_events_supported(3, 64, 8, 8, False)
    assert not _lib.iter_events_supported(2, 8, -1, 4, False) and not _lib.iter_events_supported(2, 8, 4, 1 << 30, False)


def _fake_params(F=2, D=8, T=2, shared=0):
    p = _lib.GnnIterParams()
    p.Win = p.bin = 0x1000                      # never read: every call below is refused before a launch
    for s in [p.out] + [p.edge[i] for i in range(min(T, 16))] + [p.node[i] for i in range(min(T, 16))]:
        s.Wa = s.ba = s.Wb = s.bb = 0x1000
    p.F, p.D, p.n_iters, p.shared = F, D, T, shared
    return p


def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    g = _lib.GnnGraph()
    g.n_hits, g.n_segments = 4, 3
    byref, fwd, bwd = ctypes.byref, lib.gnn_iter_forward_events, lib.gnn_iter_backward_events
    ok = _fake_params()

    def msg():
        return lib.gnn_last_error().decode()
    assert fwd(byref(g), None, 1, 1, 1, 4, 3, 1, None, None, None) == _lib.GNN_ERR_BADARG and "params" in msg()
    assert fwd(None, byref(ok), 1, 1, 1, 4, 3, 1, None, None, None) == _lib.GNN_ERR_BADARG
    assert fwd(byref(g), byref(_fake_params(T=17)), 1, 1, 1, 4, 3, 1, None, None, None) == _lib.GNN_ERR_BADARG
    assert "n_iters" in msg()
    assert fwd(byref(g), byref(_fake_params(F=5, D=7)), 1, 1, 1, 4, 3, 1, None, None, None) == _lib.GNN_ERR_UNSUPPORTED
    assert fwd(byref(g), byref(_fake_params(D=64, F=3)), 1, 1, 1, 4, 3, 1, None, None, None) == _lib.GNN_ERR_UNSUPPORTED
    missing = _fake_params()
    missing.node[1].Wb = None
    assert fwd(byref(g), byref(missing), 1, 1, 1, 4, 3, 1, None, None, None) == _lib.GNN_ERR_BADARG
    assert "iteration 1" in msg()
    own = _fake_params(shared=1)
    own.edge[1].Wa = 0x2000
    assert fwd(byref(g), byref(own), 1, 1, 1, 4, 3, 1, None, None, None) == _lib.GNN_ERR_BADARG and "shared" in msg()
    assert fwd(byref(g), byref(ok), None, 1, 1, 4, 3, 1, None, None, None) == _lib.GNN_ERR_BADARG      # offsets
    assert fwd(byref(g), byref(ok), 1, 1, 1, 4, 3, 1, None, None, None) == _lib.GNN_ERR_BADARG         # hit arrays NULL
    for k in ("X", "src", "dst", "in_ptr", "in_eid", "in_nbr", "out_ptr", "out_eid", "out_nbr"):
        setattr(g, k, 0x1000)
    assert fwd(byref(g), byref(ok), 1, 1, 1, 4, 3, None, None, None, None) == _lib.GNN_ERR_BADARG      # no output
    assert fwd(byref(g), byref(ok), 1, 1, 1, 4, 3, 1, 1, None, None) == _lib.GNN_ERR_BADARG            # e_all alone
    assert fwd(byref(g), byref(ok), 1, 1, 1, -4, 3, 1, None, None, None) == _lib.GNN_ERR_BADARG
    assert fwd(byref(g), byref(ok), 1, 1, 1, 5000, 3, 1, None, None, None) == _lib.GNN_ERR_UNSUPPORTED
    assert "do not fit" in msg()
    assert bwd(byref(g), byref(ok), 1, 1, 1, 4, 3, 1, 1, 1, None, 1, 1 << 20, None) == _lib.GNN_ERR_BADARG   # grads_flat
    assert bwd(byref(g), byref(ok), 1, 1, 1, 4, 3, None, 1, 1, 1, 1, 1 << 20, None) == _lib.GNN_ERR_BADARG   # e_all
    assert bwd(byref(g), byref(ok), 1, 1, 1, 5000, 3, 1, 1, 1, 1, 1, 1 << 20, None) == _lib.GNN_ERR_UNSUPPORTED
    assert bwd(byref(g), byref(ok), 1, 1, 1, 4, 3, 1, 1, 1, 1, 1, 16, None) == _lib.GNN_ERR_WORKSPACE
    assert bwd(byref(g), byref(ok), 1, 1, 1, 4, 3, 1, 1, 1, 1, None, 1 << 20, None) == _lib.GNN_ERR_WORKSPACE
    inb = lib.gnn_iter_input_bwd
    assert inb(None, 1, 12, 1, 12, 5, 2, 8, 1, 1, 1 << 20, None) == _lib.GNN_ERR_BADARG
    assert inb(1, 1, 4, 1, 12, 5, 2, 8, 1, 1, 1 << 20, None) == _lib.GNN_ERR_BADARG and "ldh" in msg()
    assert inb(1, 1, 12, 1, 12, 5, 2, 8, None, 1, 1 << 20, None) == _lib.GNN_ERR_BADARG
    assert inb(1, 1, 12, 1, 12, 5, 2, 8, 1, 1, 8, None) == _lib.GNN_ERR_WORKSPACE


def test_params_struct_refuses_what_the_kernels_would_misread():
    z = lambda *s: torch.zeros(*s)      # noqa: E731
    e, n = [z(8, 20), z(8), z(1, 8), z(1)], [z(8, 30), z(8), z(8, 8), z(8)]
    with pytest.raises(_lib.GnnHipError, match="ROCm device"):
        _lib.iter_params_struct(z(8, 2), z(8), [e], [n], e, 2, 8)
    with pytest.raises(_lib.GnnHipError, match="at most 16"):
        _lib.iter_params_struct(z(8, 2), z(8), [e] * 17, [n] * 17, e, 2, 8)
    with pytest.raises(_lib.GnnHipError, match="needs shape"):
        _lib.iter_params_struct(z(8, 3), z(8), [e], [n], e, 2, 8)


# ---- the route rule ----------------------------------------------------------------------------------------------------
def test_route_rule_table():
    lay = _EventLayout([0, 40], [0, 144])
    T = _lib.GNN_ITER_MAX
    rows = [((True, 1, lay, 10, True), "iter_events"),
            ((True, cr.EVENTS_MAX_GRAPHS, lay, T, True), "iter_events"),
            ((True, cr.EVENTS_MAX_GRAPHS + 1, lay, 10, True), "per_module"),      # too many graphs
            ((True, 0, lay, 10, True), "per_module"),                             # an empty batch
            ((False, 4, lay, 10, True), "per_module"),                            # use_events off
            ((True, 4, None, 10, True), "per_module"),                            # not block-diagonal
            ((True, 4, lay, T + 1, True), "per_module"),                          # more passes than the table holds
            ((True, 4, lay, 10, False), "per_module"),                            # the largest graph does not fit
            ((True, 4, lay, 0, True), "iter_events")]
    for args, want in rows:
        assert cr.choose_iter(*args) == want, args


class _Stub:
    def __init__(self, n_graphs, layout):
        self.n_graphs, self._layout, self.asked = n_graphs, layout, 0

    def event_layout(self):
        self.asked += 1
        return self._layout


def test_iter_route_asks_once_and_leaves_the_kind_on_the_model():
    m = ToySegmentClassifier(2, 32, 10)
    b = _Stub(4, _EventLayout([0, 40], [0, 144]))
    r = cr.iter_route(m, b, training=True)
    assert (r.kind, m._route.kind, b.asked) == ("iter_events", "iter_events", 1) and r.layout is b._layout
    assert m._route.batch is None and m._route.layout is None
    big = _Stub(4, _EventLayout([0, 65], [0, 150]))
    assert cr.iter_route(m, big, training=False).kind == "iter_events"            # the forward's LDS takes 65 hits
    r = cr.iter_route(m, big, training=True)                                      # the backward's does not
    assert (r.kind, r.layout, m._route.kind) == ("per_module", None, "per_module")
    m.use_events = False
    assert cr.iter_route(m, b, training=False).kind == "per_module" and b.asked == 1
    assert ToySegmentClassifier.use_events is True and ToySegmentClassifier2.use_events is True
    # the existing rules are as they were: the wide one-launch kernel stays opt-in through the new class only
    assert not _lib.events_preferred(2, 32, _EventLayout([0, 40], [0, 144]))


# ---- the power of the fixtures -----------------------------------------------------------------------------------------
FLOOR = 16 * 2.0 ** -24         # 16 fp32 ulp of a value near 1: the floor the parity bounds stand on


def _moved(fx, got):
    """Largest move of a checked tensor (every e_t, every stored H_t) in units of the 1e-5 bound."""
    C = fx.F + fx.D
    de = max(np.abs(got["e"][t] - fx["e64_%d" % t].reshape(-1)).max() for t in range(fx.T + 1))
    dh = max(np.abs(got["H"][t] - fx["H64_%d" % t].reshape(-1, C)).max() for t in fx.h_passes())
    return max(de, dh) / ref.SCORE_BOUND


@pytest.mark.parametrize("case", ["a_unshared_f2_d32_t10_b4", "b_unshared_f2_d8_t3_b3"])
def test_a_mis_wired_weight_set_moves_the_checked_tensors(case):
    fx = fixture(case)
    faults = [("swap", t) for t in range(fx.T)] + [("out_for_last",)]
    for f in faults:
        got = ref.run(fx.params, fx["X"], fx["src"], fx["dst"], None, fx.T, faults=(f,))
        moved = _moved(fx, got)
        print("  %s %-20s moves a checked tensor by %.1e x the bound" % (case[0], f, moved))
        assert moved * ref.SCORE_BOUND >= 1e4 * FLOOR, f           # (measured: at least 1e5 x the floor)
        # ... and a gradient of the sets involved leaves its bound
        full = ref.run(fx.params, fx["X"], fx["src"], fx["dst"], fx["y"], fx.T, faults=(f,))
        t = f[1] if f[0] == "swap" else fx.T - 1
        k = "edge_networks.%d.network.0.weight" % t
        assert ref.rel_err(full["grads"][k], fx.grad64[k]) > 10 * ref.grad_bound(fx.ref_err_grad[k]), (f, k)


@pytest.mark.parametrize("case", ["a_unshared_f2_d32_t10_b4", "b_unshared_f2_d8_t3_b3"])
def test_a_dropped_segment_moves_the_checked_tensors(case):
    fx = fixture(case)
    src, dst = fx["src"].copy(), fx["dst"].copy()
    j = fx.E + 17                                   # a segment of the second event: padded away
    src[j] = dst[j] = -1
    got = ref.run(fx.params, fx["X"], src, dst, None, fx.T)
    C = fx.F + fx.D
    d_h1 = np.abs(got["H"][1] - fx["H64_1"].reshape(-1, C)).max()
    others = np.arange(src.shape[0]) != j
    d_e = np.abs(got["e"][fx.T] - fx["e64_%d" % fx.T].reshape(-1))[others].max()
    print("  %s: H_1 moves by %.1e, the other segments' scores by %.1e" % (case[0], d_h1, d_e))
    assert d_h1 >= 1e4 * FLOOR and d_e >= 10 * ref.SCORE_BOUND


def test_the_shared_passes_header_rebuilds_its_three_units():
    """csrc/event_passes.h holds what k_event, k_event_bwd and the two per-iteration kernels share: it is in the Makefile's
    HDR, which every object depends on, and the three units include it."""
    csrc = os.path.join(REPO, "gnn-fpga_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "$(CSRC)/event_passes.h" in re.search(r"^HDR\s*:=\s*(.*)$", mk, re.M).group(1).split()
    assert re.search(r"^\$\(ROOT\)/build/%\.o: \$\(CSRC\)/%\.hip \$\(HDR\)$", mk, re.M)
    assert os.path.exists(os.path.join(csrc, "event_passes.h"))
    for unit in ("gnn_kernels", "backward", "iter_events"):
        assert re.search(r'^#include "event_passes\.h"$', open(os.path.join(csrc, unit + ".hip")).read(), re.M), unit


def test_the_shared_byte_counts_stay_wide():
    """The LDS byte counts are 64-bit sums: a segment count whose id words (6 per segment) pass 2^31 is refused, not
    wrapped into a few KB that fit."""
    assert _lib.events_supported(11, 8, 60, 300) and not _lib.events_supported(11, 8, 10, 613566757)
    assert not _lib.events_supported(3, 16, 10, 1 << 40) and not _lib.events_supported(3, 16, 1 << 40, 10)
