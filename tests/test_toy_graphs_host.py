"""Host checks of the toy graph builders (csrc/toy_graphs.hip, gnn_fpga_amd/toy_graphs.py): the numpy specification in
synth.py against the reference notebooks' own cells (tests/golden/toy_graphs, tools/gen_toy_graphs_golden.py), the
new entry points, and the argument checks.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import toy_graphs_fixtures as fx
import gnn_fpga_amd
from gnn_fpga_amd import _lib, synth, toy_graphs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MIN = np.finfo(np.float32).tiny


@pytest.mark.parametrize("shape", fx.SHAPES)
def test_segment_specification_equals_the_notebook(shape):
    """X, y and A bit for bit: the fixture is numpy and so is the specification."""
    d = fx.load("seg_" + shape)
    X, A, y = synth.toy_segment_graphs_from_hits(d["hit_x"], d["hit_y"], det_r=d["det_r"], sigma=float(d["sigma"]))
    assert fx.same_bits(X, d["X"]) and fx.same_bits(y, d["y"])
    assert fx.same_bits(A, fx.dense(d))
    L, T = d["det_r"].shape[0], d["hit_x"].shape[1] // d["det_r"].shape[0]
    assert A.shape[1] == T * T * (L - 1) and int((A != 0).sum(axis=2).max(initial=0)) <= 2 * T
    # the structural entries are the index relation the kernel uses: (l, a, b) touches (l - 1, *, a) and (l + 1, b, *)
    s = np.arange(A.shape[1])
    l, a, b = s // (T * T), (s // T) % T, s % T
    touch = (l[:, None] + 1 == l[None, :]) & (b[:, None] == a[None, :])
    touch = touch | touch.T
    got = np.zeros(A.shape, bool)
    got[d["A_batch"], d["A_rows"], d["A_cols"]] = True
    assert np.array_equal(got, np.broadcast_to(touch, A.shape))


def test_segment_edge_fixture_holds_every_class_of_entry():
    v = fx.load("seg_edge")["A_vals"]
    assert (v >= FLT_MIN).any() and ((v > 0) & (v < FLT_MIN)).any() and (v == 0).any()
    x = fx.load("seg_edge")["hit_x"].reshape(-1, 10, 5)
    assert (np.diff(x, axis=-1) == 0).any()                                  # a tie within a layer
    assert (x == 0).any() and (x == np.nextafter(np.float32(1), np.float32(0))).any() and (x == np.float32(1e-30)).any()


@pytest.mark.parametrize("norm", fx.NORMS)
@pytest.mark.parametrize("shape", fx.SHAPES)
def test_hit_specification_equals_the_notebook(shape, norm):
    """X, y0 and A bit for bit for all three norms; the fixture's A has the notebook's NaN rows zeroed (iso_rows)."""
    d = fx.load("hits_" + shape)
    X, A, y0 = synth.toy_hit_graphs_from_hits(d["hit_x"], d["hit_y"], det_r=d["det_r"], seed_size=int(d["seed_size"]),
                                              norm=norm)
    assert fx.same_bits(X, d["X"]) and fx.same_bits(y0, d["y0"])
    assert fx.same_bits(A, fx.dense(d, norm or "none"))
    if norm == "row":
        assert not A[d["iso_batch"], d["iso_rows"]].any()


def test_hit_edge_fixture_has_isolated_hits_and_a_tie():
    d = fx.load("hits_edge")
    assert d["iso_rows"].shape[0] > 0
    assert (np.diff(d["hit_x"].reshape(-1, 10, 4), axis=-1) == 0).any()
    a = fx.dense(d, "none")
    assert not np.array_equal(a, a.transpose(0, 2, 1))                       # a[i, j] and a[j, i] do round differently


def test_from_hits_form_is_what_toy_hit_graphs_returns():
    tracks = synth.toy_tracks(5, 4, seed=3).astype(np.float64).transpose(0, 2, 1)
    order = np.argsort(tracks, axis=-1)
    x = np.take_along_axis(tracks, order, axis=-1).reshape(5, -1)
    for norm in fx.NORMS:
        want = synth.toy_hit_graphs(5, seed=3, norm=norm)
        got = synth.toy_hit_graphs_from_hits(x, order.reshape(5, -1), norm=norm)
        assert all(fx.same_bits(g, w) for g, w in zip(got, want))
    assert synth.toy_hit_graphs_from_hits(x, order.reshape(5, -1), target=2)[2].sum() == 50.0


def test_new_entry_points_are_declared_bound_and_exported():
    lib = _lib.load()
    hdr = open(os.path.join(REPO, "include", "gnn_hip.h")).read()
    for n in ("gnn_toy_graphs_list_width", "gnn_toy_segment_graphs", "gnn_toy_hit_graphs"):
        assert re.search(r"\b%s\(" % n, hdr) and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert lib.gnn_abi_version() == 7 and "#define GNN_ABI_VERSION 7" in hdr
    assert "GCN_Seg_Toy2D.ipynb (cells 10-17 and 24" in hdr and "GCN_Toy2D.ipynb (cells 8 and 17" in hdr
    for n in ("sort_toy_tracks", "build_toy_segment_graphs", "build_toy_hit_graphs", "ToySegmentGraphs", "ToyHitGraphs"):
        assert getattr(gnn_fpga_amd, n) is getattr(toy_graphs, n)
    mk = open(os.path.join(REPO, "gnn-fpga_amd", "csrc", "Makefile")).read()
    assert "toy_graphs" in re.search(r"^UNITS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    assert "cells 10-17 and 24" in toy_graphs.build_toy_segment_graphs.__doc__
    assert "cells 8 and 17" in toy_graphs.build_toy_hit_graphs.__doc__


def test_list_widths_and_shape_limits():
    w = _lib.toy_list_width
    S, H = _lib.GNN_TOY_SEGMENTS, _lib.GNN_TOY_HITS
    assert w(S, 10, 5) == 10 and w(H, 10, 4) == 8 and w(H, 10, 4, "row") == 8 and w(H, 10, 4, "kw") == 9
    assert w(S, 3, 2) == 4 and w(H, 3, 2, "kw") == 5
    assert w(S, 2, 1) == 1 and w(H, 2, 1) == 2 and w(H, 2, 1, "kw") == 2    # never wider than a row
    with pytest.raises(RuntimeError, match="1 to 16 tracks"):
        w(S, 10, 17)
    with pytest.raises(RuntimeError, match="at least 2 detector layers"):
        w(H, 1, 4)
    with pytest.raises(RuntimeError, match="at most 4096"):
        w(S, 18, 16)
    with pytest.raises(RuntimeError, match="at most 4096"):
        w(H, 300, 14)


def test_bad_arguments_through_the_c_abi():
    lib, bad = _lib.load(), _lib.GNN_ERR_BADARG
    one = 1                                                                   # any non-null address: nothing is launched
    seg = lambda **k: lib.gnn_toy_segment_graphs(*[k.get(n, one) for n in (                        # noqa: E731
        "hit_x", "hit_y", "det_r")], k.get("E", 1), k.get("L", 10), k.get("T", 5), k.get("c", 2e-4),
        *[k.get(n, one) for n in ("X", "y", "row_cnt", "row_idx", "row_val")], None)
    for name in ("hit_x", "hit_y", "det_r", "X", "y", "row_cnt", "row_idx", "row_val"):
        assert seg(**{name: None}) == bad
        assert name.encode() in lib.gnn_last_error(), (name, lib.gnn_last_error())
    assert seg(E=-1) == bad and b"n_events" in lib.gnn_last_error()
    assert seg(E=2 ** 31) == bad and b"n_events" in lib.gnn_last_error()
    assert seg(c=0.0) == bad and b"two_sigma2" in lib.gnn_last_error()
    assert seg(c=float("nan")) == bad and seg(c=float("inf")) == bad and seg(c=-1.0) == bad
    assert seg(T=17) == _lib.GNN_ERR_UNSUPPORTED and b"n_tracks" in lib.gnn_last_error()
    assert seg(L=1) == _lib.GNN_ERR_UNSUPPORTED and b"n_layers" in lib.gnn_last_error()
    hit = lambda **k: lib.gnn_toy_hit_graphs(*[k.get(n, one) for n in (                            # noqa: E731
        "hit_x", "hit_y", "det_r", "r_norm", "norm_table")], k.get("E", 1), k.get("L", 10), k.get("T", 4), 3,
        k.get("norm", 1), 0, *[k.get(n, one) for n in ("X", "y0", "row_cnt", "row_idx", "row_val", "col_cnt", "col_idx",
                                                       "col_val", "n_isolated")], None)
    for name in ("det_r", "r_norm", "norm_table", "n_isolated"):
        assert hit(**{name: None}) == bad
        assert name.encode() in lib.gnn_last_error(), (name, lib.gnn_last_error())
    assert hit(norm=3) == bad and b"norm" in lib.gnn_last_error()
    assert hit(E=-1) == bad and b"n_events" in lib.gnn_last_error()
    assert hit(T=17) == _lib.GNN_ERR_UNSUPPORTED
    assert lib.gnn_toy_graphs_list_width(2, 10, 5, 0) == 0 and b"kind" in lib.gnn_last_error()
    assert lib.gnn_toy_graphs_list_width(0, 10, 5, 1) == 0 and b"norm" in lib.gnn_last_error()


def test_python_side_validation():
    x32, x64 = torch.zeros(2, 50), torch.zeros(2, 40, dtype=torch.float64)
    y5, y4 = torch.zeros(2, 50, dtype=torch.int64), torch.zeros(2, 40, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        toy_graphs.build_toy_segment_graphs(x32, y5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        toy_graphs.build_toy_hit_graphs(x64, y4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        toy_graphs.sort_toy_tracks(torch.zeros(2, 4, 10))
    with pytest.raises(ValueError, match="sigma"):
        toy_graphs.build_toy_segment_graphs(x32, y5, sigma=0.0)
    with pytest.raises(ValueError, match="sigma"):
        toy_graphs.build_toy_segment_graphs(x32, y5, sigma=1e-30)            # 2 sigma^2 underflows float32
    with pytest.raises(ValueError, match="strictly increasing"):
        toy_graphs.build_toy_segment_graphs(x32, y5, det_r=(0, 1, 1, 2, 3))
    with pytest.raises(ValueError, match="strictly increasing"):
        toy_graphs.build_toy_hit_graphs(x64, y4, det_r=(0, 1, float("nan"), 3))
    with pytest.raises(ValueError, match="at least 2"):
        toy_graphs.build_toy_hit_graphs(x64, y4, det_r=(0,))
    with pytest.raises(ValueError, match="norm"):
        toy_graphs.build_toy_hit_graphs(x64, y4, norm="col")
