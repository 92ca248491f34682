"""The full-event graph builder's specification (gnn-fpga_amd/event_graphs.py) against the reference's own graph
preparation (tests/golden/event_graphs, written by tools/gen_event_graphs_golden.py running cells 5, 7, 8, 16-18 and
24 of gnn/MPNN_Seg_ACTS_fullEvents.ipynb), GraphStore.from_batch, input validation and the C ABI's new entry points;
no GPU."""
import json
import os
import re

import numpy as np
import pytest
import torch

from gnn_fpga_amd import EventGraphs, GraphStore, HitGraph, _lib, batch_generator, build_event_graphs, synth
from gnn_fpga_amd.event_graphs import barrel_layers, build_event_graphs_numpy
from event_graphs_fixtures import CASES, COLS, GOLD, assert_equals_reference, build, load

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixtures_cover_the_cases():
    assert set(CASES) >= {"duplicates", "missing_layers", "odd_zero_layid", "non_barrel_empty_event", "phi_wrap",
                          "thresholds", "filter", "notebook"}
    assert os.path.exists(os.path.join(GOLD, "reference_time.json"))
    for c in CASES:
        assert json.loads(str(load(c)["dtypes"])) == {"features": "float64", "layer": "int8", "phi": "float32",
                                                      "z": "float32"}


@pytest.mark.parametrize("case", CASES)
def test_specification_equals_the_reference(case):
    f = load(case)
    g = build(f)
    assert isinstance(g, EventGraphs) and g.batch.X.device.type == "cpu"
    assert_equals_reference(g, f)


def test_fixture_traps_are_present():
    """The cases pin what they are named for."""
    f = load("duplicates")
    ev = np.repeat(np.arange(len(f["event_ptr"]) - 1), np.diff(f["event_ptr"]))
    k = np.stack([ev, f["barcode"], f["volid"], f["layid"], f["r"].view(np.int32)])
    assert np.unique(k, axis=1).shape[1] < k.shape[1]                 # two rows of one group with exactly equal r
    g = build(load("odd_zero_layid"))
    assert int(g.layer.min()) == -1 and set(g.layer.tolist()) >= {-1, 0, 2, 3, 4, 7}
    lay = g.layer.numpy()
    src = g.batch.src.numpy()
    assert np.any(lay[src] == -1)                                     # a layer -1 hit starts segments to layer 0
    f = load("non_barrel_empty_event")
    assert not np.isin(f["volid"], (8, 13, 17)).all() and build(f).event_index.tolist() == [0, 2]
    assert np.abs(load("phi_wrap")["phi"]).max() > 3.14
    f = load("thresholds")
    g = build(f)
    pos = {int(b): i for i, b in enumerate(f["barcode"][g.hit_index.numpy()])}
    seg = set(zip(g.batch.src.tolist(), g.batch.dst.tolist()))
    t7 = np.float32(0.7)
    assert f["phi"][f["barcode"] == 701][0] == t7 and f["z"][f["barcode"] == 704][0] == t7
    assert (pos[701], pos[702]) not in seg and (pos[701], pos[704]) not in seg       # exactly f32(0.7): left out
    assert (pos[701], pos[703]) in seg and (pos[701], pos[705]) in seg               # one ulp less: kept
    f = load("filter")
    every = build(f, n_nodes_min=None, n_nodes_max=None, n_edges_max=None)
    nh, ns = np.diff(every.batch.hit_ptr), np.diff(every.batch.seg_ptr)
    lo, hi, emax = (int(v) for v in f["bounds"])
    assert np.any(nh <= lo) and np.any(nh == hi) and np.any((nh > lo) & (nh < hi) & (ns == emax))
    assert 0 < len(build(f)) < len(every)
    nh = np.diff(load("notebook")["ref_hit_ptr"])
    assert nh.min() > 50 and nh.max() < 500


def test_layer_renumbering():
    """The (volid, layid) -> layer values observed in the reference."""
    vol = np.array([13, 17, 8, 8, 8, 8, 7])
    lid = np.array([3, 1, 9, 7, 0, 2, 2])
    sel, lay = barrel_layers(vol, lid)
    assert sel.tolist() == [True] * 6 + [False] and lay[:6].tolist() == [4, 7, 3, 2, -1, 0]
    assert barrel_layers(np.array([8]), np.array([1]))[1].tolist() == [0]           # -0.5 truncates toward zero
    assert barrel_layers(np.array([8, 17]), np.array([-254, 238]))[1].tolist() == [-128, 126]
    for v, l in ((17, 242), (8, -256)):
        with pytest.raises(ValueError, match="layer outside int8"):
            barrel_layers(np.array([v]), np.array([l]))
    assert barrel_layers(np.array([9]), np.array([10 ** 6]))[0].tolist() == [False]  # not a barrel row: no layer


def test_hit_index_layer_and_labels_are_consistent():
    f = load("notebook")
    g = build(f)
    hi = g.hit_index.numpy()
    assert np.array_equal(g.batch.X[:, 2].numpy(), (f["z"][hi].astype(np.float64) / 1000.0).astype(np.float32))
    assert np.array_equal(g.layer.numpy(), barrel_layers(f["volid"], f["layid"])[1][hi]) and g.layer.dtype == torch.int32
    src, dst = g.batch.src.numpy(), g.batch.dst.numpy()
    assert np.all(g.layer.numpy()[dst] - g.layer.numpy()[src] == 1)
    assert np.array_equal(g.batch.y.numpy(), f["barcode"][hi][src] == f["barcode"][hi][dst])
    ev = np.repeat(np.arange(len(f["event_ptr"]) - 1), np.diff(f["event_ptr"]))
    assert np.array_equal(ev[hi], np.repeat(g.event_index.numpy(), np.diff(g.batch.hit_ptr)))
    for a, b in zip(g.batch.hit_ptr[:-1], g.batch.hit_ptr[1:]):                       # (barcode, layer) order
        k = np.stack([f["barcode"][hi[a:b]], g.layer.numpy()[a:b]], axis=1)
        assert np.array_equal(k, k[np.lexsort((k[:, 1], k[:, 0]))]) and len(np.unique(k, axis=0)) == b - a


def test_padded_batch_of_4_equals_merge_samples():
    f = load("notebook")
    g = build(f)
    b, y = g.store().batch(0, 4, "padded")
    bX, bs, bd, by = f["batch_X"], f["batch_src"], f["batch_dst"], f["batch_y"]
    assert b.dense_shape == (4, bX.shape[1], by.shape[1]) and tuple(y.shape) == by.shape
    assert np.array_equal(y.numpy(), by.astype(np.float32))
    src, dst = b.src.numpy().reshape(by.shape), b.dst.numpy().reshape(by.shape)
    for k in range(4):
        h0, h1 = int(b.hit_ptr[k]), int(b.hit_ptr[k + 1])
        assert np.array_equal(b.X[h0:h1].numpy().view(np.uint32), bX[k, :h1 - h0].view(np.uint32))
        assert not bX[k, h1 - h0:].any()                                              # merge_samples' zero rows
        assert np.array_equal(np.where(src[k] >= 0, src[k] - h0, -1), bs[k])
        assert np.array_equal(np.where(dst[k] >= 0, dst[k] - h0, -1), bd[k])
    gen = batch_generator(g.store(), len(g), batch_size=4, layout="padded")
    b0, y0 = next(gen)
    b1, y1 = next(gen)
    assert torch.equal(b0.X, b.X) and torch.equal(y0, y) and b1.n_graphs == len(g) - 4


def test_store_from_batch_equals_store_of_graphs():
    f = load("filter")
    g = build(f, n_nodes_min=None, n_nodes_max=None, n_edges_max=None)
    b = g.batch
    graphs = []
    for k in range(len(g)):
        h0, h1, s0, s1 = (int(v) for v in (b.hit_ptr[k], b.hit_ptr[k + 1], b.seg_ptr[k], b.seg_ptr[k + 1]))
        graphs.append(HitGraph(b.X[h0:h1].numpy(), b.src[s0:s1].numpy() - h0, b.dst[s0:s1].numpy() - h0,
                               b.y[s0:s1].numpy()))
    a, c = GraphStore.from_batch(b), GraphStore(graphs)
    assert a.n_graphs == c.n_graphs and np.array_equal(a.hit_ptr, c.hit_ptr) and np.array_equal(a.seg_ptr, c.seg_ptr)
    for u, v in ((a.X, c.X), (a.src, c.src), (a.dst, c.dst), (a.y, c.y)):
        assert u.dtype == v.dtype and torch.equal(u, v)
    for layout in ("padded", "flat"):
        for j, bs in ((0, 3), (3, 4), (7, 4), (0, len(g))):
            (p, py), (q, qy) = a.batch(j, bs, layout), c.batch(j, bs, layout)
            assert torch.equal(p.X, q.X) and torch.equal(p.src, q.src) and torch.equal(p.dst, q.dst)
            assert torch.equal(py, qy) and p.dense_shape == q.dense_shape
            assert np.array_equal(p.hit_ptr, q.hit_ptr) and np.array_equal(p.seg_ptr, q.seg_ptr)
    bad = build(f)
    bad.batch.hit_ptr = bad.batch.hit_ptr[:-1]
    with pytest.raises(ValueError, match="hit_ptr"):
        GraphStore.from_batch(bad.batch)


def test_specification_on_synthetic_events():
    """Properties the fixtures are too small for, on seeded acts_events: the filter is the three strict tests on the
    unfiltered sizes, and a brute-force adjacency of one event gives the same segments."""
    ev = synth.acts_events(40, (3, 40), (5, 100), seed=5)
    every = build_event_graphs(*ev)
    nh, ns = np.diff(every.batch.hit_ptr), np.diff(every.batch.seg_ptr)
    some = build_event_graphs(*ev, n_nodes_min=50, n_nodes_max=400, n_edges_max=1500)
    ok = (nh > 50) & (nh < 400) & (ns < 1500)
    assert 0 < ok.sum() < 40 and np.array_equal(some.event_index.numpy(), every.event_index.numpy()[ok])
    assert np.array_equal(np.diff(some.batch.hit_ptr), nh[ok]) and np.array_equal(np.diff(some.batch.seg_ptr), ns[ok])
    one = build_event_graphs(*ev[:6], ev.event_ptr, n_nodes_min=int(nh.max()) - 1)     # the largest event alone
    hi = one.hit_index.numpy()
    phi, z, lay = ev.phi[hi], ev.z[hi], one.layer.numpy()
    d = phi[:, None] - phi[None, :]
    d[d > np.float32(np.pi)] -= np.float32(2 * np.pi)
    d[d < -np.float32(np.pi)] += np.float32(2 * np.pi)
    adj = ((lay[None, :] - lay[:, None]) == 1) & (np.abs(d) < np.float32(np.pi / 4)) & \
        (np.abs(z[None, :] - z[:, None]) < np.float32(300.0))
    i, j = np.where(adj)
    assert len(one) == 1 and np.array_equal(one.batch.src.numpy(), i) and np.array_equal(one.batch.dst.numpy(), j)


def test_empty_results():
    z32, zi = np.zeros(0, np.float32), np.zeros(0, np.int32)
    e = build_event_graphs(z32, z32, z32, zi, zi, np.zeros(0, np.int64))
    assert len(e) == 0 and e.batch.n_hits == 0 and e.batch.n_segments == 0 and tuple(e.batch.X.shape) == (0, 3)
    assert e.event_index.shape == (0,) and e.store().n_graphs == 0
    f = load("non_barrel_empty_event")
    none = build(f, cols=[f["r"], f["phi"], f["z"], np.full_like(f["volid"], 9), f["layid"], f["barcode"]])
    assert len(none) == 0 and none.batch.hit_ptr.tolist() == [0]
    assert len(build(load("filter"), n_nodes_max=10)) == 0


def test_input_validation():
    f = load("missing_layers")
    r, phi, z, vol, lid, bc = (f[k] for k in COLS)
    ep = f["event_ptr"]
    for k in range(3):
        c = [r, phi, z]
        c[k] = c[k].astype(np.float64)
        with pytest.raises(ValueError, match="float64: the reference's cuts are float32 arithmetic"):
            build_event_graphs(*c, vol, lid, bc, ep)
    with pytest.raises(ValueError, match="entries"):
        build_event_graphs(r, phi[:-1], z, vol, lid, bc, ep)
    with pytest.raises(ValueError, match="entries"):
        build_event_graphs(r, phi, z, vol, lid[:-1], bc, ep)
    with pytest.raises(ValueError, match="integer"):
        build_event_graphs(r, phi, z, vol.astype(np.float32), lid, bc, ep)
    with pytest.raises(ValueError, match="barcode"):
        build_event_graphs(r, phi, z, vol, lid, None, ep)
    for bad_ep in (ep[::-1].copy(), ep[:-1], ep + 1, np.array([0]), ep.astype(np.float32)):
        with pytest.raises(ValueError, match="event_ptr"):
            build_event_graphs(r, phi, z, vol, lid, bc, bad_ep)
    for col in range(3):
        c = [r.copy(), phi.copy(), z.copy()]
        c[col][5] = (np.nan, np.inf, -np.inf)[col]
        with pytest.raises(ValueError, match="non-finite"):
            build_event_graphs(*c, vol, lid, bc, ep)
    wide = lid.copy()
    wide[np.flatnonzero(vol == 17)[0]] = 300
    with pytest.raises(ValueError, match="layer outside int8"):
        build_event_graphs(r, phi, z, vol, wide, bc, ep)
    for kw in ({"feature_scale": (1.0, 0.0, 1.0)}, {"feature_scale": (1.0, 2.0)}, {"n_nodes_min": 1.5},
               {"n_edges_max": "many"}, {"dphi_max": float("nan")}):
        with pytest.raises((ValueError, TypeError)):
            build_event_graphs(r, phi, z, vol, lid, bc, ep, **kw)
    t = torch.from_numpy
    g = build_event_graphs(t(r), t(phi), t(z), t(vol), t(lid), t(bc), t(ep))
    assert g.batch.X.device.type == "cpu" and torch.equal(g.batch.X, build(f).batch.X)


def test_numpy_entry_point_matches():
    f = load("filter")
    a = build(f)
    b = build_event_graphs_numpy(*[f[k] for k in COLS], f["event_ptr"], np.pi / 4, 300.0, (1000.0, np.pi, 1000.0),
                                 *[int(v) for v in f["bounds"]])
    assert torch.equal(a.batch.X, b.batch.X) and torch.equal(a.hit_index, b.hit_index)
    assert torch.equal(a.batch.src, b.batch.src) and torch.equal(a.event_index, b.event_index)


def test_new_symbols_are_declared_bound_and_exported():
    with open(os.path.join(REPO, "include", "gnn_hip.h")) as fh:
        hdr = fh.read()
    names = ("gnn_event_graphs_workspace_bytes", "gnn_event_graphs_sizes", "gnn_event_graphs_fill")
    for n in names:
        assert re.search(r"\b%s\(" % n, hdr) and n in _lib.SIGNATURES
    assert "GNN_ABI_VERSION 7" in hdr and _lib.GNN_ABI_VERSION == 7
    for cell in ("cell 5", "cell 7", "cell 8", "16-18", "cell 24"):             # each cites the cells it replaces
        assert cell in hdr.split("csrc/event_graphs.hip; ABI 7")[1].split("gnn_event_graphs_fill(")[0]
    lib = _lib.load()
    for n in names:
        assert hasattr(lib, n)
    assert lib.gnn_abi_version() == 7
    assert lib.gnn_event_graphs_workspace_bytes(100, 0) == 0 and "n_events" in lib.gnn_last_error().decode()
    assert lib.gnn_event_graphs_workspace_bytes(-1, 1) == 0
    assert lib.gnn_event_graphs_workspace_bytes(2 ** 31, 1) == 0
    assert lib.gnn_event_graphs_workspace_bytes(100, 3) > 0
    nulls = lib.gnn_event_graphs_sizes(None, None, None, None, None, None, 10, None, 1, 0.5, 1.0, -1, 2 ** 63 - 1,
                                       2 ** 63 - 1, None, 0, None, None, None, None, None)
    assert nulls == _lib.GNN_ERR_BADARG and "pointer" in lib.gnn_last_error().decode()
    nan_cut = lib.gnn_event_graphs_sizes(None, None, None, None, None, None, 10, None, 1, float("nan"), 1.0, -1, 5, 5,
                                         None, 0, None, None, None, None, None)
    assert nan_cut == _lib.GNN_ERR_BADARG and "NaN" in lib.gnn_last_error().decode()
    assert lib.gnn_event_graphs_sizes(None, None, None, None, None, None, 10, None, 0, 0.5, 1.0, -1, 5, 5, None, 0,
                                      None, None, None, None, None) == _lib.GNN_ERR_BADARG
    flagged = _lib.GnnEventGraphsSizes(n_graphs=1, n_hits=5, n_segments=4, n_kept=5, n_tasks=1, n_tested=4, status=8)
    assert lib.gnn_event_graphs_fill(None, None, None, None, 100, 1, 0.5, 1.0, 1.0, 1.0, 1.0, flagged, None, 0,
                                     *([None] * 7)) == _lib.GNN_ERR_BADARG
    assert "flagged" in lib.gnn_last_error().decode()
    too_many = _lib.GnnEventGraphsSizes(n_graphs=1, n_hits=500, n_segments=4, n_kept=500, n_tasks=1, n_tested=4)
    assert lib.gnn_event_graphs_fill(None, None, None, None, 100, 1, 0.5, 1.0, 1.0, 1.0, 1.0, too_many, None, 0,
                                     *([None] * 7)) == _lib.GNN_ERR_BADARG
    fine = _lib.GnnEventGraphsSizes(n_graphs=1, n_hits=5, n_segments=4, n_kept=5, n_tasks=1, n_tested=4)
    assert lib.gnn_event_graphs_fill(None, None, None, None, 100, 1, 0.5, 1.0, 1.0, 1.0, 1.0, fine, None, 0,
                                     *([None] * 7)) == _lib.GNN_ERR_BADARG
    assert "pointer" in lib.gnn_last_error().decode()


def test_units_name_event_graphs():
    from variant_scripts import assert_variant_libraries_link
    assert_variant_libraries_link("event_graphs")


def test_new_kernels_have_no_scratch():
    path = os.path.join(REPO, "build", "event_graphs.remarks")
    if not os.path.exists(path):
        pytest.fail("build/event_graphs.remarks is missing: build the library first")
    with open(path) as fh:
        text = fh.read()
    blocks = re.split(r"remark: Function Name: ", text)[1:]
    ours = [b for b in blocks if "k_eg_" in b.split()[0]]
    assert len(ours) >= 13                                        # eleven kernels, k_eg_pairs in two forms
    for b in ours:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, b.split()[0]
