"""Every batch-assembly entry on the host against ONE restatement (tests/batch_cases.py `assemble`: plain loops, the
reference's rule of gnn/trainSegmentClassifier.py:66-111): `HitGraphBatch.from_graphs` / `merge_graphs`,
`GraphStore.batch`, `GraphStore.from_batch`, and `batch_generator` over a list and over a store - every window of a
ragged dataset (a graph without segments, one with padded segments of its own, one with a negative pair that is not
(-1, -1)), tail windows (`n_samples` no multiple of `batch_size`, fewer samples than graphs), windows without graphs,
and malformed graphs, which every entry refuses with a ValueError that names the graph."""
import numpy as np
import pytest
import torch

import gnn_fpga_amd
from batch_cases import LAYOUTS, MALFORMED, RAGGED, assemble, assert_batch_equal, long_y, short_y, windows
from gnn_fpga_amd import HitGraphBatch, synth
from gnn_fpga_amd.batcher import GraphStore, merge_graphs


def test_the_restatement_on_a_case_worked_out_by_hand():
    """`assemble` itself, on three graphs small enough to write the answer down."""
    f = np.float32
    g0 = synth.HitGraph(np.array([[1, 2], [3, 4], [5, 6]], f), np.array([0, 1]), np.array([1, 2]), np.array([1, 0], f))
    g1 = synth.HitGraph(np.zeros((2, 2), f), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, f))
    g2 = synth.HitGraph(np.array([[7, 8], [9, 10]], f), np.array([1, -4, 0]), np.array([0, -2, 1]), np.array([0, 0, 1], f))
    a = assemble([g0, g1, g2], 0, 3, "padded")
    assert a.src.tolist() == [0, 1, -1, -1, -1, -1, 6, -1, 5] and a.dst.tolist() == [1, 2, -1, -1, -1, -1, 5, -1, 6]
    assert a.y.tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 1] and a.dense_shape == (3, 3, 3)
    assert a.hit_ptr.tolist() == [0, 3, 5, 7] and a.seg_ptr.tolist() == [0, 3, 6, 9]
    assert a.X.tolist() == [[1, 2], [3, 4], [5, 6], [0, 0], [0, 0], [7, 8], [9, 10]]
    a = assemble([g0, g1, g2], 1, 5, "flat")
    assert a.src.tolist() == [3, -1, 2] and a.dst.tolist() == [2, -1, 3] and a.y.tolist() == [0, 0, 1]
    assert a.hit_ptr.tolist() == [0, 2, 4] and a.seg_ptr.tolist() == [0, 0, 3] and a.dense_shape is None
    assert (a.X.dtype, a.src.dtype, a.y.dtype, a.seg_ptr.dtype) == (np.float32, np.int32, np.float32, np.int64)
    assert windows(5, 2) == [0, 2, 4] and windows(6, 4) == [0, 4] and windows(1, 1) == [0] and windows(3, 8) == [0]


def test_every_window_of_every_path_equals_the_restatement():
    """j in 0..6, batch_size in 1..8 over the seven ragged graphs, both layouts: 2 x 56 = 112 windows, none skipped."""
    compared = {layout: _every_window(layout) for layout in LAYOUTS}
    assert compared == {"padded": 56, "flat": 56} and sum(compared.values()) == 112


def _every_window(layout):
    graphs = RAGGED
    store = GraphStore(graphs)
    whole = HitGraphBatch.from_graphs(graphs)
    back = GraphStore.from_batch(whole)
    kept = [t.clone() for t in (store.X, store.src, store.dst, store.y, whole.X, whole.src, whole.dst, whole.y)]
    compared = 0
    for j in range(7):
        for k in range(1, 9):
            want = assemble(graphs, j, k, layout)
            assert_batch_equal(merge_graphs(graphs[j:j + k], layout), want)
            assert_batch_equal(store.batch(j, k, layout), want)
            assert_batch_equal(back.batch(j, k, layout), want)
            b = HitGraphBatch.from_graphs(graphs[j:j + k], pad_segments=layout == "padded", pin_memory=False)
            assert_batch_equal((b, b.y.reshape(-1) if layout == "flat" else b.y.view(b.dense_shape[0], b.dense_shape[2])),
                               want)
            # the y handed out is a copy: writing into it reaches neither the batch nor the dataset
            for got, y in (merge_graphs(graphs[j:j + k], layout), store.batch(j, k, layout), back.batch(j, k, layout)):
                y.fill_(7.0)
                assert np.array_equal(got.y.numpy(), want.y)
            compared += 1
    now = (store.X, store.src, store.dst, store.y, whole.X, whole.src, whole.dst, whole.y)
    assert all(torch.equal(a, b) for a, b in zip(kept, now))
    assert all(torch.equal(a, b) for a, b in zip((back.X, back.y), (whole.X, whole.y)))
    return compared


GENERATOR_CASES = [(6, 5, 2), (7, 7, 3), (7, 6, 4), (7, 1, 1), (7, 7, 7), (7, 3, 8)]     # graphs, n_samples, batch_size


@pytest.mark.parametrize("n_graphs,n_samples,batch_size", GENERATOR_CASES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_generator_windows_from_a_list_and_from_a_store(layout, n_graphs, n_samples, batch_size):
    """Two epochs: batch b is assemble(graphs, windows[b], batch_size) - the tail window is not clipped to n_samples -
    from the list and from the store alike; with the cache the second epoch hands the same objects out."""
    graphs = RAGGED[:n_graphs]
    starts = windows(n_samples, batch_size)
    want = [assemble(graphs, j, batch_size, layout) for j in starts]
    kw = dict(n_samples=n_samples, batch_size=batch_size, layout=layout)
    from_list = gnn_fpga_amd.batch_generator(graphs, **kw)
    from_store = gnn_fpga_amd.batch_generator(GraphStore(graphs), **kw)
    seen = {"list": [], "store": []}
    for epoch in range(2):
        for b in range(len(starts)):
            items = {"list": next(from_list), "store": next(from_store)}
            for name, item in items.items():
                assert_batch_equal(item, want[b])
                seen[name].append(item)
            (bl, yl), (bs, ys) = items["list"], items["store"]
            assert all(torch.equal(getattr(bl, k), getattr(bs, k)) for k in ("X", "src", "dst", "y")) and torch.equal(yl, ys)
    n = len(starts)
    for items in seen.values():
        assert all(a[0] is c[0] and a[1] is c[1] for a, c in zip(items[:n], items[n:]))
    uncached = gnn_fpga_amd.batch_generator(GraphStore(graphs), cache=False, **kw)
    first = [next(uncached) for _ in range(n)]
    second = [next(uncached) for _ in range(n)]
    for b in range(n):
        assert first[b][0] is not second[b][0]
        assert_batch_equal(second[b], want[b])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_window_without_graphs_is_an_empty_batch(layout):
    """GraphStore.batch keeps Python's slice semantics: a window that starts at or past the end raises nothing."""
    store = GraphStore(RAGGED)
    for j, k in ((7, 4), (9, 2), (7, 0), (3, 0), (100, 100)):
        b, y = store.batch(j, k, layout)
        assert (b.n_graphs, b.n_hits, b.n_segments) == (0, 0, 0) and b.n_features == 3
        assert y.numel() == 0 and b.y.numel() == 0 and b.src.dtype == torch.int32 and b.X.dtype == torch.float32
        assert np.array_equal(b.hit_ptr, [0]) and np.array_equal(b.seg_ptr, [0])
        assert b.dense_shape == ((0, 0, 0) if layout == "padded" else None)
    assert_batch_equal(store.batch(5, 100, layout), assemble(RAGGED, 5, 100, layout))
    with pytest.raises(ValueError):
        store.batch(-1, 2, layout)


@pytest.mark.parametrize("store", [False, True])
def test_generator_refuses_a_configuration_with_an_empty_window(store):
    graphs = [synth.layered_graph(20 + 3 * s, 50 + 7 * s, 3, n_layers=3, seed=s) for s in range(6)]
    data = GraphStore(graphs) if store else graphs
    for n_samples, batch_size in ((9, 2), (7, 1), (7, 6), (13, 4), (0, 2), (-3, 2), (5, 0), (5, -1)):
        with pytest.raises(ValueError, match="n_samples"):
            next(gnn_fpga_amd.batch_generator(data, n_samples=n_samples, batch_size=batch_size))
    # the last window may reach past n_samples and past the data, as long as it holds a graph
    for n_samples, batch_size, sizes in ((5, 2, [2, 2, 2]), (6, 4, [4, 2]), (7, 7, [6]), (8, 8, [6]), (6, 1, [1] * 6),
                                         (100, 100, [6])):
        gen = gnn_fpga_amd.batch_generator(data, n_samples=n_samples, batch_size=batch_size)
        assert [next(gen)[0].n_graphs for _ in sizes] == sizes


def _place(name, pos):
    """RAGGED's (7, 7) graph, malformed as `name` says, at list position `pos` among well-formed graphs."""
    graphs = [RAGGED[3], RAGGED[0], RAGGED[2], RAGGED[5], RAGGED[1]]
    graphs[pos] = MALFORMED[name](RAGGED[4])
    return graphs


def _refusals(graphs, pos, pins=(False, None)):
    """Every entry that takes a list of graphs refuses this one, naming graph `pos`; none lets a numpy message out."""
    named = r"graph %d\b" % pos
    for layout in LAYOUTS:
        for pin in pins:
            with pytest.raises(ValueError, match=named):
                HitGraphBatch.from_graphs(graphs, pad_segments=layout == "padded", pin_memory=pin)
        with pytest.raises(ValueError, match=named):
            merge_graphs(graphs, layout)
        with pytest.raises(ValueError, match=named):
            gen = gnn_fpga_amd.batch_generator(graphs, n_samples=len(graphs), batch_size=2, layout=layout)
            for _ in range(pos // 2 + 1):              # the windows before the graph's own are well-formed
                next(gen)
    with pytest.raises(ValueError, match=named):
        GraphStore(graphs)


@pytest.mark.parametrize("pos", [0, 2, 4])
@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_malformed_graphs_are_refused_by_name(name, pos):
    """y too short or too long, X not [N, F of graph 0], endpoints of a non-integer dtype, exactly one negative end,
    an endpoint >= n_hits: first, in the middle and last in the list."""
    if pos == 0 and name in ("x_narrow", "x_wide"):
        # graph 0 sets the width: the graphs after it are the ones that do not fit
        graphs = _place(name, 0)
        with pytest.raises(ValueError, match=r"graph 1\b"):
            merge_graphs(graphs)
        with pytest.raises(ValueError, match=r"graph 1\b"):
            GraphStore(graphs)
        return
    _refusals(_place(name, pos), pos)


def test_label_arrays_of_the_wrong_length_never_reach_a_batch():
    """The issue's own cases: a y three short, a y four long (first, middle, last), and the constructor."""
    graphs = [synth.layered_graph(20 + 3 * s, 50 + 7 * s, 3, n_layers=3, seed=s) for s in range(3)]
    for pos in range(3):
        for bad in (short_y(graphs[pos], 3), long_y(graphs[pos], 4), short_y(graphs[pos], 1), long_y(graphs[pos], 1)):
            gs = list(graphs)
            gs[pos] = bad
            _refusals(gs, pos)
    g = graphs[0]
    for y in (g.y[:-3], np.concatenate([g.y, g.y[:4]]), g.y[:0], g.y[None]):
        with pytest.raises(ValueError, match="y of shape"):
            HitGraphBatch(g.X, g.src, g.dst, y=y)
    assert HitGraphBatch(g.X, g.src, g.dst, y=g.y).y.shape == (50,) and HitGraphBatch(g.X, g.src, g.dst).y is None


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_dataset_with_unlabelled_graphs_has_no_labels(layout):
    graphs = list(RAGGED[:4])
    graphs[2] = synth.HitGraph(graphs[2].X, graphs[2].src, graphs[2].dst, None)
    want = assemble(RAGGED, 0, 4, layout)
    gen_list = gnn_fpga_amd.batch_generator(graphs, n_samples=4, batch_size=4, layout=layout)
    gen_store = gnn_fpga_amd.batch_generator(GraphStore(graphs), n_samples=4, batch_size=4, layout=layout)
    for b, y in (merge_graphs(graphs, layout), GraphStore(graphs).batch(0, 4, layout), next(gen_list), next(gen_store)):
        assert y is None and b.y is None
        assert np.array_equal(b.src.numpy(), want.src) and np.array_equal(b.dst.numpy(), want.dst)
        assert np.array_equal(b.X.numpy(), want.X) and b.dense_shape == want.dense_shape
    # a labelled graph of such a dataset is still checked
    graphs[1] = short_y(RAGGED[0])
    with pytest.raises(ValueError, match=r"graph 1\b"):
        merge_graphs(graphs, layout)
    with pytest.raises(ValueError, match=r"graph 1\b"):
        GraphStore(graphs)
