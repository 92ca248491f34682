"""gnn_fx_forward (include/gnn_hip_fixed.h) against the numpy specification `fixed_forward_numpy`, bit for bit: raw
scores, both traces, the overflow counters and scores == raw * 2^-Fb.  No tolerance anywhere: the arithmetic is integers.

Each axis varies with the others at DEFAULT, then a handful of crossed cases.  `gain` scales every weight of torch's
default initialisation: at gain 1 the narrow-range formats barely overflow, the crossed cases make every stage do so."""
import numpy as np
import pytest
import torch

import fixed_point_cases as fc
from gnn_fpga_amd import (FixedPointFormat, HitGraph, HitGraphBatch, SegmentMetrics, fixed_forward_numpy, quantize_model,
                          scan_precision, synth)
from gnn_fpga_amd.metrics import segment_metrics_numpy

pytestmark = pytest.mark.gpu

#          graph      F  D  T   W  I  rounding overflow tb  gain
DEFAULT = ("layered", 3, 8, 3, 16, 6, "trn", "wrap", 10, 1.0)


def _vary(**kw):
    names = ("graph", "F", "D", "T", "W", "I", "rounding", "overflow", "tb", "gain")
    case = dict(zip(names, DEFAULT))
    case.update(kw)
    return tuple(case[n] for n in names)


CASES = (
    [_vary(F=F, D=D) for F, D in [(3, 8), (2, 32), (11, 8), (4, 16), (3, 64)]] +
    [_vary(T=T) for T in (0, 1)] +
    [_vary(W=W, I=I) for W, I in [(24, 8), (8, 3), (6, 4), (24, 2), (16, 3), (12, 12)]] +
    [_vary(rounding=r, overflow=o) for r, o in [("trn", "sat"), ("rnd", "wrap"), ("rnd", "sat")]] +
    [_vary(tb=tb) for tb in (4, 12)] +
    [_vary(graph=g) for g in ("star", "block3_padded", "one_hit")] + [_vary(graph="no_segments", T=2)] +
    [("star", 11, 8, 2, 16, 3, "rnd", "sat", 12, 2.0),
     ("layered", 3, 64, 1, 24, 2, "rnd", "wrap", 12, 2.0),
     ("star", 2, 32, 3, 8, 3, "trn", "sat", 4, 1.0),
     ("layered", 4, 16, 3, 12, 12, "rnd", "sat", 10, 6.0),
     ("star", 3, 8, 3, 24, 8, "rnd", "wrap", 12, 3.0),
     ("block3_padded", 3, 64, 2, 16, 3, "trn", "wrap", 7, 1.5),
     ("star", 4, 16, 1, 6, 4, "rnd", "wrap", 5, 4.0),
     ("layered", 3, 8, 3, 24, 2, "trn", "sat", 10, 2.0),
     ("layered", 3, 8, 2, 24, 2, "rnd", "wrap", 8, 2.0)]
)


def _graphs(kind, F):
    """(graphs, pad_segments)"""
    if kind == "layered":                   # 150 segments: more than one wave of segments, 70 hits: more than one of hits
        return [fc.layered(70, 150, F, 1)], False
    if kind == "star":
        return [fc.cached_star(0, F)], False
    if kind == "block3_padded":
        return [fc.layered(70, 150, F, 1), fc.layered(33, 41, F, 2), fc.cached_star(5, F)], True
    if kind == "one_hit":                   # N = 1, E = 0
        g = fc.layered(10, 12, F, 3)
        return [HitGraph(g.X[:1], g.src[:0], g.dst[:0], g.y[:0])], False
    if kind == "no_segments":               # E = 0 with hits
        g = fc.layered(40, 50, F, 3)
        return [HitGraph(g.X, g.src[:0], g.dst[:0], g.y[:0])], False
    raise KeyError(kind)


def _model(F, D, T, gain=1.0, seed=0):
    m = fc.default_model(F, D, T, seed)
    if gain != 1.0:
        with torch.no_grad():
            for p in m.parameters():
                p.mul_(gain)
    return m.cuda()


def _assert_bits(out, want, what=""):
    f = want.fmt
    got = {k: getattr(out, k).cpu().numpy() for k in ("raw", "scores", "counts", "e_trace", "H_trace")}
    assert got["raw"].dtype == np.int32 and got["scores"].dtype == np.float32 and got["counts"].dtype == np.int64
    assert got["e_trace"].dtype == np.int32 and got["H_trace"].dtype == np.int32
    for k in ("counts", "H_trace", "e_trace", "raw"):
        w = getattr(want, k)
        assert got[k].shape == w.shape, (what, k, got[k].shape, w.shape)
        bad = np.flatnonzero(got[k].reshape(-1) != w.reshape(-1))
        assert bad.size == 0, "%s %s: %d of %d differ, first at %d: %d != %d" % (
            what, k, bad.size, w.size, bad[0], got[k].reshape(-1)[bad[0]], w.reshape(-1)[bad[0]])
    assert np.array_equal(got["scores"].view(np.uint32), want.scores.view(np.uint32))
    assert np.array_equal(got["scores"].astype(np.float64), got["raw"].astype(np.float64) * 2.0 ** -f.frac_bits)
    return got


def _run(case):
    kind, F, D, T, W, I, rounding, overflow, tb, gain = case
    f = FixedPointFormat(W, I, rounding, overflow, tb)
    graphs, pad = _graphs(kind, F)
    hb = HitGraphBatch.from_graphs(graphs, pad_segments=pad)
    model = _model(F, D, T, gain)
    want = fixed_forward_numpy(hb.X.numpy(), hb.src.numpy(), hb.dst.numpy(), fc.host_weights(model), T, f)
    n_padded = int((hb.src.numpy() < 0).sum())
    qm = quantize_model(model, f)
    hb = hb.to("cuda")                      # (moves the batch itself)
    out = qm(hb, trace=True)
    got = _assert_bits(out, want, str(case))
    plain = qm(hb)
    assert plain.e_trace is None and plain.H_trace is None and plain.fmt == f
    assert torch.equal(plain.raw, out.raw) and torch.equal(plain.counts, out.counts) and torch.equal(plain.scores, out.scores)
    return got, want, hb, n_padded


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_bit_equal_to_the_specification(hip, case):
    got, want, hb, n_padded = _run(case)
    if case[0] == "block3_padded":
        assert hb.dense_shape is not None and n_padded > 100
    print("overflows per stage:", got["counts"].sum(axis=0).tolist())


def test_the_cases_overflow_in_every_stage(hip):
    """Together the cases above must run requant's overflow branch in every kernel, in both modes."""
    total = {"wrap": np.zeros(6, dtype=np.int64), "sat": np.zeros(6, dtype=np.int64)}
    for case in CASES:
        if case[-1] != 1.0:
            kind, F, D, T, W, I, rounding, overflow, tb, gain = case
            graphs, pad = _graphs(kind, F)
            hb = HitGraphBatch.from_graphs(graphs, pad_segments=pad)
            f = FixedPointFormat(W, I, rounding, overflow, tb)
            total[overflow] += fixed_forward_numpy(hb.X.numpy(), hb.src.numpy(), hb.dst.numpy(),
                                                   fc.host_weights(_model(F, D, T, gain)), T, f).counts.sum(axis=0)
    assert np.all(total["wrap"] > 0) and np.all(total["sat"] > 0), total


@pytest.mark.parametrize("n_hits,n_segments,T", [(5000, 50000, 3), (140000, 300000, 1)])
def test_large_graphs(hip, n_hits, n_segments, T):
    """5 000 hits and 50 000 segments: many workgroups of every kernel.  140 000 hits and 300 000 segments: past one pass
    of every kernel's grid on a 256-CU part (the hit kernels launch at most 2 workgroups of 256 lanes per CU, the
    segment and column kernels 4: 131 072 and 262 144 items), so the grid-stride loops go round."""
    g = synth.layered_graph(n_hits, n_segments, 3, seed=11)
    hb = HitGraphBatch.from_graphs([g])
    model = _model(3, 8, T, 2.0)
    f = FixedPointFormat(24, 2, "rnd", "sat", 10)          # two integer bits: every stage overflows somewhere
    want = fixed_forward_numpy(g.X, g.src, g.dst, fc.host_weights(model), T, f)
    got = _assert_bits(quantize_model(model, f)(hb.to("cuda"), trace=True), want)
    assert got["counts"].sum() > 0


def test_star_overflow_modes(hip):
    """Format (16, 3) on the star graph: the sums of hit 0 leave the word.  Both modes equal the specification, the
    counters are non-zero, and the modes differ from each other."""
    raws = {}
    for overflow in ("wrap", "sat"):
        got, want, _, _ = _run(_vary(graph="star", W=16, I=3, overflow=overflow))
        assert got["counts"].sum() > 0 and got["counts"][:, 3].sum() > 0
        raws[overflow] = got["raw"]
    assert int((raws["wrap"] != raws["sat"]).sum()) > 306 // 2


def test_two_runs_give_the_same_bits(hip):
    graphs, _ = _graphs("star", 3)
    hb = HitGraphBatch.from_graphs(graphs).to("cuda")
    qm = quantize_model(_model(3, 8, 3, 3.0), FixedPointFormat(16, 3, "rnd", "wrap", 10))
    a, b = qm(hb, trace=True), qm(hb, trace=True)
    assert a.counts.sum().item() > 0
    for k in ("raw", "scores", "counts", "e_trace", "H_trace"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def test_rebuilt_when_the_weights_change(hip):
    graphs, _ = _graphs("layered", 3)
    g = graphs[0]
    hb = HitGraphBatch.from_graphs(graphs).to("cuda")
    model = _model(3, 8, 2)
    f = FixedPointFormat(16, 6)
    qm = quantize_model(model, f)
    first = qm(hb).raw.cpu().numpy()
    with torch.no_grad():
        model.edge_network.network[2].weight.mul_(-1.5)          # in place: the parameter's version moves
    want = fixed_forward_numpy(g.X, g.src, g.dst, fc.host_weights(model), 2, f)
    second = qm(hb).raw.cpu().numpy()
    assert np.array_equal(second, want.raw) and not np.array_equal(first, second)
    with pytest.raises(RuntimeError, match="ROCm device"):
        qm(HitGraphBatch.from_graphs(graphs))                     # a host batch: there is no CPU path
    with torch.no_grad():
        model.input_network[0].bias[0] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        qm(hb)


def test_inputs_that_are_not_finite(hip):
    """X is quantised on the device: NaN becomes 0, +-Inf saturates, and ties round to even as rint does."""
    g = fc.layered(70, 150, 3, 1)
    X = g.X.copy()
    X[0], X[1, 0], X[2, 1] = (np.nan, np.inf, -np.inf), 1e30, -1e30
    X[3] = (0.5 / 1024, 1.5 / 1024, -2.5 / 1024)                  # ties at Fb = 10
    hb = HitGraphBatch.from_graphs([HitGraph(X, g.src, g.dst, g.y)])
    model = _model(3, 8, 1)
    f = FixedPointFormat(16, 6, overflow="sat")
    want = fixed_forward_numpy(X, g.src, g.dst, fc.host_weights(model), 1, f)
    assert want.H_trace[0, 0, 8:].tolist() == [0, f.hi, f.lo] and want.H_trace[0, 3, 8:].tolist() == [0, 2, -2]
    _assert_bits(quantize_model(model, f)(hb.to("cuda"), trace=True), want)


def test_list_length_bound_on_the_device(hip):
    """At 24 bits a list of 131 072 entries is refused (one read-back of the longest list); one entry fewer runs."""
    f = FixedPointFormat(24, 8)
    n = f.max_list_entries
    X = np.random.default_rng(0).uniform(-1, 1, size=(3, 3)).astype(np.float32)
    src, dst = np.ones(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    model = _model(3, 8, 1)
    qm = quantize_model(model, f)
    with pytest.raises(ValueError, match="131072"):
        qm(HitGraphBatch.from_graphs([HitGraph(X, src, dst, None)]).to("cuda"))
    out = qm(HitGraphBatch.from_graphs([HitGraph(X, src[:-1], dst[:-1], None)]).to("cuda"), trace=True)
    _assert_bits(out, fixed_forward_numpy(X, src[:-1], dst[:-1], fc.host_weights(model), 1, f))


def test_scores_feed_segment_metrics(hip):
    graphs, pad = _graphs("block3_padded", 3)
    hb = HitGraphBatch.from_graphs(graphs, pad_segments=pad)
    model = _model(3, 8, 3)
    f = FixedPointFormat(12, 4)
    want = fixed_forward_numpy(hb.X.numpy(), hb.src.numpy(), hb.dst.numpy(), fc.host_weights(model), 3, f)
    th = (0.3, 0.5)
    src = hb.src.numpy().copy()
    host = segment_metrics_numpy(want.scores, hb.y.numpy(), th, src=src)["counts"]
    dev = hb.to("cuda")
    out = quantize_model(model, f)(dev)
    m = SegmentMetrics(thresholds=th)
    m.update(out.scores, dev.y, batch=dev)
    c = m.compute()
    assert c["n"] == int((src >= 0).sum()) == int(host[0].sum())
    assert c["tp"].tolist() == host[1:, 1].tolist() and c["fp"].tolist() == host[1:, 0].tolist()


def test_scan_precision_rows(hip):
    model = _model(3, 8, 3)
    items = []
    for seed in (1, 2):
        g = fc.layered(70, 150, 3, seed)
        b = HitGraphBatch.from_graphs([g]).to("cuda")
        items.append((b, b.y))
    formats = [FixedPointFormat(16, 6), FixedPointFormat(8, 3, "rnd", "sat", 8)]
    th = (0.4, 0.5)
    rows = scan_precision(model, items, formats, thresholds=th)
    assert [r["format"] for r in rows] == formats
    with torch.no_grad():
        floats = [model(b).reshape(-1) for b, _ in items]
    for row, f in zip(rows, formats):
        qm = quantize_model(model, f)
        m = SegmentMetrics(thresholds=th)
        over, worst = np.zeros(6, dtype=np.int64), 0.0
        for (b, y), ref in zip(items, floats):
            out = qm(b)
            m.update(out.scores, y, batch=b)
            over += out.counts.cpu().numpy().sum(axis=0)
            worst = max(worst, float((out.scores - ref).abs().max().item()))
        c = m.compute()
        for k in ("tp", "fp", "tn", "fn", "accuracy", "precision", "recall"):
            assert np.array_equal(row[k], c[k]), k
        assert row["n"] == c["n"] == 300 and row["auc"] == m.auc()[0]
        assert np.array_equal(row["overflows"], over) and row["max_abs_diff"] == worst and 0 < worst < 0.2
