"""gnn_fxev_forward (include/gnn_hip_fixed_events.h): the fixed-point forward of a batch of small graphs in one launch,
against the numpy specification `fixed_forward_numpy`, bit for bit - raw scores, both traces, the overflow counters,
scores == raw * 2^-Fb - and the per-graph overflow counts against the specification run on every graph's slice alone.
No tolerance anywhere: the arithmetic is integers.  Then the route through `quantize_model(...)(batch)` and
`scan_precision`, against the per-module kernels (_lib.fx_forward).

Each axis varies with the others at DEFAULT, then a handful of crossed cases; `gain` scales every weight of torch's
default initialisation so that every stage overflows."""
import types

import numpy as np
import pytest
import torch

import fixed_events_cases as fe
import fixed_point_cases as fc
from gnn_fpga_amd import FixedPointFormat, HitGraph, HitGraphBatch, quantize_model, scan_precision, synth

pytestmark = pytest.mark.gpu

#          batch     F   D  T   W  I  rounding overflow tb  gain
DEFAULT = ("muon64", 11, 8, 3, 16, 6, "trn", "wrap", 10, 1.0)
NAMES = ("graph", "F", "D", "T", "W", "I", "rounding", "overflow", "tb", "gain")


def _vary(**kw):
    case = dict(zip(NAMES, DEFAULT))
    case.update(kw)
    return tuple(case[n] for n in NAMES)


CASES = (
    [_vary(graph=g, F=F) for g, F in [("block3_padded", 3), ("toy32", 2), ("single", 11), ("mixed600", 11),
                                      ("mixed600_padded", 11)]] +
    [_vary(F=F, D=D) for F, D in [(11, 8), (11, 16), (3, 8), (4, 16), (2, 4)]] + [_vary(graph="toy32", F=2, D=32)] +
    [_vary(T=T) for T in (0, 1, 17)] +
    [_vary(W=W, I=I) for W, I in [(24, 8), (8, 3), (6, 4), (24, 2), (12, 12)]] +
    [_vary(rounding=r, overflow=o) for r, o in [("trn", "sat"), ("rnd", "wrap"), ("rnd", "sat")]] +
    [_vary(tb=tb) for tb in (4, 12)] +
    [("muon64", 11, 8, 3, 24, 2, "trn", "wrap", 10, 2.0),
     ("muon64", 11, 8, 3, 24, 2, "rnd", "sat", 10, 2.0),
     ("muon64", 11, 16, 2, 24, 2, "rnd", "wrap", 10, 2.0),
     ("mixed600_padded", 11, 16, 2, 24, 2, "rnd", "wrap", 8, 2.0),
     ("mixed600", 11, 16, 2, 24, 2, "trn", "sat", 8, 2.0),
     ("block3_padded", 3, 8, 2, 16, 3, "rnd", "sat", 12, 2.0),
     ("toy32", 2, 32, 10, 12, 4, "rnd", "wrap", 7, 3.0),
     ("block3_padded", 4, 16, 1, 6, 4, "trn", "wrap", 5, 4.0)]
)


def _assert_bits(got, want, what=""):
    """got: (raw, scores, counts, graph_overflows, e_trace, H_trace) of _lib.fxev_forward(trace=True)."""
    raw, scores, counts, _, et, Ht = (t.cpu().numpy() for t in got)
    assert raw.dtype == np.int32 and scores.dtype == np.float32 and counts.dtype == np.int64
    for name, g, w in (("counts", counts, want.counts), ("H_trace", Ht, want.H_trace), ("e_trace", et, want.e_trace),
                       ("raw", raw, want.raw)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
        assert bad.size == 0, "%s %s: %d of %d differ, first at %d: %d != %d" % (
            what, name, bad.size, w.size, bad[0], g.reshape(-1)[bad[0]], w.reshape(-1)[bad[0]])
    assert np.array_equal(scores.view(np.uint32), want.scores.view(np.uint32))
    assert np.array_equal(scores.astype(np.float64), raw.astype(np.float64) * 2.0 ** -want.fmt.frac_bits)
    return counts


def _assert_per_graph(got, hb, weights, T, f):
    """graph_overflows against the specification on every graph's slice; they add up to the counters."""
    per_graph = got[3].cpu().numpy()
    want = np.array([int(p.counts.sum()) for p in fe.spec_per_graph(hb, weights, T, f)], dtype=np.int64)
    assert per_graph.dtype == np.int64 and np.array_equal(per_graph, want)
    assert int(per_graph.sum()) == int(got[2].sum().item())
    return per_graph


def _run(case, hip):
    kind, F, D, T, W, I, rounding, overflow, tb, gain = case
    f = FixedPointFormat(W, I, rounding, overflow, tb)
    hb = fe.host_batch(kind, F)
    weights = fe.gained(F, D, T, gain)
    want = fe.spec(hb, weights, T, f)
    dev = fe.host_batch(kind, F).to("cuda")
    lay = dev.event_layout()
    assert lay is not None and hip.fxev_supported(F, D, tb, lay.max_hits, lay.max_segments)
    params, fmt, tables = fe.device_args(weights, f, F, D)
    got = hip.fxev_forward(dev, lay, params, fmt, tables, T, trace=True)
    counts = _assert_bits(got, want, str(case))
    per_graph = _assert_per_graph(got, hb, weights, T, f)
    plain = hip.fxev_forward(dev, lay, params, fmt, tables, T)
    assert plain[4] is None and plain[5] is None
    for a, b in zip(plain[:4], got[:4]):
        assert torch.equal(a, b)
    return counts, per_graph, hb


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_bit_equal_to_the_specification(hip, case):
    counts, per_graph, hb = _run(case, hip)
    print("overflows per stage:", counts.sum(axis=0).tolist(), "graphs with one:", int((per_graph > 0).sum()))
    if case[0].startswith("mixed600"):
        sizes = np.diff(hb.hit_ptr) + np.diff(hb.seg_ptr)
        assert per_graph[100] == 0 or case[0] == "mixed600_padded"      # (padded segments can overflow like any other)
        assert np.all(per_graph[sizes == 0] == 0) and hb.hit_ptr[101] == hb.hit_ptr[100]
        if case[5] == 2:
            assert (per_graph > 0).any() and (per_graph == 0).any()
    if case[0] == "block3_padded":
        assert int((hb.src.numpy() < 0).sum()) > 100 and int(np.diff(hb.hit_ptr).max()) > 64


@pytest.mark.parametrize("D,T", [(8, 3), (16, 2)])
def test_every_stage_overflows_in_both_modes(hip, D, T):
    """Asserted on the SPECIFICATION, so that the bit-equality of the crossed cases above is not one of idle branches:
    at (24, 2) with the weights doubled every one of the six stage totals is positive, wrapping and saturating."""
    hb, w = fe.host_batch("muon64", 11), fe.gained(11, D, T, 2.0)
    for overflow in ("wrap", "sat"):
        f = FixedPointFormat(24, 2, "trn", overflow, 10)
        want = fe.spec(hb, w, T, f)
        assert np.all(want.counts.sum(axis=0) > 0), (overflow, want.counts.sum(axis=0))
        dev = HitGraphBatch.from_graphs(list(fe.muon(64))).to("cuda")
        got = hip.fxev_forward(dev, dev.event_layout(), *fe.device_args(w, f, 11, D), T, trace=True)
        _assert_bits(got, want, overflow)


# ---- the LDS boundary ----------------------------------------------------------------------------------------------------
def _largest(ok):
    lo, hi = 1, 1 << 20         # ok(lo), not ok(hi)
    assert ok(lo) and not ok(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return lo


def _one_graph(hip, n_hits, n_segments, T=1):
    """A layered graph of exactly that size through gnn_fxev_forward with max_hits / max_segments = its size (the
    package's own layout stops at _lib.EVENTS_MAX_SEGMENTS: the entry point itself is asked here)."""
    g = synth.layered_graph(n_hits, n_segments, 3, seed=7)
    assert g.X.shape[0] == n_hits and g.src.shape[0] == n_segments
    hb = HitGraphBatch.from_graphs([g])
    f = FixedPointFormat(16, 6, "trn", "wrap", 12)
    w = fe.gained(3, 8, T)
    dev = HitGraphBatch.from_graphs([g]).to("cuda")
    ptrs = torch.tensor([[0, n_hits], [0, n_segments]], dtype=torch.int32, device="cuda")
    lay = types.SimpleNamespace(hit_ptr=ptrs[0], seg_ptr=ptrs[1], max_hits=n_hits, max_segments=n_segments)
    return hip.fxev_forward(dev, lay, *fe.device_args(w, f, 3, 8), T, trace=True), fe.spec(hb, w, T, f)


def test_the_largest_graph_that_fits(hip):
    e_star = _largest(lambda e: hip.fxev_supported(3, 8, 12, 64, e))
    n_star = _largest(lambda n: hip.fxev_supported(3, 8, 12, n, 100))
    print("(3, 8), 12 table bits: 64 hits take %d segments, 100 segments take %d hits" % (e_star, n_star))
    assert hip.fxev_lds_bytes(3, 8, 12, 64, e_star) <= 160 * 1024 < hip.fxev_lds_bytes(3, 8, 12, 64, e_star + 1)
    assert e_star < 7000                # (the header's statement on the exactness bound)
    for n_hits, n_segments in ((64, e_star), (n_star, 100)):
        _assert_bits(*_one_graph(hip, n_hits, n_segments), what=str((n_hits, n_segments)))
    for n_hits, n_segments in ((64, e_star + 1), (n_star + 1, 100)):
        with pytest.raises(hip.GnnHipError) as exc:          # refused before any launch
            _one_graph(hip, n_hits, n_segments)
        need = hip.fxev_lds_bytes(3, 8, 12, n_hits, n_segments)
        assert need > 160 * 1024 and str(need) in str(exc.value) and str(160 * 1024) in str(exc.value)


# ---- X that is not finite, reproducibility ---------------------------------------------------------------------------------
def test_inputs_that_are_not_finite(hip):
    """X is quantised in the kernel: NaN becomes 0, +-Inf and +-1e30 saturate, ties round to even as rint does."""
    g = fc.layered(70, 150, 3, 1)
    X = g.X.copy()
    X[0], X[1, 0], X[2, 1] = (np.nan, np.inf, -np.inf), 1e30, -1e30
    X[3] = (0.5 / 1024, 1.5 / 1024, -2.5 / 1024)                  # ties at Fb = 10
    graphs = [HitGraph(X, g.src, g.dst, g.y), fc.layered(33, 41, 3, 2)]
    hb = HitGraphBatch.from_graphs(graphs)
    f = FixedPointFormat(16, 6, overflow="sat")
    w = fe.gained(3, 8, 1)
    want = fe.spec(hb, w, 1, f)
    assert want.H_trace[0, 0, 8:].tolist() == [0, f.hi, f.lo] and want.H_trace[0, 3, 8:].tolist() == [0, 2, -2]
    assert want.H_trace[0, 1, 8] == f.hi and want.H_trace[0, 2, 9] == f.lo
    dev = HitGraphBatch.from_graphs(graphs).to("cuda")
    _assert_bits(hip.fxev_forward(dev, dev.event_layout(), *fe.device_args(w, f, 3, 8), 1, trace=True), want)


def test_two_runs_give_the_same_bits(hip):
    dev = HitGraphBatch.from_graphs(list(fe.muon(64))).to("cuda")
    args = fe.device_args(fe.gained(11, 8, 3, 2.0), FixedPointFormat(24, 2, "rnd", "wrap", 10), 11, 8)
    a = hip.fxev_forward(dev, dev.event_layout(), *args, 3, trace=True)
    b = hip.fxev_forward(dev, dev.event_layout(), *args, 3, trace=True)
    assert a[2].sum().item() > 0 and a[3].sum().item() > 0
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---- the route through quantize_model ------------------------------------------------------------------------------------
def _model(F, D, T, gain=1.0):
    m = fc.default_model(F, D, T)
    if gain != 1.0:
        with torch.no_grad():
            for p in m.parameters():
                p.mul_(gain)
    return m.cuda()


def _per_module(hip, qm, dev):
    """The parent's kernels on the same batch: what every route must equal."""
    params, tables, fmt = qm._ensure()
    return hip.fx_forward(dev, params, fmt, tables, qm.model.n_iters)[:3]


def _same(out, ref):
    return all(torch.equal(a, b) for a, b in zip((out.raw, out.scores, out.counts), ref))


@pytest.mark.parametrize("kind,F,D", [("muon64", 11, 8), ("mixed600_padded", 11, 16), ("block3_padded", 3, 8),
                                      ("toy32", 2, 32), ("single", 11, 8)])
def test_small_batches_take_the_events_route(hip, kind, F, D):
    f = FixedPointFormat(24, 2, "rnd", "wrap", 10)
    qm = quantize_model(_model(F, D, 2, 2.0), f)
    hb = fe.host_batch(kind, F)
    dev = fe.host_batch(kind, F).to("cuda")
    out = qm(dev)
    assert qm.last_route == "events" and out.e_trace is None and out.H_trace is None and out.fmt == f
    assert out.event_overflows is not None and out.event_overflows.dtype == torch.int64
    assert out.event_overflows.shape == (hb.n_graphs,) and out.event_overflows.is_cuda
    assert out.counts.sum().item() > 0 and int(out.event_overflows.sum().item()) == int(out.counts.sum().item())
    assert _same(out, _per_module(hip, qm, dev))
    traced = qm(dev, trace=True)
    assert qm.last_route == "per_module" and traced.event_overflows is None and traced.e_trace is not None
    assert _same(traced, (out.raw, out.scores, out.counts))
    qm.use_events = False
    forced = qm(dev)
    assert qm.last_route == "per_module" and forced.event_overflows is None and _same(forced, (out.raw, out.scores, out.counts))


def _crossed():
    """Two graphs, one segment of the first ending in the second: no event layout."""
    hb = HitGraphBatch.from_graphs([fc.layered(70, 150, 3, 1), fc.layered(33, 41, 3, 2)])
    hb.dst[0] = int(hb.hit_ptr[1]) + 5
    return hb


@pytest.mark.parametrize("what,F,D,make", [
    ("a 5000-hit graph", 3, 8, lambda: HitGraphBatch.from_graphs([synth.layered_graph(5000, 1100, 3, seed=3)])),
    ("hidden_dim 64", 3, 64, lambda: HitGraphBatch.from_graphs([fc.layered(70, 150, 3, 1)])),
    ("the star at (2, 32)", 2, 32, lambda: HitGraphBatch.from_graphs([fc.cached_star(0, 2)])),
    ("a segment between two graphs", 3, 8, _crossed),
], ids=lambda v: v.replace(" ", "_") if isinstance(v, str) else None)
def test_what_does_not_fit_runs_per_module(hip, what, F, D, make):
    f = FixedPointFormat(16, 6)
    model = _model(F, D, 2)
    qm = quantize_model(model, f)
    host = make()
    want = fe.spec(host, fc.host_weights(model), 2, f)
    dev = make().to("cuda")
    out = qm(dev)
    assert qm.last_route == "per_module" and out.event_overflows is None, what
    assert np.array_equal(out.raw.cpu().numpy(), want.raw) and np.array_equal(out.counts.cpu().numpy(), want.counts)
    assert np.array_equal(out.scores.cpu().numpy().view(np.uint32), want.scores.view(np.uint32))
    lay = dev.event_layout()
    if what == "a segment between two graphs":
        assert lay is None
    else:       # a layout, but no room in a workgroup's LDS
        assert lay is not None and not hip.fxev_supported(F, D, f.table_bits, lay.max_hits, lay.max_segments)


# ---- scan_precision --------------------------------------------------------------------------------------------------------
def test_scan_precision_counts_the_events_that_overflow(hip):
    model = _model(11, 8, 2, 2.0)
    w = fc.host_weights(model)
    groups = [list(fe.muon(64))[:32], list(fe.muon(64))[32:]]
    items = []
    for gs in groups:
        b = HitGraphBatch.from_graphs(gs).to("cuda")
        items.append((b, b.y))
    formats = [FixedPointFormat(16, 6), FixedPointFormat(24, 2, "rnd", "wrap", 10), FixedPointFormat(12, 3, "trn", "sat", 8)]
    rows = scan_precision(model, items, formats)
    base = scan_precision(model, items, formats, use_events=False)
    for row, ref, f in zip(rows, base, formats):
        want = sum(int(p.counts.sum() > 0) for gs in groups
                   for p in fe.spec_per_graph(HitGraphBatch.from_graphs(gs), w, 2, f))
        assert row["events_overflowed"] == want and ref["events_overflowed"] is None, (f, row["events_overflowed"], want)
        assert set(row) == set(ref)
        for k in set(row) - {"events_overflowed"}:
            assert np.array_equal(row[k], ref[k]) if isinstance(row[k], np.ndarray) else row[k] == ref[k], k
    assert rows[0]["events_overflowed"] < rows[1]["events_overflowed"] <= 64
    # one detector-size batch among them: that format's count is not known
    big = HitGraphBatch.from_graphs([synth.layered_graph(5000, 20000, 11, seed=1)]).to("cuda")
    mixed = scan_precision(model, items + [(big, big.y)], formats[:1])
    assert mixed[0]["events_overflowed"] is None and mixed[0]["n"] == rows[0]["n"] + 20000
