"""GPU checks of the segment metrics kernel (csrc/metrics.hip through gnn-fpga_amd/metrics.py): bit-for-bit against
segment_metrics_numpy, against the golden sklearn records, streaming, run-to-run identity, evaluate() over
batch_generator output, 64-bit counters past 2^32, and bad input raising from compute() without a fault."""
import os

import numpy as np
import pytest
import torch

from gnn_fpga_amd import SegmentMetrics, batch_generator, evaluate, synth
from gnn_fpga_amd.metrics import segment_metrics_numpy
from gnn_fpga_amd.model import SegmentClassifier

pytestmark = pytest.mark.gpu

# the trapezoid and roc_auc_score sum different point sets: when no bin holds both classes the bound is 0 and the
# two float64 sums may still differ in the last bits
AUC_ULPS = 8 * np.finfo(np.float64).eps
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "metrics")
DEV = torch.device("cuda", 0)
THRESHOLDS = (0.5, 0.25, 0.75, 0.0, 1.0, 1e-3, 0.999, float(np.float32(0.5) + np.float32(2 ** -24)))


def scores(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        e = rng.random(n, dtype=np.float32)
    elif kind == "clustered":                                  # sigmoid of normals: piles near 1, spread near 0
        e = (1 / (1 + np.exp(-rng.normal(0, 8, n)))).astype(np.float32)
    else:                                                      # adversarial: thresholds, edges, 0, 1, subnormals, ties
        e = rng.random(n, dtype=np.float32)
        pick = rng.integers(0, 6, n)
        edges = (rng.integers(0, 0x3F800000, n).astype(np.uint32) & np.uint32(0xFFFFFC00)).view(np.float32)
        e = np.where(pick == 0, np.float32(THRESHOLDS)[rng.integers(0, len(THRESHOLDS), n)], e)
        e = np.where(pick == 1, edges, e)
        e = np.where(pick == 2, np.float32([0.0, 1.0, 1e-45, 1e-40, 2 ** -126, -0.0])[rng.integers(0, 6, n)], e)
        e = np.where(pick == 3, np.float32(0.123), e).astype(np.float32)
    y = (rng.random(n) < 0.3 + 0.4 * e).astype(np.float32)
    return e, y


def ragged_seg_ptr(n, seed, n_graphs=300):
    """Graph boundaries with empty graphs among them, some graphs much longer than a kernel tile."""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.integers(0, n + 1, n_graphs - 1))
    cuts[: n_graphs // 10] = cuts[n_graphs // 10]               # a run of empty graphs
    return np.concatenate([[0], cuts, [n]]).astype(np.int64)


def kernel_update(e, y, src=None, seg_ptr=None, bpo=1024, thresholds=THRESHOLDS, m=None):
    from gnn_fpga_amd import _lib
    m = m or SegmentMetrics(thresholds, bins_per_octave=bpo, device=DEV)
    status, counts, hist = m._views()
    t = lambda a, dt: torch.as_tensor(a).to(DEV, dt)   # noqa: E731
    pg = None
    if seg_ptr is not None:
        pg = torch.full((seg_ptr.size - 1, len(thresholds) + 1, 2), -7, dtype=torch.int64, device=DEV)
    _lib.segment_metrics_update(t(e, torch.float32), t(y, torch.float32), None if src is None else t(src, torch.int32),
                                m.thresholds, m.key_shift, counts, hist, status,
                                None if seg_ptr is None else t(seg_ptr, torch.int64), pg)
    return m, pg


def assert_equal_to_spec(m, pg, spec):
    host = m.counts.cpu().numpy()
    assert int(host[:1].view(np.int32)[0]) == spec["status"]
    nc = 2 * (len(m.thresholds) + 1)
    assert np.array_equal(host[1:1 + nc].reshape(-1, 2), spec["counts"])
    assert np.array_equal(host[1 + nc:].reshape(2, -1), spec["hist"])
    if spec["per_graph"] is not None:
        assert np.array_equal(pg.cpu().numpy(), spec["per_graph"])


@pytest.mark.parametrize("bpo", [1, 1024, 8192])
@pytest.mark.parametrize("kind", ["uniform", "adversarial", "clustered"])
def test_kernel_equals_specification(hip, kind, bpo):
    n = 3 * 2048 * 41 + 777                                    # many tiles and a ragged tail
    e, y = scores(kind, n, seed=bpo)
    rng = np.random.default_rng(7)
    src = np.where(rng.random(n) < 0.1, -1, 0).astype(np.int32)
    sp = ragged_seg_ptr(n, seed=bpo)
    m, pg = kernel_update(e, y, src, sp, bpo)
    assert_equal_to_spec(m, pg, segment_metrics_numpy(e, y, THRESHOLDS, bpo, src, sp))
    # without src (include_padding), one threshold, and from addresses that are not 16-B aligned (scalar loads)
    m, _ = kernel_update(e, y, bpo=bpo, thresholds=(0.5,))
    assert_equal_to_spec(m, None, segment_metrics_numpy(e, y, (0.5,), bpo))
    et, yt = torch.from_numpy(e).to(DEV), torch.from_numpy(y).to(DEV)
    m1 = SegmentMetrics(THRESHOLDS, bins_per_octave=bpo, device=DEV)
    m1.update(et[1:], yt[1:])
    assert_equal_to_spec(m1, None, segment_metrics_numpy(e[1:], y[1:], THRESHOLDS, bpo))


@pytest.mark.parametrize("bpo", [1024, 8192])
@pytest.mark.parametrize("kind", ["uniform", "clustered", "narrow"])
def test_kernel_equals_specification_at_scale(hip, kind, bpo):
    """Several tiles per workgroup, as a c3 x 256 batch has: the LDS table is reused across tiles and, for spread-out
    scores, emptied mid-run (uniform: after every tile; clustered: most tiles; narrow, a pile of a few bins: never
    before the end); the per-graph search restarts on every tile; two runs give the same bits."""
    grid = torch.cuda.get_device_properties(DEV).multi_processor_count * 4          # k_metrics' grid
    n = 2048 * grid * 6 + 1234
    if kind == "narrow":
        rng = np.random.default_rng(bpo)
        e = (np.float32(0.3) + np.float32(0.01) * rng.random(n, dtype=np.float32)).astype(np.float32)
        y = (rng.random(n) < 0.4).astype(np.float32)
    else:
        e, y = scores(kind, n, seed=bpo)
    rng = np.random.default_rng(11)
    src = np.where(rng.random(n) < 0.05, -1, 0).astype(np.int32)
    sp = ragged_seg_ptr(n, seed=bpo, n_graphs=5000)
    spec = segment_metrics_numpy(e, y, THRESHOLDS, bpo, src, sp)
    m, pg = kernel_update(e, y, src, sp, bpo)
    assert_equal_to_spec(m, pg, spec)
    m2, pg2 = kernel_update(e, y, src, sp, bpo)
    assert torch.equal(m2.counts, m.counts) and torch.equal(pg2, pg)


@pytest.mark.parametrize("name", ["adversarial_s0", "clustered_s1", "fixture_c2_scale", "fixture_sector_d64"])
def test_kernel_metrics_match_golden_sklearn_records(hip, name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    m = SegmentMetrics(tuple(float(t) for t in z["thresholds"]), device=DEV)
    m.update(torch.from_numpy(z["scores"]).to(DEV), torch.from_numpy(z["labels"]).to(DEV))
    r = m.compute()
    for k in ("accuracy", "precision", "recall"):
        assert np.all(np.abs(r[k] - z[k]) <= np.spacing(z[k])), k
    fpr, tpr, thr = m.roc()
    sk_thr = z["roc_thresholds"]
    assert thr[0] == np.inf and np.all(np.diff(thr) < 0)
    for f, t, h in zip(fpr[1:], tpr[1:], thr[1:]):
        i = np.flatnonzero(sk_thr >= h)[-1]
        assert f == z["roc_fpr"][i] and t == z["roc_tpr"][i]
    auc, bound = m.auc()
    assert abs(auc - float(z["roc_auc"])) <= bound + AUC_ULPS


def test_streaming_equals_one_pass_and_runs_are_identical(hip):
    parts = [scores(k, n, s) for k, n, s in (("clustered", 100003, 1), ("adversarial", 2048, 2),
                                             ("uniform", 333333, 3))]
    streamed = SegmentMetrics(THRESHOLDS, device=DEV)
    for e, y in parts:
        streamed.update(torch.from_numpy(e).to(DEV), torch.from_numpy(y).to(DEV))
    whole = SegmentMetrics(THRESHOLDS, device=DEV)
    e = np.concatenate([p[0] for p in parts])
    y = np.concatenate([p[1] for p in parts])
    whole.update(torch.from_numpy(e).to(DEV), torch.from_numpy(y).to(DEV))
    assert torch.equal(streamed.counts, whole.counts)
    again = SegmentMetrics(THRESHOLDS, device=DEV)
    again.update(torch.from_numpy(e).to(DEV), torch.from_numpy(y).to(DEV))
    assert torch.equal(again.counts, whole.counts)
    assert_equal_to_spec(whole, None, segment_metrics_numpy(e, y, THRESHOLDS))


@pytest.mark.parametrize("include_padding", [False, True])
def test_evaluate_over_padded_batches(hip, include_padding):
    graphs = [synth.layered_graph(60 + 7 * s, 150 + 31 * s, 3, seed=s) for s in range(7)]
    graphs.insert(2, synth.HitGraph(graphs[0].X[:4], np.zeros(0, np.int32), np.zeros(0, np.int32),
                                    np.zeros(0, np.float32)))           # a graph with zero segments
    torch.manual_seed(0)
    model = SegmentClassifier(input_dim=3, hidden_dim=8, n_iters=2).to(DEV)
    m = evaluate(model, batch_generator(graphs, len(graphs), 3, device=DEV, layout="padded"), 3, THRESHOLDS,
                 include_padding=include_padding)
    assert not model.training
    # the specification on the read-back scores of the same batches
    gen = batch_generator(graphs, len(graphs), 3, device=DEV, layout="padded")
    ref = SegmentMetrics(THRESHOLDS, device="cpu")
    pgs = []
    with torch.no_grad():
        for _ in range(3):
            b, y = next(gen)
            e = model(b)
            assert b.dense_shape is not None and int((b.src < 0).sum()) > 0          # padded
            ref.update(e.cpu().numpy(), y.cpu().numpy(), batch=b, include_padding=include_padding)
            pg = SegmentMetrics(THRESHOLDS, device=DEV).update(e, y, batch=b, include_padding=include_padding,
                                                               per_graph=True)
            src = None if include_padding else b.src.cpu().numpy()
            spec = segment_metrics_numpy(e.cpu().numpy(), y.cpu().numpy(), THRESHOLDS, 1024, src, b.seg_ptr)
            assert np.array_equal(pg.cpu().numpy(), spec["per_graph"])
            pgs.append(pg)
    assert torch.equal(m.counts.cpu(), ref.counts)
    n_valid = sum(g.src.shape[0] for g in graphs)
    assert (m.compute()["n"] == n_valid) != include_padding
    # the graph with zero segments (third of the first batch): nothing, or its padded slots as fakes
    e_max = int(pgs[0][0, 0].sum())
    assert pgs[0][2, 0].tolist() == ([e_max, 0] if include_padding else [0, 0])


def test_counters_pass_two_to_the_32(hip):
    n = 1 << 27
    e = torch.full((n,), 0.375, dtype=torch.float32, device=DEV)
    y = torch.ones(n, dtype=torch.float32, device=DEV)
    m = SegmentMetrics((0.25,), device=DEV)
    for _ in range(33):
        m.update(e, y)
    del e, y
    _, counts, hist = m._views()
    key = (int(np.float32(0.375).view(np.uint32)) & 0x7FFFFFFF) >> m.key_shift
    total = 33 * n
    assert total > 1 << 32
    assert int(hist[1, key]) == total and int(hist.sum()) == total
    r = m.compute()
    assert r["n_pos"] == total and int(r["tp"][0]) == total and r["precision"][0] == 1.0


@pytest.mark.parametrize("bad", ["nan", "label", "above_one"])
def test_bad_input_raises_from_compute_without_a_fault(hip, bad):
    e, y = scores("uniform", 10000, 3)
    e2, y2 = e.copy(), y.copy()
    if bad == "nan":
        e2[4321] = np.nan
    elif bad == "label":
        y2[77] = 0.5
    else:
        e2[9999] = 1.5
    m = SegmentMetrics(THRESHOLDS, device=DEV)
    m.update(torch.from_numpy(e2).to(DEV), torch.from_numpy(y2).to(DEV))
    m.update(torch.from_numpy(e).to(DEV), torch.from_numpy(y).to(DEV))
    for _ in range(2):
        with pytest.raises(ValueError):
            m.compute()
    with pytest.raises(ValueError):
        m.auc()
    m.reset()
    m.update(torch.from_numpy(e).to(DEV), torch.from_numpy(y).to(DEV))
    assert m.compute()["n"] == e.size
    torch.cuda.synchronize()
