"""CPU checks of the segment metrics (gnn-fpga_amd/metrics.py): the specification against sklearn, the AUC bound,
zero divisions, merge / reset, input checks, the golden records, and the ABI 7 entry points that need no GPU."""
import os

import numpy as np
import pytest
import torch

from gnn_fpga_amd import HitGraphBatch, SegmentMetrics, synth
from gnn_fpga_amd.batcher import merge_graphs
from gnn_fpga_amd.metrics import bin_edges, key_shift_for, n_bins_for, segment_metrics_numpy

# the trapezoid and roc_auc_score sum different point sets: when no bin holds both classes the bound is 0 and the
# two float64 sums may still differ in the last bits
AUC_ULPS = 8 * np.finfo(np.float64).eps
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "metrics")
THRESHOLDS = (0.5, 0.25, 0.75, 0.0, float(np.float32(0.5) + np.float32(2 ** -24)))


def adversarial(seed, n=4000):
    """Scores exactly at thresholds and at bin edges, 0.0, 1.0, subnormals and ties."""
    rng = np.random.default_rng(seed)
    e = rng.random(n, dtype=np.float32)
    edges = (rng.integers(0x30000000, 0x3F800000, 300).astype(np.uint32) & np.uint32(0xFFFFFC00)).view(np.float32)
    special = np.concatenate([np.float32(THRESHOLDS), np.float32([0.0, 1.0, 1e-45, 1e-40, 2 ** -126, -0.0]), edges])
    e[:special.size] = special
    e[special.size:special.size + 300] = np.float32(0.5)
    rng.shuffle(e)
    y = (rng.random(n) < 0.2 + 0.6 * e).astype(np.float32)
    return e, y


def host_metrics(e, y, thresholds=THRESHOLDS, bpo=1024, **kw):
    m = SegmentMetrics(thresholds, bins_per_octave=bpo, device="cpu")
    m.update(e, y, **kw)
    return m


def check_roc_points(fpr, tpr, thr, sk_fpr, sk_tpr, sk_thr):
    """Each point at threshold t equals sklearn's point at the smallest of its thresholds >= t (same `e >= t` set)."""
    assert thr[0] == np.inf and fpr[0] == 0 and tpr[0] == 0
    assert np.all(np.diff(thr) < 0)
    for f, t, h in zip(fpr[1:], tpr[1:], thr[1:]):
        i = np.flatnonzero(sk_thr >= h)[-1]
        assert f == sk_fpr[i] and t == sk_tpr[i], (h, f, t, sk_fpr[i], sk_tpr[i])
    assert fpr[-1] == 1.0 and tpr[-1] == 1.0


@pytest.mark.parametrize("bpo", [1, 1024, 8192])
@pytest.mark.parametrize("seed", [0, 1])
def test_specification_agrees_with_sklearn(bpo, seed):
    skm = pytest.importorskip("sklearn.metrics")
    e, y = adversarial(seed)
    m = host_metrics(e, y, bpo=bpo)
    r = m.compute()
    assert r["n"] == e.size and r["n_pos"] == int(y.sum())
    for k, t in enumerate(THRESHOLDS):
        pred = e > np.float32(t)
        assert r["accuracy"][k] == skm.accuracy_score(y, pred)
        assert r["precision"][k] == skm.precision_score(y, pred, zero_division=0.0)
        assert r["recall"][k] == skm.recall_score(y, pred, zero_division=0.0)
        assert r["tp"][k] + r["fp"][k] + r["tn"][k] + r["fn"][k] == e.size
    check_roc_points(*m.roc(), *skm.roc_curve(y, e, drop_intermediate=False))
    auc, bound = m.auc()
    assert abs(auc - skm.roc_auc_score(y, e)) <= bound + AUC_ULPS
    if bpo == 8192:                     # (the 300 exact ties at 0.5 alone give about 0.0028)
        assert bound < 0.004


def test_auc_bound_holds_on_clustered_scores():
    skm = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(5)
    y = (rng.random(20000) < 0.3).astype(np.float32)
    e = (1 / (1 + np.exp(-np.where(y == 1, rng.normal(3, 3, y.size), rng.normal(-3, 3, y.size))))).astype(np.float32)
    for bpo in (1, 16, 1024):
        auc, bound = host_metrics(e, y, bpo=bpo).auc()
        assert abs(auc - skm.roc_auc_score(y, e)) <= bound + AUC_ULPS


def test_histogram_keys_and_edges():
    for bpo in (1, 2, 1024, 8192):
        ks = key_shift_for(bpo)
        assert n_bins_for(ks) == (0x3F800000 >> ks) + 1
        edges = bin_edges(ks)
        assert edges[0] == 0.0 and edges[-1] == 1.0 and np.all(np.diff(edges) > 0)
    assert n_bins_for(key_shift_for(1024)) == 130049 and n_bins_for(key_shift_for(8192)) == 1040385
    # every score lands in the bin whose edges enclose it
    e = np.float32([0.0, -0.0, 1e-45, 0.3, 0.5, np.nextafter(np.float32(0.5), np.float32(0)), 1.0])
    spec = segment_metrics_numpy(e, np.zeros_like(e), bins_per_octave=64)
    edges = bin_edges(key_shift_for(64))
    b = np.repeat(np.arange(edges.size), spec["hist"][0])
    assert np.all(edges[b] <= np.sort(e)) and np.all((b + 1 == edges.size) | (np.sort(e) < edges[np.minimum(b + 1, edges.size - 1)]))


def test_zero_division_is_zero():
    e = np.float32([0.1, 0.2, 0.3])
    r = host_metrics(e, np.zeros(3, np.float32), thresholds=(0.5, 0.15)).compute()
    assert r["precision"][0] == 0.0 and r["recall"][0] == 0.0 and r["accuracy"][0] == 1.0     # nothing predicted, P = 0
    assert r["precision"][1] == 0.0 and r["recall"][1] == 0.0
    r = host_metrics(np.float32([]), np.float32([])).compute()
    assert r["n"] == 0 and r["accuracy"][0] == 0.0 and r["precision"][0] == 0.0
    fpr, tpr, thr = host_metrics(e, np.ones(3, np.float32)).roc()
    assert np.all(np.isnan(fpr)) and tpr[-1] == 1.0                                        # sklearn: NaN FPR, N = 0
    assert all(np.isnan(v) for v in host_metrics(e, np.ones(3, np.float32)).auc())


def test_merge_and_reset():
    e, y = adversarial(3)
    whole = host_metrics(e, y)
    a, b = host_metrics(e[:1500], y[:1500]), host_metrics(e[1500:], y[1500:])
    assert torch.equal(a.merge(b).counts, whole.counts)
    streamed = SegmentMetrics(THRESHOLDS, device="cpu")
    for s in (slice(0, 1000), slice(1000, 1001), slice(1001, None)):
        streamed.update(e[s], y[s])
    assert torch.equal(streamed.counts, whole.counts)
    with pytest.raises(ValueError):
        a.merge(SegmentMetrics((0.5,), device="cpu"))
    with pytest.raises(ValueError):
        a.merge(SegmentMetrics(THRESHOLDS, bins_per_octave=8, device="cpu"))
    a.reset()
    assert int(a.counts.abs().sum()) == 0 and a.compute()["n"] == 0


def test_input_validation():
    for th in ((), tuple(np.linspace(0, 1, 17)), (0.5, float("nan")), (float("inf"),)):
        with pytest.raises(ValueError):
            SegmentMetrics(th, device="cpu")
    for bpo in (0, 3, 16384, 1.5):
        with pytest.raises(ValueError):
            SegmentMetrics(bins_per_octave=bpo, device="cpu")
    m = SegmentMetrics(device="cpu")
    with pytest.raises(ValueError):
        m.update(np.zeros(3, np.float32), np.zeros(4, np.float32))
    with pytest.raises(ValueError):
        m.update(np.zeros(3, np.float32), np.zeros(3, np.float32), per_graph=True)
    g = synth.layered_graph(30, 60, 3, seed=1)
    with pytest.raises(ValueError):
        m.update(np.zeros(59, np.float32), np.zeros(59, np.float32), batch=HitGraphBatch(g.X, g.src, g.dst))
    assert segment_metrics_numpy([0.5], [1.0], thresholds=(float("nan"),))["status"] == 4


@pytest.mark.parametrize("bad", ["nan", "label", "above_one"])
def test_bad_input_raises_until_reset(bad):
    e, y = np.float32([0.1, 0.9, 0.5]), np.float32([0, 1, 1])
    e2, y2 = e.copy(), y.copy()
    if bad == "nan":
        e2[1] = np.nan
    elif bad == "label":
        y2[0] = 0.5
    else:
        e2[2] = 1.5
    m = SegmentMetrics(device="cpu")
    m.update(e2, y2)
    m.update(e, y)
    for _ in range(2):
        with pytest.raises(ValueError):
            m.compute()
    with pytest.raises(ValueError):
        m.roc()
    m.reset()
    m.update(e, y)
    assert m.compute()["n"] == 3


def test_padding_and_per_graph_on_the_host():
    graphs = [synth.layered_graph(40, 90, 3, seed=s) for s in range(3)]
    graphs.insert(1, synth.HitGraph(graphs[0].X[:5], np.zeros(0, np.int32), np.zeros(0, np.int32),
                                    np.zeros(0, np.float32)))
    b, y = merge_graphs(graphs, "padded")
    rng = np.random.default_rng(0)
    e = rng.random(b.n_segments, dtype=np.float32)
    m = SegmentMetrics((0.3, 0.6), device="cpu")
    pg = m.update(e, y, batch=b, per_graph=True).numpy()
    assert pg.shape == (4, 3, 2) and np.all(pg[1] == 0)
    assert pg[:, 0].sum() == sum(g.src.shape[0] for g in graphs)
    c = m.counts[1:7].view(3, 2).numpy()
    assert np.array_equal(pg.sum(0), c)
    for gi, g in enumerate(graphs):
        s = slice(int(b.seg_ptr[gi]), int(b.seg_ptr[gi]) + g.src.shape[0])
        assert pg[gi, 0, 1] == int(g.y.sum()) and pg[gi, 1, 1] == int(((e[s] > np.float32(0.3)) & (g.y == 1)).sum())
    with_pad = SegmentMetrics((0.3, 0.6), device="cpu")
    with_pad.update(e, y, batch=b, include_padding=True)
    assert with_pad.compute()["n"] == b.n_segments


def test_score_histogram_is_close():
    e, y = adversarial(4)
    counts, edges = host_metrics(e, y, bpo=1024).score_histogram(20)
    exact = np.stack([np.histogram(e[y == c], bins=edges)[0] for c in (0, 1)])
    assert counts.sum() == e.size and np.abs(counts - exact).sum() <= 0.01 * e.size


@pytest.mark.parametrize("name", ["adversarial_s0", "clustered_s1", "fixture_c2_scale", "fixture_sector_d64"])
def test_specification_matches_golden_sklearn_records(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    th = tuple(float(t) for t in z["thresholds"])
    m = host_metrics(z["scores"], z["labels"], thresholds=th, bpo=1024)
    r = m.compute()
    for k in ("accuracy", "precision", "recall"):
        assert np.all(np.abs(r[k] - z[k]) <= np.spacing(z[k])), k
    check_roc_points(*m.roc(), z["roc_fpr"], z["roc_tpr"], z["roc_thresholds"])
    auc, bound = m.auc()
    assert abs(auc - float(z["roc_auc"])) <= bound + AUC_ULPS


def test_abi7_entry_points_without_a_gpu():
    from gnn_fpga_amd import _lib
    assert _lib.GNN_ABI_VERSION == 7
    lib = _lib.load()
    assert lib.gnn_abi_version() == 7
    for bpo in (1, 1024, 8192):
        assert _lib.metrics_bins(key_shift_for(bpo)) == n_bins_for(key_shift_for(bpo))
    assert _lib.metrics_bins(9) == 0 and _lib.metrics_bins(24) == 0
    assert lib.gnn_metrics_workspace_bytes(1 << 31, 16, 10, 1000) == 0
    assert lib.gnn_segment_metrics_update(None, None, None, -1, None, 1, 13, None, None, None, 0, None, None, None,
                                          0, None) == _lib.GNN_ERR_BADARG


def test_merge_keeps_the_kind_of_bad_input():
    """merge ORs the status words (a sum would turn two 'bad score' words into 'bad label')."""
    bad = np.float32([0.1, np.nan]), np.float32([0, 1])
    a, b = SegmentMetrics(device="cpu"), SegmentMetrics(device="cpu")
    a.update(*bad)
    b.update(*bad)
    a.merge(b)
    assert int(a.counts[:1].view(torch.int32)[0]) == 1
    with pytest.raises(ValueError, match="score") as err:
        a.compute()
    assert "label" not in str(err.value)
