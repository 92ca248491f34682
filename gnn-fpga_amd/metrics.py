"""Scoring a segment classifier: confusion counts, ROC and AUC, accumulated on the GPU.

The reference's notebooks (gnn/MPNN_Seg_ACTS*.ipynb: `makeROC` and the per-sample cells) flatten
`Estimator.predict(...)` (gnn/estimator.py:137-146), read the scores back and call
`sklearn.metrics.accuracy_score / precision_score / recall_score` on `pred > thresh` and `roc_curve` on the
scores.  Here one kernel pass per batch (csrc/metrics.hip) adds into int64 counters that stay on the device:

* per class (0: y == 0, 1: y == 1): the number of segments, and the number with `e > t` at up to 16
  thresholds - exact confusion matrices, so accuracy, precision and recall are sklearn's numbers;
* per class, a histogram of the scores with relative resolution: the bin of a score in [0, 1] is its float32
  bit pattern shifted right by key_shift = 23 - log2(bins_per_octave), an order-preserving key.  Bin b holds
  the scores in [edge_b, edge_b+1), edge_b = the float32 with bit pattern b << key_shift, so the rates at every
  edge are exact: `roc()` is sklearn's curve sampled at those thresholds, fine near 0 as a log-FPR plot needs;
* optionally, per graph of a batch (`per_graph=True`), the counts of the first item.

`segment_metrics_numpy` is the specification of every counter; numpy arrays and CPU tensors take it, CUDA
tensors the kernel.  Segments with src < 0 (padding) are left out unless `include_padding=True`, which counts
them as the reference's flattened, zero-padded outputs do (label 0, the padded segment's score).  A NaN, an inf
or a score outside [0, 1], a label other than 0 / 1 or a non-finite threshold sets the status word; such
segments are counted nowhere, and `compute()` raises ValueError until `reset()`.
"""
import numpy as np
import torch

from . import _lib

MAX_THRESHOLDS = 16
_ONE_BITS = 0x3F800000                     # float32 1.0
STATUS_SCORE, STATUS_LABEL, STATUS_THRESHOLD = 1, 2, 4


def key_shift_for(bins_per_octave):
    b = int(bins_per_octave)
    if b != bins_per_octave or b < 1 or b > 8192 or b & (b - 1):
        raise ValueError("bins_per_octave must be a power of two in [1, 8192], got %r" % (bins_per_octave,))
    return 23 - (b.bit_length() - 1)


def n_bins_for(key_shift):
    return (_ONE_BITS >> key_shift) + 1


def bin_edges(key_shift):
    """Lower edge of every bin (float32 values, as float64): the smallest float32 with that key."""
    return (np.arange(n_bins_for(key_shift), dtype=np.uint32) << np.uint32(key_shift)).view(np.float32).astype(
        np.float64)


def _check_thresholds(thresholds):
    th = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    if th.size < 1 or th.size > MAX_THRESHOLDS:
        raise ValueError("between 1 and %d thresholds, got %d" % (MAX_THRESHOLDS, th.size))
    if not np.all(np.isfinite(th)):
        raise ValueError("thresholds must be finite, got %s" % th.tolist())
    return tuple(float(np.float32(t)) for t in th)


def _check_seg_ptr(seg_ptr, n):
    sp = np.asarray(seg_ptr, dtype=np.int64).reshape(-1)
    if sp.size < 1 or sp[0] != 0 or sp[-1] != n or np.any(np.diff(sp) < 0):
        raise ValueError("seg_ptr must run non-decreasing from 0 to the number of segments (%d)" % n)
    return sp


def segment_metrics_numpy(scores, targets, thresholds=(0.5,), bins_per_octave=1024, src=None, seg_ptr=None):
    """The specification of gnn_segment_metrics_update on host arrays.

    scores, targets: [n] (any shape, flattened) as float32; src [n] or None (None: every segment counts, else
    src < 0 is padding and skipped); seg_ptr [G + 1] or None.  Returns a dict:
      counts [T + 1, 2] int64 - row 0 segments per class, row 1 + k segments with e > thresholds[k];
      hist [2, n_bins] int64 - per class, segments per key (float32 bits >> key_shift);
      per_graph [G, T + 1, 2] int64 or None - counts graph by graph;
      status - bits STATUS_SCORE / STATUS_LABEL / STATUS_THRESHOLD (0 = fine)."""
    ks = key_shift_for(bins_per_octave)
    nb = n_bins_for(ks)
    e = np.ascontiguousarray(np.asarray(scores, dtype=np.float32).reshape(-1))
    y = np.asarray(targets, dtype=np.float32).reshape(-1)
    if e.shape != y.shape:
        raise ValueError("scores and targets differ in size: %d vs %d" % (e.size, y.size))
    th = np.asarray(thresholds, dtype=np.float32).reshape(-1)
    if th.size > MAX_THRESHOLDS:
        raise ValueError("at most %d thresholds" % MAX_THRESHOLDS)
    keep = np.ones(e.size, dtype=bool) if src is None else np.asarray(src).reshape(-1) >= 0
    if keep.shape != e.shape:
        raise ValueError("src and scores differ in size")
    ok_e = (e >= 0) & (e <= 1)                                   # False for NaN
    is1, is0 = y == 1, y == 0
    status = (STATUS_SCORE if np.any(keep & ~ok_e) else 0) | (STATUS_LABEL if np.any(keep & ~(is0 | is1)) else 0) \
        | (STATUS_THRESHOLD if not np.all(np.isfinite(th)) else 0)
    valid = keep & ok_e & (is0 | is1)
    key = (e.view(np.uint32) & np.uint32(0x7FFFFFFF)) >> np.uint32(ks)
    cls = [valid & is0, valid & is1]
    above = [e > t for t in th]
    counts = np.zeros((th.size + 1, 2), dtype=np.int64)
    hist = np.zeros((2, nb), dtype=np.int64)
    for c in (0, 1):
        counts[0, c] = np.count_nonzero(cls[c])
        for k in range(th.size):
            counts[1 + k, c] = np.count_nonzero(cls[c] & above[k])
        hist[c] = np.bincount(key[cls[c]], minlength=nb)
    per_graph = None
    if seg_ptr is not None:
        sp = _check_seg_ptr(seg_ptr, e.size)
        G = sp.size - 1
        gid = np.repeat(np.arange(G), np.diff(sp))
        per_graph = np.zeros((G, th.size + 1, 2), dtype=np.int64)
        for c in (0, 1):
            per_graph[:, 0, c] = np.bincount(gid[cls[c]], minlength=G)
            for k in range(th.size):
                per_graph[:, 1 + k, c] = np.bincount(gid[cls[c] & above[k]], minlength=G)
    return {"counts": counts, "hist": hist, "per_graph": per_graph, "status": status}


def _ratio(a, b):
    """a / b in float64, 0.0 where b == 0 (sklearn's zero_division default)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.divide(a, b, out=np.zeros_like(a), where=b != 0)


class SegmentMetrics:
    """Counters for accuracy, precision, recall at fixed thresholds, the ROC curve and AUC, on one device.

    `counts` is ONE int64 tensor holding everything - [status word | counts (T + 1) x 2 | hist 2 x n_bins] - so
    `torch.distributed.all_reduce(m.counts)` (a sum, exact in int64) combines ranks.  The sum adds the status words
    too: after it the word only says nonzero = some rank saw bad input, not which kind (`merge` ORs it and keeps
    the kinds).  `update` is asynchronous; `compute`, `roc`, `auc` and `score_histogram` read
    the counters back once each."""

    def __init__(self, thresholds=(0.5,), bins_per_octave=1024, device=None):
        self.thresholds = _check_thresholds(thresholds)
        self.bins_per_octave = int(bins_per_octave)
        self.key_shift = key_shift_for(bins_per_octave)
        self.n_bins = n_bins_for(self.key_shift)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        T = len(self.thresholds)
        self._nc = 2 * (T + 1)
        self.counts = torch.zeros(1 + self._nc + 2 * self.n_bins, dtype=torch.int64, device=self.device)

    # views into `counts`
    def _views(self):
        c = self.counts
        return c[:1].view(torch.int32)[:1], c[1:1 + self._nc].view(-1, 2), c[1 + self._nc:].view(2, self.n_bins)

    def reset(self):
        self.counts.zero_()
        return self

    def merge(self, other):
        """Add another object's counters (same thresholds and resolution) into these."""
        if not isinstance(other, SegmentMetrics) or other.thresholds != self.thresholds or \
                other.key_shift != self.key_shift:
            raise ValueError("merge needs SegmentMetrics with the same thresholds and bins_per_octave")
        theirs = other.counts.to(self.device)
        word = self.counts[:1] | theirs[:1]                     # the status word: its bits ORed, not summed
        self.counts += theirs
        self.counts[:1] = word
        return self

    def update(self, scores, targets, batch=None, include_padding=False, per_graph=False):
        """Add one batch.  scores / targets: the model's output and labels, any matching shapes (flattened);
        CUDA tensors run the kernel, numpy arrays and CPU tensors `segment_metrics_numpy`.  With a HitGraphBatch,
        its src marks the padded segments (left out unless include_padding) and its seg_ptr the graphs:
        per_graph=True returns int64 [G, T + 1, 2] (row 0 the segments per class, row 1 + k those with
        e > thresholds[k]), on the device of the scores.  No read-back, no synchronisation."""
        if per_graph and batch is None:
            raise ValueError("per_graph=True needs the batch (its seg_ptr gives the graphs)")
        on_gpu = torch.is_tensor(scores) and scores.is_cuda
        n = int(scores.numel() if torch.is_tensor(scores) else np.asarray(scores).size)
        n_t = int(targets.numel() if torch.is_tensor(targets) else np.asarray(targets).size)
        if n != n_t:
            raise ValueError("scores and targets differ in size: %d vs %d" % (n, n_t))
        if batch is not None and batch.n_segments != n:
            raise ValueError("the batch has %d segments, the scores %d" % (batch.n_segments, n))
        status, counts, hist = self._views()
        if not on_gpu:
            e = scores.detach().cpu().numpy() if torch.is_tensor(scores) else scores
            y = targets.detach().cpu().numpy() if torch.is_tensor(targets) else targets
            src = None if batch is None or include_padding else _host(batch.src)
            spec = segment_metrics_numpy(e, y, self.thresholds, self.bins_per_octave, src,
                                         batch.seg_ptr if per_graph else None)
            counts += torch.from_numpy(spec["counts"]).to(self.device)
            hist += torch.from_numpy(spec["hist"]).to(self.device)
            if spec["status"]:
                status |= spec["status"]
            return None if not per_graph else torch.from_numpy(spec["per_graph"])
        if scores.device != self.device:
            raise ValueError("the counters live on %s, the scores on %s" % (self.device, scores.device))
        e = scores.detach().reshape(-1)
        e = e if e.dtype == torch.float32 and e.is_contiguous() else e.to(torch.float32).contiguous()
        y = torch.as_tensor(targets).detach().reshape(-1).to(device=self.device, dtype=torch.float32).contiguous()
        src = seg_ptr = pg = None
        if batch is not None:
            if not include_padding:
                src = batch.src
                if not torch.is_tensor(src) or src.device != self.device:
                    raise ValueError("the batch is not on %s" % self.device)
            if per_graph:
                seg_ptr = _device_seg_ptr(batch, self.device)
                pg = torch.empty((batch.n_graphs, len(self.thresholds) + 1, 2), dtype=torch.int64,
                                 device=self.device)
        _lib.segment_metrics_update(e, y, src, self.thresholds, self.key_shift, counts, hist, status, seg_ptr, pg)
        return pg

    def _read(self):
        host = self.counts.cpu().numpy()
        st = int(host[:1].view(np.int32)[0])
        if st:
            what = [w for bit, w in ((STATUS_SCORE, "a score that is NaN, inf or outside [0, 1]"),
                                     (STATUS_LABEL, "a label other than 0 or 1"),
                                     (STATUS_THRESHOLD, "a threshold that is not finite")) if st & bit]
            raise ValueError("SegmentMetrics saw bad input (status %d: %s; after an all_reduce of `counts` the word is "
                             "a sum over ranks and only its being nonzero counts); call reset()"
                             % (st, " or ".join(what) or "bad input"))
        counts = host[1:1 + self._nc].reshape(-1, 2)
        hist = host[1 + self._nc:].reshape(2, self.n_bins)
        return counts, hist

    def compute(self):
        """One read-back.  Returns a dict: n, n_pos, n_neg (ints); thresholds; tp, fp, tn, fn (int64 arrays, one
        entry per threshold, `e > t` predicts 1); accuracy, precision, recall (float64 arrays; 0.0 where the
        denominator is 0, sklearn's default).  Raises ValueError if bad input was seen (until reset())."""
        counts, _ = self._read()
        n_neg, n_pos = int(counts[0, 0]), int(counts[0, 1])
        tp, fp = counts[1:, 1].copy(), counts[1:, 0].copy()
        fn, tn = n_pos - tp, n_neg - fp
        return {"n": n_pos + n_neg, "n_pos": n_pos, "n_neg": n_neg, "thresholds": self.thresholds,
                "tp": tp, "fp": fp, "tn": tn, "fn": fn,
                "accuracy": _ratio(tp + tn, np.full_like(tp, n_pos + n_neg)),
                "precision": _ratio(tp, tp + fp), "recall": _ratio(tp, np.full_like(tp, n_pos))}

    def _curve(self, hist):
        neg, pos = hist
        nz = np.flatnonzero((neg + pos) > 0)[::-1]              # non-empty bins, highest first
        P, N = int(pos.sum()), int(neg.sum())
        tps = np.concatenate([[0], np.cumsum(pos[nz])]).astype(np.float64)
        fps = np.concatenate([[0], np.cumsum(neg[nz])]).astype(np.float64)
        thr = np.concatenate([[np.inf], bin_edges(self.key_shift)[nz]])
        tpr = tps / P if P else np.full(tps.shape, np.nan)
        fpr = fps / N if N else np.full(fps.shape, np.nan)
        return fpr, tpr, thr, pos, neg, P, N

    def roc(self):
        """(fpr, tpr, thresholds) in sklearn's orientation: thresholds decreasing, the first +inf, then the lower
        edge (a float32 value) of every non-empty bin; the point at threshold t counts `e >= t`, exactly.  NaN
        rates where a class is empty, as sklearn.  No drop_intermediate thinning."""
        fpr, tpr, thr, *_ = self._curve(self._read()[1])
        return fpr, tpr, thr

    def auc(self):
        """(auc, bound): the trapezoid under roc(), and a bound on its distance from the exact AUC (Mann-Whitney,
        ties counted one half: sklearn's roc_auc_score): 0.5 * sum_b pos_b * neg_b / (P * N), the pairs that share
        a bin and whose order the histogram does not see."""
        fpr, tpr, _, pos, neg, P, N = self._curve(self._read()[1])
        if not P or not N:
            return float("nan"), float("nan")
        bound = 0.5 * float(np.dot(pos.astype(np.float64), neg.astype(np.float64))) / (float(P) * float(N))
        return float(np.trapezoid(tpr, fpr)), bound

    def score_histogram(self, n_bins=50):
        """(counts int64 [2, n_bins] per class (0: fake, 1: true), edges [n_bins + 1]) over [0, 1], for plotting.
        APPROXIMATE: each fine bin is put whole into the linear bin that holds its lower edge, so a count can sit
        one linear bin low by up to one fine bin's width (1 / bins_per_octave of the score)."""
        _, hist = self._read()
        lin = np.minimum((bin_edges(self.key_shift) * n_bins).astype(np.int64), n_bins - 1)
        out = np.stack([np.bincount(lin, weights=hist[c], minlength=n_bins) for c in (0, 1)]).astype(np.int64)
        return out, np.linspace(0.0, 1.0, n_bins + 1)


def _host(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _device_seg_ptr(batch, device):
    """The batch's seg_ptr as an int64 tensor on `device` (the counters', which an `include_padding` update does not
    compare with the batch's: hence the device in the entry's name), uploaded once."""
    return batch.derived("device", ("seg_ptr", device),
                         lambda b: torch.from_numpy(_check_seg_ptr(b.seg_ptr, b.n_segments)).to(device))


_CTOR_KW = ("bins_per_octave", "device")
_UPDATE_KW = ("include_padding",)


def evaluate(model, generator, n_batches, thresholds=(0.5,), **kw):
    """`Estimator.predict` (gnn/estimator.py:137-146) with metrics in place of torch.cat: model.eval(), no_grad,
    n_batches of `(batch, targets)` from `generator` (batch_generator's output); the scores stay on the device.
    kw: bins_per_octave, device (default: the model's) go to SegmentMetrics, include_padding to update.
    Returns the SegmentMetrics."""
    bad = set(kw) - set(_CTOR_KW) - set(_UPDATE_KW)
    if bad:
        raise TypeError("evaluate() got unexpected keyword arguments %s" % sorted(bad))
    ctor = {k: kw[k] for k in _CTOR_KW if k in kw}
    if "device" not in ctor:
        p = next(model.parameters(), None)
        ctor["device"] = p.device if p is not None else None
    m = SegmentMetrics(thresholds, **ctor)
    model.eval()
    with torch.no_grad():
        for _ in range(int(n_batches)):
            batch, target = next(generator)
            if target is None:
                raise ValueError("the generator gave a batch without targets")
            if getattr(model, "scores_hits", False):
                # a NodeClassifier scores hits: every hit counts, as in the notebook's sklearn calls on the flattened
                # labels (gnn/MPNN_HitClassifier.ipynb cell 35)
                m.update(model(batch), target)
            else:
                m.update(model(batch), target, batch=batch, include_padding=kw.get("include_padding", False))
    return m
