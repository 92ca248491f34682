"""Fixed-point inference: SegmentClassifier as an FPGA would run it (include/gnn_hip_fixed.h, csrc/fixed_point.hip; for
batches of small graphs include/gnn_hip_fixed_events.h, csrc/fixed_events.hip: one launch, overflows per graph).

The reference's goal is a segment classifier small enough for an FPGA.  Pruning is `MaskedLinear`; this module is the
other lever, word length: a bit-accurate forward in two's-complement words of a chosen width with table-lookup
activations, on the GPU at detector scale, so that a scan over formats feeds `SegmentMetrics` directly.

    qm = quantize_model(model, FixedPointFormat(16, 6))
    out = qm(batch)                       # FixedPointScores: raw, scores, counts (overflows per pass and stage), fmt,
                                          # event_overflows (per graph, for batches of small graphs)
    rows = scan_precision(model, [(batch, y), ...], [FixedPointFormat(w, 6) for w in (8, 12, 16, 24)])

The arithmetic ("Fixed point") is all integers, so `fixed_forward_numpy` - the specification, vectorised
numpy int64 on the host - and the kernels agree bit for bit: no tolerance, no summation order.
"""
import numpy as np
import torch
from torch import nn

from . import _lib, call_route
from .hitgraph import HitGraphBatch

ROUNDINGS = ("trn", "rnd")
OVERFLOWS = ("wrap", "sat")
STAGES = ("input_z", "edge_z1", "edge_z2", "aggregate", "node_z3", "node_z4")      # the columns of `counts`


class FixedPointFormat:
    """A word format: `total_bits` W in 4..24, `int_bits` I in 2..W (sign included), Fb = W - I fraction bits; a stored
    integer k in [lo, hi] = [-2^(W-1), 2^(W-1) - 1] means k * 2^-Fb.  `rounding`: "trn" (floor) or "rnd" (add half a
    step, then floor); `overflow`: "wrap" (keep the low W bits) or "sat" (clip); `table_bits` in 4..12: the activation
    tables have 2^table_bits entries."""

    __slots__ = ("total_bits", "int_bits", "rounding", "overflow", "table_bits")

    def __init__(self, total_bits=16, int_bits=6, rounding="trn", overflow="wrap", table_bits=10):
        for name, v in (("total_bits", total_bits), ("int_bits", int_bits), ("table_bits", table_bits)):
            if isinstance(v, bool) or int(v) != v:
                raise ValueError("%s must be an integer, got %r" % (name, v))
        total_bits, int_bits, table_bits = int(total_bits), int(int_bits), int(table_bits)
        if not 4 <= total_bits <= 24:
            raise ValueError("total_bits must be in 4..24, got %d" % total_bits)
        if not 2 <= int_bits <= total_bits:
            raise ValueError("int_bits must be in 2..total_bits (%d), got %d" % (total_bits, int_bits))
        if rounding not in ROUNDINGS:
            raise ValueError("rounding must be one of %s, got %r" % (ROUNDINGS, rounding))
        if overflow not in OVERFLOWS:
            raise ValueError("overflow must be one of %s, got %r" % (OVERFLOWS, overflow))
        if not 4 <= table_bits <= 12:
            raise ValueError("table_bits must be in 4..12, got %d" % table_bits)
        for name, v in zip(self.__slots__, (total_bits, int_bits, rounding, overflow, table_bits)):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError("FixedPointFormat is immutable")

    frac_bits = property(lambda self: self.total_bits - self.int_bits)
    lo = property(lambda self: -(1 << (self.total_bits - 1)))
    hi = property(lambda self: (1 << (self.total_bits - 1)) - 1)
    max_list_entries = property(lambda self: 1 << (65 - 2 * self.total_bits), doc="every per-hit list must be SHORTER")

    def _key(self):
        return tuple(getattr(self, n) for n in self.__slots__)

    def __eq__(self, other):
        return isinstance(other, FixedPointFormat) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return "FixedPointFormat(total_bits=%d, int_bits=%d, rounding=%r, overflow=%r, table_bits=%d)" % self._key()


class FixedPointScores:
    """What a fixed-point forward returns: `raw` int32 [E] stored integers, `scores` float32 [E] = raw * 2^-Fb (exact),
    `counts` int64 [T + 1, 6] overflows per pass and stage (STAGES), `e_trace` [T + 1, E] / `H_trace` [T + 1, N, C]
    int32 or None, `fmt`; `event_overflows` int64 [n_graphs], the overflows of every graph over all passes and stages
    (they add up to `counts.sum()`), from the one-launch route for small graphs, else None."""

    __slots__ = ("raw", "scores", "counts", "e_trace", "H_trace", "fmt", "event_overflows")

    def __init__(self, raw, scores, counts, e_trace, H_trace, fmt, event_overflows=None):
        self.raw, self.scores, self.counts, self.e_trace, self.H_trace, self.fmt = raw, scores, counts, e_trace, H_trace, fmt
        self.event_overflows = event_overflows


# ---- the specification ------------------------------------------------------------------------------------------------
def quantize(v, fmt):
    """clip(rint(float64(v) * 2^Fb), lo, hi) as int64: half to even, always saturating; NaN -> 0."""
    k = np.rint(np.asarray(v, dtype=np.float64) * float(1 << fmt.frac_bits))
    return np.clip(np.where(np.isnan(k), 0.0, k), fmt.lo, fmt.hi).astype(np.int64)


def quantize_weights(weights, fmt):
    """The ten effective weight tensors (state_dict order, masks applied) as int64 arrays.  ValueError: a weight that
    is not finite."""
    out = []
    for i, w in enumerate(weights):
        w = np.asarray(w.detach().cpu().numpy() if torch.is_tensor(w) else w, dtype=np.float64)
        if not np.all(np.isfinite(w)):
            raise ValueError("weight tensor %d holds a value that is not finite: it has no fixed-point word" % i)
        out.append(quantize(w, fmt))
    return out


def activation_tables(fmt):
    """(T_tanh, T_sig): 2^table_bits int64 entries each, tanh sampled on [-4, 4) and the sigmoid on [-8, 8), in
    float64, then quantised."""
    n = 1 << fmt.table_bits
    i = np.arange(n, dtype=np.float64)
    return (quantize(np.tanh(-4.0 + 8.0 * i / n), fmt),
            quantize(1.0 / (1.0 + np.exp(-(-8.0 + 16.0 * i / n))), fmt))


def _requant(acc, fmt):
    """(stored integers, number of overflows) of exact accumulators at scale 2^-2Fb."""
    Fb, W = fmt.frac_bits, fmt.total_bits
    if fmt.rounding == "rnd" and Fb > 0:
        acc = acc + (1 << (Fb - 1))
    k = acc >> Fb
    over = (k < fmt.lo) | (k > fmt.hi)
    if fmt.overflow == "sat":
        k = np.clip(k, fmt.lo, fmt.hi)
    else:
        k = ((k + (1 << (W - 1))) & ((1 << W) - 1)) - (1 << (W - 1))
    return k, int(over.sum())


def _lookup(table, k, s, fmt):
    idx = ((k << s) >> fmt.frac_bits) + (1 << (fmt.table_bits - 1))
    return table[np.clip(idx, 0, (1 << fmt.table_bits) - 1)]


def _check_list_lengths(src, dst, n_hits, fmt):
    valid = src >= 0
    longest = 0
    if valid.any():
        longest = max(int(np.bincount(dst[valid], minlength=n_hits).max()),
                      int(np.bincount(src[valid], minlength=n_hits).max()))
    _refuse_long_lists(longest, fmt)


def _refuse_long_lists(longest, fmt):
    if longest >= fmt.max_list_entries:
        raise ValueError("a hit has a segment list of %d entries; at total_bits=%d the 64-bit sums are exact only for "
                         "lists shorter than %d" % (longest, fmt.total_bits, fmt.max_list_entries))


def fixed_forward_numpy(X, src, dst, weights, n_iters, fmt):
    """The specification of gnn_fx_forward on host arrays: X [N, F] float32, src / dst [E] (-1 / -1: a padded segment),
    `weights` the ten effective float tensors in state_dict order.  Returns FixedPointScores of numpy arrays, traces
    included."""
    X = np.asarray(X, dtype=np.float32)
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    N, E = X.shape[0], src.shape[0]
    _check_list_lengths(src, dst, N, fmt)
    Win, bin_, W1, b1, W2, b2, W3, b3, W4, b4 = quantize_weights(weights, fmt)
    D, F = Win.shape
    C = D + F
    Fb = fmt.frac_bits
    T_tanh, T_sig = activation_tables(fmt)
    st, ss = fmt.table_bits - 3, fmt.table_bits - 4
    counts = np.zeros((n_iters + 1, len(STAGES)), dtype=np.int64)
    valid = src >= 0
    s_v, d_v = src[valid], dst[valid]

    x = quantize(X, fmt)
    z, counts[0, 0] = _requant(x @ Win.T + (bin_ << Fb), fmt)
    H = np.concatenate([_lookup(T_tanh, z, st, fmt), x], axis=1)
    e_trace = np.zeros((n_iters + 1, E), dtype=np.int64)
    H_trace = np.zeros((n_iters + 1, N, C), dtype=np.int64)
    for t in range(n_iters + 1):
        H_trace[t] = H
        # edge pass: the per-hit halves of W1 [H_s | H_d]; a padded segment has zero rows
        P, Q = H @ W1[:, :C].T, H @ W1[:, C:].T
        acc = np.zeros((E, D), dtype=np.int64)
        acc[valid] = P[s_v] + Q[d_v]
        z1, counts[t, 1] = _requant(acc + (b1 << Fb), fmt)
        a = _lookup(T_tanh, z1, st, fmt)
        z2, counts[t, 2] = _requant(a @ W2.reshape(-1) + (int(b2.reshape(-1)[0]) << Fb), fmt)
        e = _lookup(T_sig, z2, ss, fmt)
        e_trace[t] = e
        if t == n_iters:
            break
        # node pass: exact sums over the in and the out list of every hit, then the two layers
        mi, mo = np.zeros((N, C), dtype=np.int64), np.zeros((N, C), dtype=np.int64)
        np.add.at(mi, d_v, e[valid, None] * H[s_v])
        np.add.at(mo, s_v, e[valid, None] * H[d_v])
        mi, n_i = _requant(mi, fmt)
        mo, n_o = _requant(mo, fmt)
        counts[t, 3] = n_i + n_o
        z3, counts[t, 4] = _requant(np.concatenate([mi, mo, H], axis=1) @ W3.T + (b3 << Fb), fmt)
        q = _lookup(T_tanh, z3, st, fmt)
        z4, counts[t, 5] = _requant(q @ W4.T + (b4 << Fb), fmt)
        H = np.concatenate([_lookup(T_tanh, z4, st, fmt), x], axis=1)
    raw = e_trace[n_iters].astype(np.int32)
    scores = raw.astype(np.float32) * np.float32(2.0 ** -Fb)
    return FixedPointScores(raw, scores, counts, e_trace.astype(np.int32), H_trace.astype(np.int32), fmt)


# ---- the product: HIP ----------------------------------------------------------------------------------------------
def _require_tanh_modules(model):
    acts = [model.input_network[1], model.edge_network.network[1], model.node_network.network[1],
            model.node_network.network[3]]
    for a in acts:
        if type(a) is not nn.Tanh:
            raise NotImplementedError("the fixed-point tables are nn.Tanh's: hidden_activation %s has none"
                                      % type(a).__name__)


class FixedPointSegmentClassifier:
    """`quantize_model`'s result: the model's ten effective weight tensors as int32 stored integers and the two
    activation tables, on the model's device; rebuilt when a parameter changes (the model's `_param_key`; after an
    in-place edit through `.data` call the model's `invalidate()` and this object's).  Calling it runs
    gnn_fxev_forward - one launch, one workgroup per graph - on a batch of small graphs and gnn_fx_forward, one kernel
    per reference module, on everything else (`call_route.choose_fixed`; the same bits either way).  `use_events =
    False` forces the per-module kernels; `last_route` is the kind of the last call."""

    use_events = True
    last_route = None

    def __init__(self, model, fmt):
        if not isinstance(fmt, FixedPointFormat):
            raise TypeError("fmt must be a FixedPointFormat, got %s" % type(fmt).__name__)
        _require_tanh_modules(model)
        self.model, self.fmt = model, fmt
        self._cache = None
        self._ensure()

    def invalidate(self):
        self._cache = None

    def _ensure(self):
        key = self.model._param_key()
        if self._cache is None or self._cache[0] != key:
            weights = self.model.effective_weights()
            dev = weights[0].device
            if dev.type != "cuda":
                raise _lib.GnnHipError("quantize_model needs a model on a ROCm device (no CPU path exists; the host "
                                       "specification is fixed_forward_numpy); got %s" % dev)
            F, D = self.model.input_dim, self.model.hidden_dim
            f = self.fmt
            if not _lib.fx_supported(F, D, f.total_bits, f.int_bits, f.table_bits):
                raise _lib.GnnHipError("no fixed-point kernel for input_dim=%d hidden_dim=%d" % (F, D))
            q = [torch.from_numpy(w.astype(np.int32)).to(dev) for w in quantize_weights(weights, f)]
            tabs = [torch.from_numpy(t.astype(np.int32)).to(dev) for t in activation_tables(f)]
            self._cache = (key, _lib.fx_params_struct(q, F, D), _lib.fx_tables_struct(tabs[0], tabs[1], f.table_bits),
                           _lib.fx_format_struct(*f._key()))
        return self._cache[1:]

    @property
    def weights(self):
        """The ten int32 tensors the kernels read (state_dict order)."""
        return self._ensure()[0]._keep

    @property
    def tables(self):
        return self._ensure()[1]._keep

    def _check_lists(self, batch):
        f = self.fmt
        if batch.n_segments < f.max_list_entries:
            return                              # no list can be that long
        longest = torch.maximum(batch.in_ptr.diff().max(), batch.out_ptr.diff().max())       # one read-back
        _refuse_long_lists(int(longest.item()), f)

    def __call__(self, batch, trace=False):
        if not isinstance(batch, HitGraphBatch):
            raise TypeError("the fixed-point forward takes a HitGraphBatch, got %s" % type(batch).__name__)
        if not batch.X.is_cuda:
            raise _lib.GnnHipError("the batch must be on a ROCm device (no CPU path exists; the host specification is "
                                   "fixed_forward_numpy)")
        if batch.X.shape[1] != self.model.input_dim:
            raise ValueError("the batch has %d features per hit, the model input_dim=%d"
                             % (batch.X.shape[1], self.model.input_dim))
        params, tables, fmt = self._ensure()
        self._check_lists(batch)
        f, n_graphs = self.fmt, batch.n_graphs
        # (the layout is asked for only where it can matter: a batch's first answer costs a pass over its endpoints)
        lay = (batch.event_layout() if self.use_events and not trace and 0 < n_graphs <= call_route.EVENTS_MAX_GRAPHS
               else None)
        fits = lay is not None and _lib.fxev_supported(self.model.input_dim, self.model.hidden_dim, f.table_bits,
                                                       lay.max_hits, lay.max_segments)
        self.last_route = call_route.choose_fixed(self.use_events, trace, n_graphs, lay, fits)
        if self.last_route == "events":
            raw, scores, counts, per_graph, _, _ = _lib.fxev_forward(batch, lay, params, fmt, tables, self.model.n_iters)
            return FixedPointScores(raw, scores, counts, None, None, f, per_graph)
        raw, scores, counts, et, Ht = _lib.fx_forward(batch, params, fmt, tables, self.model.n_iters, trace=trace)
        return FixedPointScores(raw, scores, counts, et, Ht, f)


def quantize_model(model, fmt):
    """A FixedPointSegmentClassifier of `model` (a SegmentClassifier on a ROCm device, hidden_activation nn.Tanh) in
    format `fmt`.  ValueError: a weight that is not finite."""
    return FixedPointSegmentClassifier(model, fmt)


def scan_precision(model, batches_with_labels, formats, thresholds=(0.5,), use_events=True):
    """One row (a dict) per format over `batches_with_labels`, a list of (HitGraphBatch, y) on the model's device:
    `format`; `n`, `tp`, `fp`, `tn`, `fn`, `accuracy`, `precision`, `recall` from SegmentMetrics.compute() (arrays, one
    entry per threshold; padded segments left out); `auc`; `overflows` int64 [6], the overflow counts of every stage
    summed over passes and batches (STAGES); `max_abs_diff`, the largest |score - float32 score| against the model's
    own forward; `events_overflowed`, the number of graphs with at least one overflow, summed over batches - what a
    trigger picks `int_bits` by - or None if a batch ran per module (FixedPointScores.event_overflows).  `use_events`
    = False forces the per-module kernels."""
    from .metrics import SegmentMetrics
    items = list(batches_with_labels)
    with torch.no_grad():
        was_training = model.training
        model.eval()
        try:
            floats = [model(b).reshape(-1) for b, _ in items]
        finally:
            model.train(was_training)
    rows = []
    for fmt in formats:
        qm = quantize_model(model, fmt)
        qm.use_events = use_events
        metrics = None
        over, worst = None, None
        spoiled, per_event = None, True         # graphs with an overflow; False once a batch ran per module
        for (b, y), ref in zip(items, floats):
            out = qm(b)
            if metrics is None:
                metrics = SegmentMetrics(thresholds=thresholds, device=out.scores.device)
            metrics.update(out.scores, y, batch=b)
            total = out.counts.sum(dim=0)
            over = total if over is None else over + total
            if out.event_overflows is None:
                per_event = False
            elif per_event:
                n = (out.event_overflows > 0).sum()
                spoiled = n if spoiled is None else spoiled + n
            if out.scores.numel():
                d = (out.scores - ref).abs().max()
                worst = d if worst is None else torch.maximum(worst, d)
        row = {"format": fmt}
        if metrics is not None:
            c = metrics.compute()
            row.update({k: c[k] for k in ("n", "tp", "fp", "tn", "fn", "accuracy", "precision", "recall")})
            row["auc"] = metrics.auc()[0]
        row["overflows"] = (over.cpu().numpy() if over is not None else np.zeros(len(STAGES), dtype=np.int64))
        row["max_abs_diff"] = float(worst.item()) if worst is not None else 0.0
        row["events_overflowed"] = (int(spoiled.item()) if spoiled is not None else 0) if per_event else None
        rows.append(row)
    return rows
