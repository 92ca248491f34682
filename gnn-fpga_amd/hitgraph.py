"""Index-form hit graphs: the HBM layout the HIP kernels consume.

The reference keeps the hit<->segment association as two dense one-hot matrices
`Ri`, `Ro` of shape [B, N, E] (reference gnn/graph.py:28-35,
gnn/trainSegmentClassifier.py:66-95) and uses `bmm` against them as gather and
scatter-add (reference gnn/model.py:71-72,114-119).  Here the same association is
stored once, in index form, for a *block-diagonal batch* of G graphs:

    X        float32 [N, F]     hit features, graphs concatenated (global hit ids)
    src,dst  int32   [E]        start / end hit of every segment; -1 = padded column
    in_ptr   int32   [N+1]      CSR over segments ENDING at each hit   (rows of Ri)
    in_eid   int32   [E_valid]  segment ids, grouped by end hit, ascending id (built on the GPU: [E], the
                                entries from in_ptr[N] on are -1)
    in_nbr   int32   [E_valid]  = src[in_eid]   (the hit at the other end)
    out_ptr / out_eid / out_nbr the same for segments STARTING at each hit (rows of Ro),
                                out_nbr = dst[out_eid]

On disk the reference already stores exactly this ordering: `Ri.nonzero()` is
row-major (reference gnn/graph.py:23-26), so `Ri_rows` is sorted by hit and
`Ri_cols` is `in_eid`; `from_sparse_arrays` therefore needs a bincount, not a sort.

Host-side numpy builds the plan once per batch; `to(device)` uploads it.
"""
import os

import numpy as np
import torch

_I32 = np.int32


def _csr_by(key, other, n_hits):
    """Group valid segments by `key` hit; stable => ascending segment id per hit."""
    valid = np.flatnonzero(key >= 0)
    k = key[valid]
    from .plan import stable_argsort
    order = stable_argsort(k)
    eid = valid[order].astype(_I32)
    ptr = np.zeros(n_hits + 1, dtype=np.int64)
    np.cumsum(np.bincount(k, minlength=n_hits), out=ptr[1:])
    if ptr[-1] >= 2 ** 31:
        raise ValueError("segment count exceeds int32 index range")
    return ptr.astype(_I32), eid, other[eid].astype(_I32)


def _csr_by_device(key, other, n_hits):
    """_csr_by with torch ops on the tensors' own device (stable sort: the same arrays)."""
    valid = torch.nonzero(key >= 0).reshape(-1)
    k = key[valid].to(torch.int64)
    order = torch.sort(k, stable=True).indices
    eid = valid[order]
    ptr = torch.zeros(n_hits + 1, dtype=torch.int64, device=key.device)
    torch.cumsum(torch.bincount(k, minlength=n_hits), 0, out=ptr[1:])
    if int(ptr[-1]) >= 2 ** 31:
        raise ValueError("segment count exceeds int32 index range")
    return ptr.to(torch.int32), eid.to(torch.int32), other[eid].to(torch.int32)


def graph_sizes(i, g, n_feat=None):
    """(hits, segments) of graph `i` of a list, after the checks that need no pass over its arrays: X [N, F] of the
    list's width (`n_feat`: graph 0's), src / dst [E] of an integer dtype (a float array would be cast silently), and
    y - where the graph has labels - [E].  A ValueError names the graph; `from_graphs` and `batcher.GraphStore`
    both go through here, so neither lets numpy broadcast, truncate or leave unwritten what does not fit."""
    X, a, b = np.asarray(g.X), np.asarray(g.src), np.asarray(g.dst)
    if X.ndim != 2 or (n_feat is not None and X.shape[1] != n_feat):
        raise ValueError("graph %d: expected X [N, %s], got %s" % (i, "F" if n_feat is None else n_feat, X.shape))
    if a.ndim != 1 or a.shape != b.shape:
        raise ValueError("graph %d: expected src [E], dst [E], got %s and %s" % (i, a.shape, b.shape))
    if not (np.issubdtype(a.dtype, np.integer) and np.issubdtype(b.dtype, np.integer)):
        raise ValueError("graph %d: src / dst must be integer arrays, got %s and %s" % (i, a.dtype, b.dtype))
    y = getattr(g, "y", None)
    if y is not None and np.shape(y) != a.shape:
        raise ValueError("graph %d: %d segments but y of shape %s" % (i, a.shape[0], np.shape(y)))
    return int(X.shape[0]), int(a.shape[0])


def check_ends(i, a, b, n_hits):
    """Endpoints of graph `i` (ids local to it, not empty): below n_hits, negative only in pairs.  True if it has
    such pairs - padded segments of its own - which the caller writes as (-1, -1)."""
    if int(a.max()) >= n_hits or int(b.max()) >= n_hits:
        raise ValueError("graph %d: segment endpoint out of range (%d hits)" % (i, n_hits))
    if int(a.min()) >= 0 and int(b.min()) >= 0:
        return False
    if np.any((a < 0) != (b < 0)):
        raise ValueError("graph %d: a padded segment must have src = dst = -1" % i)
    return True


class _EventLayout:
    """Per-graph offsets of a block-diagonal batch (HitGraphBatch.event_layout): max_hits, max_segments and - as
    device tensors, uploaded at first use (one copy for both; a single-graph forward never needs them) -
    hit_ptr / seg_ptr [G+1] int32."""

    def __init__(self, hp, sp, device=None, sizes=None, both=None):
        self._hp, self._sp = hp, sp
        if sizes is None:
            sizes = (int(np.diff(np.asarray(hp)).max(initial=0)), int(np.diff(np.asarray(sp)).max(initial=0)))
        self.max_hits, self.max_segments = sizes
        self._device, self._both = device, both      # both: [2, G+1] int32 made on the device (nothing to upload)

    def ptrs(self, device=None):
        device = self._device if device is None else device
        if self._both is None or self._both.device != torch.device(device):
            self._both = torch.from_numpy(np.stack([np.asarray(self._hp), np.asarray(self._sp)]).astype(_I32)).to(device)
        return self._both[0], self._both[1]

    hit_ptr = property(lambda self: self.ptrs()[0])
    seg_ptr = property(lambda self: self.ptrs()[1])


class DerivedStores:
    """What batches and plans share: `_derived`, one dict ("store") of derived values per kind of dependency."""
    __slots__ = ()

    def derived(self, kind, name, make=None):
        """Entry `name` of the store `kind`; if absent: made by `make(self)` and kept, or None without `make`."""
        store = self._derived[kind]
        v = store.get(name)
        if v is None and make is not None:
            v = store[name] = make(self)
        return v

    def remember(self, kind, name, value):
        self._derived[kind][name] = value


class HitGraphBatch(DerivedStores):
    """A block-diagonal batch of hit graphs in index form (see module docstring).

    Every field an instance can have is named in `__slots__` and set in `_set`, which every constructor goes through.
    What is DERIVED from the arrays - by this module or another - lives in three stores (`derived` / `remember`):

      "host"      from segments and offsets: "event" ((max_hits, max_segments) of the event layout, () = never the
                  one-launch kernels), "ends" (host copies of src / dst), call_route's counters
      "device"    also from the device: "csr", "csr_status", "layout" (the event layout with its device pointers),
                  uploaded seg_ptr / hit_ptr; on a twin the valid-segment count and the sorted targets
      "features"  also from X: both GnnGraph structs (they hold X's address) and the level-ordered twin

                         host                device                                   features
      to(device)         kept                the segment lists moved, the rest dropped dropped
      with_features(X)   copied by value     shared                                   empty
      level_ordered()    "event": () only    empty                                    empty (the twin is its own twin)
      forget()           dropped             dropped                                  dropped (and the plan)
    """

    __slots__ = ("X", "src", "dst", "y", "n_hits", "n_features", "n_segments", "n_graphs", "hit_ptr", "seg_ptr",
                 "dense_shape", "plan", "validate_csr",
                 "hit_index", "pt", "eta",                              # set by the graph builders / from_npz
                 "seg_order", "seg_rank", "_fused", "_fused_dim",       # a level-ordered twin's; None on any other batch
                 "_derived", "__weakref__")
    _TENSORS = ("X", "src", "dst", "y")        # (+ the six CSR arrays once they exist)

    def _set(self, X, src, dst, y, hit_ptr, seg_ptr, dense_shape=None, *, host=None, device=None, plan=None,
             hit_index=None, pt=None, eta=None, validate_csr=False, seg_order=None, seg_rank=None, fused=None,
             fused_dim=None):
        """THE place where a batch's fields come into being (tensors, host int64 offsets; host / device: stores)."""
        self.X, self.src, self.dst, self.y = X, src, dst, y
        self.n_hits, self.n_features, self.n_segments = int(X.shape[0]), int(X.shape[1]), int(src.shape[0])
        self.hit_ptr, self.seg_ptr, self.n_graphs = hit_ptr, seg_ptr, len(hit_ptr) - 1
        self.dense_shape, self.plan = dense_shape, plan     # dense_shape: (B, N_max, E_max) when built from a padded batch
        # Device-built lists: False = trust the endpoints (checked where the batch was made; the builder skips malformed
        # segments either way), True = read the builder's status word back - 4 bytes and one synchronisation per batch.
        self.validate_csr = validate_csr
        self.hit_index, self.pt, self.eta = hit_index, pt, eta
        self.seg_order, self.seg_rank, self._fused, self._fused_dim = seg_order, seg_rank, fused, fused_dim
        self._derived = {"host": {} if host is None else host, "device": {} if device is None else device,
                         "features": {}}
        return self

    # read-only views of four entries under the names they had as attributes (tests and diagnostics read them)
    _twin = property(lambda self: self.derived("features", "twin"))
    _csr = property(lambda self: self.derived("device", "csr"))
    _forwards = property(lambda self: self.derived("host", "forwards") or 0)
    _src_host = property(lambda self: (self.derived("host", "ends") or (None,))[0])

    def forget(self):
        """A batch nobody has seen: no derived entry (counters, and lists the caller brought, included), no plan."""
        self._derived = {"host": {}, "device": {}, "features": {}}
        self.plan = None
        return self

    def __init__(self, X, src, dst, y=None, hit_ptr=None, seg_ptr=None, dense_shape=None, csr=None, _checked=False):
        X = np.ascontiguousarray(X, dtype=np.float32)
        src = np.ascontiguousarray(src, dtype=_I32)
        dst = np.ascontiguousarray(dst, dtype=_I32)
        if X.ndim != 2 or src.ndim != 1 or src.shape != dst.shape:
            raise ValueError("expected X [N,F], src [E], dst [E]")
        n = X.shape[0]
        if y is not None and np.shape(y) != src.shape:
            raise ValueError("%d segments but y of shape %s" % (src.shape[0], np.shape(y)))
        if not _checked:                             # (from_graphs checks graph by graph, while a graph is in cache)
            if np.any((src ^ dst) < 0):              # signs differ: exactly one end negative
                raise ValueError("a padded segment must have src = dst = -1")
            if src.size and (src.max(initial=-1) >= n or dst.max(initial=-1) >= n):
                raise ValueError("segment endpoint out of range")
        t = torch.from_numpy
        # The two CSRs serve the per-module kernels, the small-event kernel and the backward; the
        # tiled pipeline works from its own plan.  They are therefore built on first use (two
        # stable sorts of E keys: 15 s for 25.6 M segments) unless the caller brought them.
        self._set(t(X), t(src), t(dst), None if y is None else t(np.ascontiguousarray(y, dtype=np.float32)),
                  np.asarray([0, n] if hit_ptr is None else hit_ptr, dtype=np.int64),
                  np.asarray([0, src.shape[0]] if seg_ptr is None else seg_ptr, dtype=np.int64), dense_shape,
                  device=None if csr is None else {"csr": tuple(t(np.ascontiguousarray(a, dtype=_I32)) for a in csr)})

    _CSR_NAMES = ("in_ptr", "in_eid", "in_nbr", "out_ptr", "out_eid", "out_nbr")

    def _build_csr(self):
        n = self.n_hits
        if self.X.is_cuda and os.environ.get("GNN_CSR_BUILDER", "hip") == "hip":
            # gnn_csr_build (csrc/csr_build.hip): counting sort + rank, a handful of launches, no read-back;
            # eid / nbr arrays keep all n_segments entries (the lists, then -1)
            from . import _lib
            parts = _lib.csr_build(self.src, self.dst, n)
            if self.validate_csr and int(parts[6].item()) & 1:
                raise ValueError("segment endpoint out of range, or a segment with exactly one negative end")
            self.remember("device", "csr_status", parts[6])
            return parts[:6]
        if self.X.is_cuda:           # torch ops (stable sorts on the GPU; GNN_CSR_BUILDER=torch): A / B runs
            return _csr_by_device(self.dst, self.src, n) + _csr_by_device(self.src, self.dst, n)
        src, dst = self.src.numpy(), self.dst.numpy()
        return tuple(torch.from_numpy(a) for a in _csr_by(dst, src, n) + _csr_by(src, dst, n))

    def _ensure_csr(self):
        return self.derived("device", "csr", HitGraphBatch._build_csr)

    in_ptr, in_eid, in_nbr, out_ptr, out_eid, out_nbr = (property(lambda self, i=i: self._ensure_csr()[i]) for i in range(6))

    def build_plan(self, hidden_dim, limits=None):
        """Tiles + windows + SELL-16 execution plan of the fused kernels, built once for the
        kernel shape (input_dim = n_features, hidden_dim): by HIP kernels when the batch lives on the
        GPU (plan_hip.py / csrc/plan_build.hip; GNN_PLAN_BUILDER=torch selects the torch-op builder
        plan_device.py, which also takes the batches outside the kernels' bounds), else on the host
        with numpy (plan.py, the specification); all three build the same plan, array for array."""
        if self.plan is None or self.plan.hidden_dim != hidden_dim:
            from . import _lib
            lim = _lib.plan_limits(self.n_features, hidden_dim)
            lim.update(limits or {})       # tests / experiments: e.g. iter_records=0 -> global mode
            builder = os.environ.get("GNN_PLAN_BUILDER", "hip" if self.X.is_cuda else "host")
            if os.environ.get("GNN_HOST_PLAN") or not self.X.is_cuda:
                builder = "host"
            plan = None
            if builder == "hip":          # HIP kernels (csrc/plan_build.hip): milliseconds
                from .plan_hip import HipSellPlan, PlanBuilderUnsupported
                try:
                    plan = HipSellPlan(self, lim)
                except PlanBuilderUnsupported:
                    builder = "torch"     # outside the kernels' static bounds, or empty
            if plan is None and builder == "torch":
                from .plan_device import DeviceSellPlan
                plan = DeviceSellPlan(self, lim)
            if plan is None:
                from .plan import SellPlan
                plan = SellPlan(self, lim)
            self.plan = plan
            self.plan.hidden_dim = hidden_dim
            self.plan.to(self.X.device)
        return self.plan

    def with_features(self, X):
        """The same graphs with other hit features (the same segments read out again: another calibration, another
        feature scaling): a new batch object that SHARES the index arrays, the segment lists and - through
        `SellPlan.with_features` - the structure of the execution plan; nothing is sorted or planned again."""
        X = torch.as_tensor(X).to(torch.float32)
        if tuple(X.shape) != tuple(self.X.shape):
            raise ValueError("expected X of shape %s" % (tuple(self.X.shape),))
        X = X.to(self.X.device).contiguous()
        d = self._derived        # (the C structs hold the old X pointer, the twin the old rows: "features" starts empty)
        return HitGraphBatch.__new__(HitGraphBatch)._set(
            X, self.src, self.dst, self.y, self.hit_ptr, self.seg_ptr, self.dense_shape, host=dict(d["host"]),
            device=d["device"], plan=None if self.plan is None else self.plan.with_features(X),
            hit_index=self.hit_index, pt=self.pt, eta=self.eta, validate_csr=self.validate_csr)

    def level_ordered(self, hidden_dim=8):
        """The same batch in PLAN SPACE: hits numbered by the execution plan's padded ids - (graph, detector
        level), tiles, degree; `plan.n_pad` hits, the padding dummies without segments and with X = 0 - and
        segments sorted by end hit (stable: a hit's incoming segments keep the caller's order, which is the order
        of its list in the plan).  In that order the neighbours of consecutive hits lie in narrow id ranges, which
        makes the training kernels' record gathers L2-local (c3 x 32 training step 1.68 -> 1.46 ms), the scores of
        a hit's incoming segments are contiguous, and - round 3 - the training forward can run the fused tile
        kernels on the ORIGINAL batch's plan (`_fused`: gnn_segclf_forward_train_plan writes e_t / H_t / Q_t
        straight in this batch's numbering).  Scores are handed back per segment in the caller's order
        (`seg_order` / `seg_rank`) and weight gradients do not depend on numbering, so the twin is a drop-in for the
        training forward / backward.  Built once per batch (one plan + GPU sorts for its CSRs) and cached; returns
        self when there is nothing to gain (CPU batch, no segments, no plan for this shape)."""
        twin = self.derived("features", "twin")
        if twin is not None:
            return twin
        self.remember("features", "twin", self)
        if not self.X.is_cuda or self.n_hits == 0 or self.n_segments == 0:
            return self
        try:
            plan = self.build_plan(hidden_dim)
        except Exception:                      # no fused kernels for this shape: keep the caller's order
            return self
        dev = self.X.device
        n_pad = int(plan.n_pad)
        perm = plan.perm.to(torch.int64)                          # padded id -> caller's hit id, -1 = dummy
        new_ids = torch.nonzero(perm >= 0).reshape(-1)
        rank = torch.empty(self.n_hits, dtype=torch.int64, device=dev)
        rank[perm[new_ids]] = new_ids                             # caller's hit id -> padded id
        src, dst = self.src.to(torch.int64), self.dst.to(torch.int64)
        ts = torch.where(src >= 0, rank[src.clamp_min(0)], src)
        td = torch.where(dst >= 0, rank[dst.clamp_min(0)], dst)
        # segments sorted by end hit, padded ones last, ties in the caller's order: seg_order[k] = caller's index
        # of the twin's segment k; the autograd function hands scores back (and takes their gradient) in the
        # caller's order
        key = torch.where(ts >= 0, td, torch.full_like(td, 2 ** 62))
        seg_order = torch.argsort(key, stable=True)
        seg_rank = torch.empty_like(seg_order)
        seg_rank[seg_order] = torch.arange(self.n_segments, dtype=torch.int64, device=dev)
        y = self.y
        if y is not None and y.numel() == self.n_segments:
            y = y.to(dev)[seg_order]
        # taken over: offsets and dense shape, not `hit_index` (the caller's numbering).  X: the plan's renumbered rows
        # (dummies: zeros); "event": () - never the one-launch kernels; fused: the plan whose padded ids ARE its hit ids
        t = HitGraphBatch.__new__(HitGraphBatch)._set(
            plan.X[:n_pad].contiguous(), ts[seg_order].to(torch.int32).contiguous(),
            td[seg_order].to(torch.int32).contiguous(), y, self.hit_ptr, self.seg_ptr, self.dense_shape,
            host={"event": ()}, validate_csr=self.validate_csr, seg_order=seg_order, seg_rank=seg_rank, fused=plan,
            fused_dim=hidden_dim)
        t.remember("features", "twin", t)
        self.remember("features", "twin", t)
        return t

    def _event_sizes(self):
        """The event layout's host part: (max_hits, max_segments) if block-diagonal as `event_layout` says, else ()."""
        hp, sp = self.hit_ptr, self.seg_ptr
        from . import _lib
        if self.n_graphs == 1:
            # one graph (a single event through the model): nothing to check beyond what the constructor checked,
            # and no numpy passes on the way to the first launch
            ok = (hp[0] == 0 and sp[0] == 0 and hp[1] == self.n_hits and sp[1] == self.n_segments and
                  self.n_hits < 2 ** 31 and self.n_segments <= _lib.EVENTS_MAX_SEGMENTS)     # (larger: never a layout)
            return (self.n_hits, self.n_segments) if ok else ()
        ok = (hp[0] == 0 and sp[0] == 0 and hp[-1] == self.n_hits and
              sp[-1] == self.n_segments and np.all(np.diff(hp) >= 0) and np.all(np.diff(sp) >= 0)
              and self.n_hits < 2 ** 31 and self.n_segments < 2 ** 31)
        # graphs too large for the one-workgroup-per-graph kernels never take them: skip the
        # endpoint check, which copies src / dst to the host (50 us and a synchronisation on the
        # first forward of every detector-size batch)
        if not ok or int(np.diff(sp).max(initial=0)) > _lib.EVENTS_MAX_SEGMENTS:
            return ()
        if self.n_segments and self.n_graphs > 1:
            # (the host copies `to` kept of a batch made on the host, else one copy back from the device)
            src, dst = self.derived("host", "ends") or (self.src.cpu().numpy(), self.dst.cpu().numpy())
            gseg = np.repeat(np.arange(self.n_graphs), np.diff(sp))
            lo, hi = hp[:-1][gseg], hp[1:][gseg]
            pad = src < 0
            if not np.all(pad | ((src >= lo) & (src < hi) & (dst >= lo) & (dst < hi))):
                return ()
        return (int(np.diff(hp).max(initial=0)), int(np.diff(sp).max(initial=0)))

    def event_layout(self):
        """Per-graph layout for the one-workgroup-per-graph kernel (`_lib.segclf_forward_events`):
        device copies of hit_ptr / seg_ptr and the largest graph's size, or None when the batch is
        not block-diagonal in the sense that kernel needs (every segment of graph i inside
        [seg_ptr[i], seg_ptr[i+1]) joins two hits of graph i; padded segments are fine).
        Checked once, on the host; the layout object itself (it uploads hit_ptr / seg_ptr when somebody asks for
        them) is the device's."""
        lay = self._derived["device"].get("layout")
        if lay is None:
            sizes = self.derived("host", "event", HitGraphBatch._event_sizes)
            if sizes:
                lay = _EventLayout(self.hit_ptr, self.seg_ptr, self.X.device, sizes)
                self.remember("device", "layout", lay)
        return lay

    # -- constructors ------------------------------------------------------------------
    @classmethod
    def from_graphs(cls, graphs, pad_segments=False, pin_memory=None, first=0, n_features=None):
        """Index-form batcher: block-diagonal concatenation.

        Replaces the zero-padding `merge_graphs` (reference
        gnn/trainSegmentClassifier.py:66-95): batch composition order is the list
        order (`graphs[j:j+batch_size]`, :103-104), features cast to float32 (:38-44).
        `pad_segments=False`: no padding at all (scores [E_total]).
        `pad_segments=True`: every graph's segment list is padded to the batch's E_max with
        `src = dst = -1` columns and `dense_shape = (B, N_max, E_max)` is set, so the model
        returns the reference's [B, E_max] layout (padded columns score sigmoid(W2 tanh(b1) + b2)
        and carry target 0, exactly like merge_graphs' zero columns); hits are never padded.
        A graph whose arrays do not fit together (`graph_sizes`, `check_ends`) is refused with a ValueError that
        names it: its place in the list plus `first`, the place of graphs[0] in the caller's dataset.
        `n_features`: the width every X must have (default: graphs[0]'s; a dataset's batches pass the dataset's).
        """
        B = len(graphs)
        hit_ptr = np.zeros(B + 1, dtype=np.int64)
        seg_ptr = np.zeros(B + 1, dtype=np.int64)
        shape0 = np.shape(graphs[0].X) if graphs else (0, 0)
        n_feat = int(shape0[1]) if len(shape0) == 2 else None           # (None: graph 0 is refused for its X)
        n_feat = n_feat if n_features is None else int(n_features)
        sizes = [graph_sizes(first + i, g, n_feat) for i, g in enumerate(graphs)]     # (before anything is allocated)
        e_max = max((e for _, e in sizes), default=0)
        for i, (n_g, e) in enumerate(sizes):
            hit_ptr[i + 1] = hit_ptr[i] + n_g
            seg_ptr[i + 1] = seg_ptr[i] + (e_max if pad_segments else e)
        # Large batches are put together in PINNED host memory when a GPU is there to receive them (pin_memory=None:
        # from 1 M segments on; torch's caching host allocator hands the same blocks out again batch after batch): the
        # upload of 256 detector graphs then runs at the link's rate, 21 -> 6 ms.
        E_all = int(seg_ptr[-1])
        pin = bool(pin_memory) if pin_memory is not None else (E_all >= (1 << 20) and torch.cuda.is_available())

        def host(shape, dtype, fill=None):
            if pin:
                a = torch.empty(shape, dtype={np.float32: torch.float32, _I32: torch.int32}[dtype], pin_memory=True).numpy()
                if fill is not None:
                    a.fill(fill)
                return a
            return np.empty(shape, dtype=dtype) if fill is None else np.full(shape, fill, dtype=dtype)

        X = host((int(hit_ptr[-1]), n_feat), np.float32)
        for i, g in enumerate(graphs):
            X[hit_ptr[i]:hit_ptr[i + 1]] = np.asarray(g.X, dtype=np.float32)
        ys = [getattr(g, "y", None) for g in graphs]
        have_y = not any(v is None for v in ys)

        if int(hit_ptr[-1]) >= 2 ** 31 or int(seg_ptr[-1]) >= 2 ** 31:
            raise ValueError("batch outside the int32 index range")

        # every graph's endpoints + its hit offset, written straight into its slice of ONE int32 array per end (the
        # first version went through int64 copies, np.where and a concatenate: 25 ms per million segments - more than
        # the GPU needs to plan AND score the batch), and checked graph by graph while the graph is in cache (the
        # constructor's checks are whole-batch passes)
        E_tot = int(seg_ptr[-1])
        src = host(E_tot, _I32, -1 if pad_segments else None)
        dst = host(E_tot, _I32, -1 if pad_segments else None)
        for i, g in enumerate(graphs):
            a, b = np.asarray(g.src), np.asarray(g.dst)
            (n_g, e), o, off = sizes[i], int(seg_ptr[i]), int(hit_ptr[i])
            if e == 0:
                continue
            own_padding = check_ends(first + i, a, b, n_g)
            np.add(a, off, out=src[o:o + e], casting="unsafe")
            np.add(b, off, out=dst[o:o + e], casting="unsafe")
            if own_padding:                              # padded segments of the graph itself stay -1
                pa = a < 0
                src[o:o + e][pa] = -1
                dst[o:o + e][pa] = -1
        y = None
        if have_y:
            y = host(E_tot, np.float32, 0.0 if pad_segments else None)
            for i, v in enumerate(ys):                   # (graph_sizes: exactly the graph's segment count)
                y[int(seg_ptr[i]):int(seg_ptr[i]) + sizes[i][1]] = np.asarray(v, dtype=np.float32)
        dense_shape = None
        if pad_segments:
            n_max = max((n_g for n_g, _ in sizes), default=0)
            dense_shape = (B, n_max, e_max)
        return cls(X, src, dst, y=y, hit_ptr=hit_ptr, seg_ptr=seg_ptr, dense_shape=dense_shape, _checked=True)

    def to_padded(self, flat, fill=0.0):
        """[E_total] values in this batch's segment order -> [B, E_max] (the reference's target /
        score layout, gnn/trainSegmentClassifier.py:86,110); `fill` in the padded entries."""
        if self.dense_shape is not None:
            return flat.reshape(self.dense_shape[0], self.dense_shape[2])
        counts = np.diff(self.seg_ptr)
        B, e_max = self.n_graphs, int(counts.max(initial=0))
        out = flat.new_full((B, e_max), fill) if torch.is_tensor(flat) else np.full((B, e_max), fill,
                                                                                 dtype=np.asarray(flat).dtype)
        for i in range(B):
            out[i, :counts[i]] = flat[self.seg_ptr[i]:self.seg_ptr[i + 1]]
        return out

    def from_padded(self, padded, counts=None):
        """[B, E_max] -> flat values of the real segments, graph by graph (`counts`: segments per
        graph; default: this batch's own when it is unpadded)."""
        if counts is None:
            if self.dense_shape is not None:
                raise ValueError("a padded batch does not know its graphs' true segment counts")
            counts = np.diff(self.seg_ptr)
        parts = [padded[i, :int(c)] for i, c in enumerate(counts)]
        return torch.cat(parts) if torch.is_tensor(padded) else np.concatenate(parts)

    @classmethod
    def from_sparse_arrays(cls, X, Ri_rows, Ri_cols, Ro_rows, Ro_cols, y=None):
        """From the reference's on-disk `SparseGraph` arrays (gnn/graph.py:20-26,179-194).

        `Ri_rows` (end hits) and `Ro_rows` (start hits) are sorted ascending because
        `nonzero()` is row-major, so they are CSR order already: rowptr is a bincount.
        Unsorted input (hand-made files) is handled by a stable sort.
        """
        X = np.asarray(X, dtype=np.float32)
        n = X.shape[0]
        e = int(np.asarray(Ri_rows).shape[0])
        if np.asarray(Ro_rows).shape[0] != e:
            raise ValueError("Ri and Ro must describe the same segments")

        def one(rows, cols):
            rows = np.asarray(rows, dtype=np.int64)
            cols = np.asarray(cols, dtype=np.int64)
            if rows.size and np.any(np.diff(rows) < 0):
                o = np.lexsort((cols, rows))
                rows, cols = rows[o], cols[o]
            ptr = np.zeros(n + 1, dtype=np.int64)
            np.cumsum(np.bincount(rows, minlength=n), out=ptr[1:])
            end = np.full(e, -1, dtype=np.int64)
            end[cols] = rows
            return ptr.astype(_I32), cols.astype(_I32), end

        in_ptr, in_eid, dst = one(Ri_rows, Ri_cols)
        out_ptr, out_eid, src = one(Ro_rows, Ro_cols)
        if np.any(src < 0) or np.any(dst < 0):
            raise ValueError("every segment needs exactly one start and one end hit")
        csr = (in_ptr, in_eid, src[in_eid].astype(_I32),
               out_ptr, out_eid, dst[out_eid].astype(_I32))
        return cls(X, src, dst, y=y, csr=csr)

    @classmethod
    def from_npz(cls, filename):
        """Read one graph file written by the reference's `save_graph` (gnn/graph.py:179-194) or its
        muon variant (gnn/Muon_graph.py:198-217, `SparseGraphProp`: + `pt`, `eta`)."""
        with np.load(filename) as f:  # allow_pickle stays False
            b = cls.from_sparse_arrays(f["X"], f["Ri_rows"], f["Ri_cols"],
                                       f["Ro_rows"], f["Ro_cols"],
                                       y=f["y"] if "y" in f.files else None)
            # the muon writer adds the generated muon's pt and eta (gnn/Muon_graph.py:198-205)
            b.pt = float(f["pt"]) if "pt" in f.files else None
            b.eta = float(f["eta"]) if "eta" in f.files else None
            return b

    @classmethod
    def from_dense(cls, X, Ri, Ro, y=None):
        """Compatibility adapter for the reference's dense inputs [B,N,F], [B,N,E], [B,N,E].

        Column j of Ri/Ro holds a single 1 at the end/start hit (gnn/graph.py:132-135);
        an all-zero column is a padded segment (gnn/trainSegmentClassifier.py:83-93)
        and becomes src = dst = -1.  O(B*N*E) reads: kept off the benchmarked path.
        """
        as_t = lambda a: a.detach() if torch.is_tensor(a) else torch.from_numpy(np.asarray(a))
        Xt, Rit, Rot = as_t(X), as_t(Ri), as_t(Ro)
        if Xt.dim() == 2:
            Xt, Rit, Rot = Xt[None], Rit[None], Rot[None]
        B, N, _ = Xt.shape
        E = Rit.shape[2]
        if tuple(Rit.shape) != (B, N, E) or tuple(Rot.shape) != (B, N, E):
            raise ValueError("expected X [B,N,F], Ri [B,N,E], Ro [B,N,E]")
        if Rit.is_cuda and Rot.is_cuda and Xt.is_cuda:
            return cls._from_dense_device(Xt, Rit, Rot, y)
        Xn = Xt.cpu().numpy()
        off = (np.arange(B, dtype=np.int64) * N)[:, None]

        def ends(R):   # the O(B*N*E) reduction runs where the matrix lives; [B,E] comes back
            nz = R != 0
            cnt = nz.sum(dim=1).cpu().numpy()
            if np.any(cnt > 1):
                raise ValueError("incidence matrix column with more than one hit")
            idx = nz.to(torch.uint8).argmax(dim=1).cpu().numpy().astype(np.int64) + off
            return np.where(cnt == 1, idx, -1).reshape(-1)

        dst, src = ends(Rit), ends(Rot)
        if np.any((src < 0) != (dst < 0)):
            raise ValueError("a segment column must be set in both Ri and Ro or in neither")
        yy = None if y is None else (y.detach().cpu().numpy() if torch.is_tensor(y) else
                                     np.asarray(y)).reshape(-1)
        return cls(Xn.reshape(B * N, -1), src, dst, y=yy,
                   hit_ptr=np.arange(B + 1) * N, seg_ptr=np.arange(B + 1) * E,
                   dense_shape=(B, N, E))

    validate_dense = True      # read the conversion kernel's error flag back (4 bytes, one sync per batch)

    @classmethod
    def _from_dense_device(cls, Xt, Rit, Rot, y=None):
        """from_dense for matrices that already live on the GPU (what an unchanged estimator.py loop
        hands over after `np_to_torch(...).cuda()`): one HIP kernel (`gnn_dense_to_index`), nothing
        crosses PCIe except - with `validate_dense` - the 4-byte error flag."""
        from . import _lib
        B, N, F = Xt.shape
        E = Rit.shape[2]
        f32 = lambda t: t.to(torch.float32).contiguous()          # noqa: E731
        src, dst, flags = _lib.dense_to_index(f32(Rit), f32(Rot))
        if cls.validate_dense:
            fl = int(flags.item())
            if fl & 1:
                raise ValueError("incidence matrix column with more than one hit")
            if fl & 2:
                raise ValueError("a segment column must be set in both Ri and Ro or in neither")
        if y is not None:
            y = (y.detach() if torch.is_tensor(y) else torch.from_numpy(np.asarray(y))
                 ).to(torch.float32).reshape(-1).to(Xt.device)
        # block-diagonal by construction: no host check of the endpoints
        return cls.__new__(cls)._set(f32(Xt).reshape(B * N, F), src, dst, y, np.arange(B + 1, dtype=np.int64) * N,
                                     np.arange(B + 1, dtype=np.int64) * E, (B, N, E),
                                     host={"event": (N, E) if B else (0, 0)})

    @classmethod
    def _from_device_arrays(cls, X, src, dst, y, hit_ptr, seg_ptr, dense_shape=None, layout_ptrs=None):
        """A batch from arrays that already live where they will be used (batcher.GraphStore): torch tensors X
        [N, F] float32, src / dst [E] int32 in batch numbering (-1 = padded), y [E] or None; hit_ptr / seg_ptr host
        arrays; layout_ptrs: the two as one int32 [2, G+1] tensor on X's device, where the maker has it.  The
        endpoints were checked when the store was built: block-diagonal by construction (a CPU batch checks)."""
        self = cls.__new__(cls)._set(X.to(torch.float32).contiguous(), src.to(torch.int32).contiguous(),
                                     dst.to(torch.int32).contiguous(), None if y is None else y.to(torch.float32).contiguous(),
                                     np.asarray(hit_ptr, dtype=np.int64), np.asarray(seg_ptr, dtype=np.int64), dense_shape)
        if X.is_cuda:
            lay = _EventLayout(self.hit_ptr, self.seg_ptr, X.device, both=layout_ptrs)
            self.remember("host", "event", (lay.max_hits, lay.max_segments))
            self.remember("device", "layout", lay)
        return self

    # -- device movement -----------------------------------------------------------------
    def to(self, device):
        d = self._derived
        if torch.device(device).type == "cuda" and not self.X.is_cuda and self.n_segments < (1 << 20):
            # for the event layout's check: views of the tensors about to go (large graphs never take those kernels)
            d["host"].setdefault("ends", (self.src.numpy(), self.dst.numpy()))
        for k in self._TENSORS:
            v = getattr(self, k)
            if v is not None:
                setattr(self, k, v.to(device))
        if self.plan is not None:
            self.plan.to(device)
        # "device": the lists go along, the rest is made again at next use; "features": pointers into the old device
        move = lambda v: v.to(device) if torch.is_tensor(v) else tuple(a.to(device) for a in v)      # noqa: E731
        d["device"] = {k: move(v) for k, v in d["device"].items() if k in ("csr", "csr_status")}
        d["features"] = {}
        return self

    def cuda(self, device=None):
        return self.to(torch.device("cuda", torch.cuda.current_device() if device is None else device))

    @property
    def device(self):
        return self.X.device

    def split_scores(self, e):
        """Per-graph views of a flat score vector [E]."""
        return [e[self.seg_ptr[i]:self.seg_ptr[i + 1]] for i in range(self.n_graphs)]
