"""Hands the package arrays that start off the 16-byte grid (test infrastructure, not product; imported by
test_offset_arrays_host.py and test_gpu_offset_arrays.py only).

torch's allocators hand out blocks that start on 64 (CPU) or 512 (GPU) bytes, so a tensor made by `torch.empty`,
`.cuda()` or `.clone()` never shows a kernel an address that is only a multiple of its element size.  The product's own
views do: a GraphStore window's X starts at a multiple of 12 bytes, a GradBucket's gradients and a flat-parameter
model's weights are packed back to back.

    shifted(t, k)           a contiguous copy of t at data_ptr() % 16 == (k * UNIT) % 16, UNIT = max(element size, 4),
                            carved from an allocation of its own between two guard bands
    Shift(mode).empty(...)  the same without values, for `out=` / `into=` / `workspace=` targets; Shift.guards_intact()
                            names the targets next to which a byte of the guard bands was written
    Shift(mode)             the k of every array of ONE call: mode 0 .. 3, or "mixed" = 1, 2, 3, 0, 1, ... over the
                            arrays in the order they are asked for (a guard that looks at one pointer only passes every
                            uniform k), or "mixed+1" .. "mixed+3", the same sequence begun one to three places later:
                            over the four, EVERY array of a call is once the one on the grid among neighbours off it,
                            whichever pointer a guard looks at.  8-byte element types have two residues: uniform modes
                            1 .. 3 give k = 1, the mixed ones alternate
    shift_batch(batch, s)   a device HitGraphBatch over shifted X, src, dst, y: no derived state, no plan
    shift_params(module, k) every parameter's `.data` re-pointed into ONE flat buffer, packed in parameters() order after
                            k leading floats: the GradBucket layout, for the weights (and with grads=True a GradBucket
                            whose flat buffer has the same lead)
    shifted_alloc(S)        context: the binding's OWN allocations (gnn_fpga_amd._lib's torch.empty / zeros / *_like: the
                            outputs the kernels store 16 bytes at a time, kept layers, gradient buffers, workspaces)
                            become guarded targets of S at its next offsets
    COVERS, NO_ARRAYS       which test of test_gpu_offset_arrays.py shifts which entry point of _lib.SIGNATURES

Element types narrower than 4 bytes (the uint8 workspaces) move in units of 4 bytes: the library rounds a workspace
pointer up itself, and an address below a float's alignment is not one a caller can hold an array at.
"""
import torch

GUARD = 4096                    # bytes either side of a body: more than any row stride of the library, a multiple of 16
GUARD_BYTE = 0xA5
MODES = (0, 1, 2, 3, "mixed", "mixed+1", "mixed+2", "mixed+3")
MIXED = (1, 2, 3, 0)
assert GUARD % 16 == 0


def unit(t_or_dtype):
    es = t_or_dtype.element_size() if torch.is_tensor(t_or_dtype) else torch.empty(0, dtype=t_or_dtype).element_size()
    return max(es, 4)


def residue(dtype, k):
    """data_ptr() % 16 that `shifted(t, k)` promises for t of `dtype`."""
    return (k * unit(dtype)) % 16


class Guarded:
    """A body between two guard bands of one uint8 block; `tensor` is the body under the asked shape and dtype."""

    def __init__(self, shape, dtype, k, device):
        es = torch.empty(0, dtype=dtype).element_size()
        n = 1
        for s in shape:
            n *= int(s)
        self.nbytes = n * es
        self.block = torch.empty(GUARD + 16 + self.nbytes + GUARD + 16, dtype=torch.uint8, device=device)
        self.block.fill_(GUARD_BYTE)
        base = self.block.data_ptr()
        self.off = GUARD + (residue(dtype, k) - (base + GUARD)) % 16
        body = self.block[self.off:self.off + self.nbytes]
        self.tensor = body.view(dtype).reshape(tuple(int(s) for s in shape))
        assert self.off >= GUARD and self.block.numel() - self.off - self.nbytes >= GUARD
        assert self.tensor.is_contiguous() and self.tensor.dtype == dtype
        assert n == 0 or self.tensor.data_ptr() % 16 == residue(dtype, k), (self.tensor.data_ptr() % 16, k, dtype)
        assert self.tensor.data_ptr() % es == 0

    def intact(self):
        """True while every byte either side of the body still holds the guard pattern.  Synchronises."""
        lo, hi = self.block[:self.off], self.block[self.off + self.nbytes:]
        return bool((lo == GUARD_BYTE).all().item()) and bool((hi == GUARD_BYTE).all().item())


def shifted(t, k):
    """A contiguous tensor with t's values, dtype and shape at data_ptr() % 16 == residue(t.dtype, k), carved from a
    larger allocation of its own (on t's device)."""
    g = Guarded(tuple(t.shape), t.dtype, k, t.device)
    out = g.tensor
    out.copy_(t.detach())
    assert out.shape == t.shape and out.dtype == t.dtype and out.device == t.device and out.is_contiguous()
    if t.numel():       # (an empty tensor from numpy has stride 0, which `view(torch.uint8)` refuses)
        assert torch.equal(out.reshape(-1).view(torch.uint8), t.detach().contiguous().reshape(-1).view(torch.uint8))
    return out


class Shift:
    """The shifts of one call.  `s(t)`: t shifted by this call's next k (None passes through); `empty(shape, dtype)`:
    a guarded target; `guards_intact()`: [] or the indices (in asking order) of the targets whose bands were written."""

    def __init__(self, mode, device="cuda"):
        assert mode in MODES, mode
        self.mode, self.device, self.count, self.targets, self.ks = mode, device, 0, [], []
        self.allocated = 0                  # targets made by shifted_alloc's proxy, not by the test

    def next_k(self, dtype):
        wide = unit(dtype) == 8
        if isinstance(self.mode, str):
            k = MIXED[(self.count + int(self.mode[6:] or 0)) % 4]
            self.count += 1
            k = k % 2 if wide else k
        else:
            k = min(self.mode, 1) if wide else self.mode
        self.ks.append(k)
        return k

    def s(self, t):
        if t is None:
            return None
        if isinstance(t, (list, tuple)):
            return type(t)(self.s(v) for v in t)
        return shifted(t, self.next_k(t.dtype))

    __call__ = s

    def empty(self, *shape, dtype=torch.float32):
        shape = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)) else shape
        g = Guarded(shape, dtype, self.next_k(dtype), self.device)
        self.targets.append(g)
        return g.tensor

    def guards_intact(self):
        if not self.targets:
            return []
        flags = [((g.block[:g.off] == GUARD_BYTE).all() & (g.block[g.off + g.nbytes:] == GUARD_BYTE).all()).reshape(1)
                 for g in self.targets]                     # one read-back for all of them
        return (~torch.cat(flags)).nonzero().flatten().tolist()


class _AllocProxy:
    """`torch` for a module of the package: `empty`, `zeros`, `empty_like` and `zeros_like` on the Shift's device type
    come from `S.empty` - shifted, between guard bands -, everything else is torch's."""

    def __init__(self, S):
        object.__setattr__(self, "_S", S)

    def __getattr__(self, name):
        return getattr(torch, name)

    def __setattr__(self, name, value):
        setattr(torch, name, value)

    def _make(self, real, size, kw, like=None, zero=False):
        S = self._S
        if set(kw) - {"dtype", "device"}:
            return real(*size, **kw) if like is None else real(like, **kw)
        if like is not None:
            device, dtype, shape = kw.get("device") or like.device, kw.get("dtype") or like.dtype, tuple(like.shape)
            if like.layout != torch.strided:
                return real(like, **kw)
        else:
            device = kw["device"] if kw.get("device") is not None else torch.empty(0).device
            dtype = kw.get("dtype") or torch.get_default_dtype()
            shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else size
        device = torch.device(device)
        if device.type != torch.device(S.device).type:
            return real(*size, **kw) if like is None else real(like, **kw)
        g = Guarded(tuple(int(s) for s in shape), dtype, S.next_k(dtype), device)
        S.targets.append(g)
        S.allocated += 1
        return g.tensor.zero_() if zero else g.tensor

    def empty(self, *size, **kw):
        return self._make(torch.empty, size, kw)

    def zeros(self, *size, **kw):
        return self._make(torch.zeros, size, kw, zero=True)

    def empty_like(self, t, **kw):
        return self._make(torch.empty_like, (), kw, like=t)

    def zeros_like(self, t, **kw):
        return self._make(torch.zeros_like, (), kw, like=t, zero=True)


class shifted_alloc:
    """Context manager: while active, the binding's OWN allocations - every output, kept training tensor, gradient
    buffer and workspace that gnn_fpga_amd._lib makes with torch.empty / zeros / empty_like / zeros_like - are targets
    of the Shift `S`: off the grid by the call's next k, between guard bands that `S.guards_intact()` checks.  That is
    how the arrays the kernels STORE 16 bytes at a time (H, Hnext, H_all, Q_all, grad_H, the builders' X) get off the
    grid: the Python wrappers take no `out=` for them.  (_lib alone: the plan's arrays, which plan_hip allocates, are
    not a caller's to place - include/gnn_hip.h, "Alignment".)"""

    MODULES = ("_lib",)

    def __init__(self, S):
        self.S, self._saved = S, None

    def __enter__(self):
        import importlib
        mods = [importlib.import_module("gnn_fpga_amd." + m) for m in self.MODULES]
        self._saved = [(m, m.__dict__["torch"]) for m in mods]
        proxy = _AllocProxy(self.S)
        for m, _ in self._saved:
            m.torch = proxy
        return self.S

    def __exit__(self, *exc):
        for m, real in self._saved:
            m.torch = real
        self._saved = None
        return False


def shift_batch(batch, s):
    """A device HitGraphBatch over shifted X, src, dst, y (`s`: a Shift, or a k for all four), with the batch's offsets
    and dense shape, no derived state and no plan."""
    from gnn_fpga_amd import HitGraphBatch
    if not isinstance(s, Shift):
        s = Shift(s)
    dev = torch.device(s.device)
    X, src, dst = (s(getattr(batch, k).to(dev)) for k in ("X", "src", "dst"))
    y = None if batch.y is None else s(batch.y.to(dev))
    out = HitGraphBatch.__new__(HitGraphBatch)._set(X, src, dst, y, batch.hit_ptr.copy(), batch.seg_ptr.copy(),
                                                    batch.dense_shape)
    assert out.plan is None and not any(out._derived.values()) and out.X.device.type == dev.type
    return out


def packed_offsets(module, k=0):
    """Element offset of every parameter in the flat buffer of shift_params(module, k)."""
    out, o = [], k
    for p in module.parameters():
        out.append(o)
        o += p.numel()
    return out


def shift_params(module, k, grads=False):
    """Re-points every parameter's `.data` into one flat float32 buffer: `k` leading floats, then the parameters back to
    back in parameters() order.  The buffer's own start is on the 16-byte grid, so parameter i sits at
    (k + sum of the sizes before it) * 4 bytes past it.  Returns the buffer (`grads=True`: (buffer, GradBucket), the
    bucket's gradients laid out the same way in a buffer of its own)."""
    params = list(module.parameters())
    assert params and all(p.dtype == torch.float32 for p in params) and 0 <= k < 4
    dev = params[0].device
    n = sum(p.numel() for p in params)
    flat = shifted(torch.zeros(k + n, dtype=torch.float32, device=dev), 0)
    for p, o in zip(params, packed_offsets(module, k)):
        view = flat[o:o + p.numel()].view_as(p)
        view.copy_(p.data)
        p.data = view
        assert p.data_ptr() == flat.data_ptr() + 4 * o and p.is_contiguous()
    if hasattr(module, "invalidate"):
        module.invalidate()
    if not grads:
        return flat
    from gnn_fpga_amd.shard import GradBucket
    bucket = GradBucket(params)
    gflat = shifted(torch.zeros(k + n + 2, dtype=torch.float32, device=dev), 0)
    bucket.flat = gflat[k:]
    for p, o in zip(params, packed_offsets(module, 0)):
        p.grad = bucket.flat[o:o + p.numel()].view_as(p)
        assert p.grad.data_ptr() == gflat.data_ptr() + 4 * (k + o)
    return flat, bucket


# ---- which test of test_gpu_offset_arrays.py shifts which entry point (test_offset_arrays_host.py holds this to
# _lib.SIGNATURES) ----------------------------------------------------------------------------------------------------
# entry point -> the test that hands it shifted arrays
COVERS = {
    "gnn_input_fwd": "test_per_module_forwards",
    "gnn_edge_fwd": "test_per_module_forwards",
    "gnn_node_fwd": "test_per_module_forwards",
    "gnn_segclf_forward": "test_per_module_forwards",
    "gnn_nodeclf_forward": "test_per_module_forwards",
    "gnn_csr_build": "test_per_module_forwards",
    "gnn_segclf_forward_events": "test_one_launch_forward",
    "gnn_segclf_forward_train_events": "test_training_forward_and_backward",
    "gnn_segclf_backward_events": "test_training_forward_and_backward",
    "gnn_segclf_forward_train": "test_training_forward_and_backward",
    "gnn_segclf_backward": "test_training_forward_and_backward",
    "gnn_nodeclf_forward_train": "test_training_forward_and_backward",
    "gnn_nodeclf_backward": "test_training_forward_and_backward",
    "gnn_edge_bwd": "test_training_forward_and_backward",
    "gnn_node_bwd": "test_training_forward_and_backward",
    "gnn_bce_loss": "test_bce_loss",
    "gnn_dense_to_index": "test_dense_to_index",
    "gnn_segclf_forward_plan": "test_plan_build_and_fused_forward",
    "gnn_segclf_forward_train_plan": "test_plan_build_and_fused_forward",
    "gnn_exp_product_bound": "test_plan_build_and_fused_forward",
    "gnn_plan_build_sizes": "test_plan_builder",
    "gnn_plan_build_sizes_graphs": "test_plan_builder",
    "gnn_plan_build_fill": "test_plan_builder",
    "gnn_graph_build_sizes": "test_graph_build",
    "gnn_graph_build_fill": "test_graph_build",
    "gnn_cut_study": "test_cut_study_and_layer_census",
    "gnn_layer_census": "test_cut_study_and_layer_census",
    "gnn_hit_samples_sizes": "test_hit_samples",
    "gnn_hit_samples_fill": "test_hit_samples",
    "gnn_muon_graph_sizes": "test_muon_graphs",
    "gnn_muon_graph_fill": "test_muon_graphs",
    "gnn_muon_graph_padded": "test_muon_graphs",
    "gnn_event_graphs_sizes": "test_event_graphs",
    "gnn_event_graphs_fill": "test_event_graphs",
    "gnn_select_hits_sizes": "test_select_hits",
    "gnn_select_hits_fill": "test_select_hits",
    "gnn_segment_metrics_update": "test_segment_metrics_update",
    "gnn_track_build_labels": "test_tracks",
    "gnn_track_build_lists": "test_tracks",
    "gnn_track_match": "test_tracks",
    "gnn_track_fit": "test_track_fit",
    "gnn_gcn_compress_count": "test_gcn",
    "gnn_gcn_compress_fill": "test_gcn",
    "gnn_gcn_forward": "test_gcn",
    "gnn_gcn_backward": "test_gcn",
    "gnn_toy_segment_graphs": "test_toy_segment_graphs",
    "gnn_toy_hit_graphs": "test_toy_hit_graphs",
}
# sizes, queries, versions and the profiler: no device array goes in or out (gnn_plan_limits, gnn_plan_route and
# gnn_profile_end fill HOST arrays; gnn_plan_route reads a gnn_plan_t's sizes only; the two *_workspace_bytes that
# take a pointer read the host's layer-pair table)
NO_ARRAYS = (
    "gnn_abi_version", "gnn_last_error", "gnn_shape_supported", "gnn_h_stride", "gnn_forward_workspace_bytes",
    "gnn_events_supported", "gnn_events_backward_supported", "gnn_backward_events_workspace_bytes",
    "gnn_backward_workspace_bytes", "gnn_plan_workspace_bytes", "gnn_plan_shape_supported", "gnn_plan_limits",
    "gnn_plan_route", "gnn_csr_build_workspace_bytes", "gnn_plan_build_workspace_bytes",
    "gnn_graph_build_workspace_bytes", "gnn_hit_samples_workspace_bytes", "gnn_muon_graph_workspace_bytes",
    "gnn_event_graphs_workspace_bytes", "gnn_select_hits_workspace_bytes", "gnn_metrics_bins",
    "gnn_metrics_workspace_bytes", "gnn_track_build_workspace_bytes", "gnn_track_match_workspace_bytes",
    "gnn_gcn_supported", "gnn_gcn_backward_workspace_bytes", "gnn_toy_graphs_list_width",
    "gnn_cut_study_workspace_bytes", "gnn_layer_census_workspace_bytes", "gnn_profile_begin", "gnn_profile_end",
)
