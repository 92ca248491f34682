"""ctypes binding of libgnn_hip.so (C ABI in include/*.h; _abi.py reads the signatures, struct layouts and constants
from those headers, this module holds the calls).

This is the only compute path of the package: there is no CPU or eager-PyTorch
fallback.  If the library is missing or a tensor is not on a ROCm device the call
raises.  torch is used for device memory and the stream handle only.
"""
import ctypes
import functools
import os

import numpy as np
import torch  # imported first: its bundled libamdhip64.so.7 is the one HIP runtime of the process

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgnn_hip.so")

from . import _abi
from ._abi import *  # noqa: F401,F403 - the signature tables, the struct classes, the headers' constants, GnnHipError

GNN_ABI_VERSION = 7           # the ABI the call sequences below are written for: the one constant not taken from the headers
GNN_FX_ROUNDING = {"trn": GNN_FX_TRN, "rnd": GNN_FX_RND}
GNN_FX_OVERFLOW = {"wrap": GNN_FX_WRAP, "sat": GNN_FX_SAT}

_f, _i32 = ctypes.c_void_p, ctypes.c_int32          # a device pointer, as the struct fields hold it; a host int32

_lib = None


def load():
    """Load libgnn_hip.so once; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if _abi.GNN_ABI_VERSION != GNN_ABI_VERSION:
        raise GnnHipError("the headers declare ABI %d but the binding's calls are written for ABI %d"
                          % (_abi.GNN_ABI_VERSION, GNN_ABI_VERSION))
    if not os.path.exists(LIB_PATH):
        raise GnnHipError(
            "HIP library %s is missing - build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C gnn-fpga_amd/csrc`; there is no CPU fallback" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for table in (SIGNATURES, ITER_SIGNATURES, FX_SIGNATURES, FXEV_SIGNATURES):
        for name, (res, args) in table.items():
            fn = getattr(lib, name)       # AttributeError if the symbol is not exported
            fn.restype, fn.argtypes = res, args
    if lib.gnn_abi_version() != GNN_ABI_VERSION:
        raise GnnHipError("libgnn_hip.so ABI %d != binding ABI %d"
                          % (lib.gnn_abi_version(), GNN_ABI_VERSION))
    with open("/proc/self/maps") as m:
        runtimes = {ln.split()[-1] for ln in m if "libamdhip64" in ln}
    if len(runtimes) > 1:
        raise GnnHipError("two HIP runtimes mapped (%s): kernels and torch streams would not "
                          "share a context" % ", ".join(sorted(runtimes)))
    _lib = lib
    return lib


def _check(rc):
    if rc != 0:
        raise GnnHipError("libgnn_hip: %s (code %d)" % (load().gnn_last_error().decode(), rc))


_cur_dev = None     # device of the call in progress (set by `_on`); _dev() checks tensors against it


def _dev(t, dtype, what):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise GnnHipError("%s must be a tensor on a ROCm device (no CPU path exists)" % what)
    if t.dtype != dtype or not t.is_contiguous():
        raise GnnHipError("%s must be contiguous %s" % (what, dtype))
    if _cur_dev is not None and t.device != _cur_dev:
        raise GnnHipError("%s is on %s but this call runs on %s: every tensor of one call must live "
                          "on one device" % (what, t.device, _cur_dev))
    return t.data_ptr()


def _rphiz(r, phi, z):
    """The pointers of the three float32 hit columns, as the builders' entry points take them."""
    return _dev(r, torch.float32, "r"), _dev(phi, torch.float32, "phi"), _dev(z, torch.float32, "z")


def _workspace(dev, need):
    """A workspace of the `need` bytes a *_workspace_bytes call asked for (0: it refused its arguments)."""
    if need == 0:
        raise GnnHipError("libgnn_hip: %s" % load().gnn_last_error().decode())
    return torch.empty(int(need), dtype=torch.uint8, device=dev)


def _read_back(struct_type, words):
    """Device int64 words that start with a sizes struct -> (the struct, all the words as a host array): the ONE
    device-to-host copy of a build."""
    host = words.cpu().numpy()
    sizes = struct_type()
    ctypes.memmove(ctypes.byref(sizes), host.ctypes.data, ctypes.sizeof(struct_type))
    return sizes, host


class _on:
    """`with _on(tensor_or_device) as stream:` - makes that device CURRENT for the library call (the
    kernels launch on the current device; a stream of another device would be an invalid handle and
    another device's pointers an illegal address), hands out ITS current stream, and lets _dev()
    refuse tensors that live elsewhere.  Structs built earlier carry `_device` and are checked too."""

    def __init__(self, where, *structs):
        dev = where.device if torch.is_tensor(where) else torch.device(where)
        if dev.type != "cuda":
            raise GnnHipError("tensors must be on a ROCm device (no CPU path exists); got %s" % dev)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        for st in structs:
            sd = getattr(st, "_device", None)
            if st is not None and sd is not None and sd != dev:
                raise GnnHipError("%s was built for %s but this call runs on %s"
                                  % (type(st).__name__, sd, dev))
        self.dev = dev
        self.ctx = torch.cuda.device(dev)

    def __enter__(self):
        global _cur_dev
        self.ctx.__enter__()
        self.prev, _cur_dev = _cur_dev, self.dev
        return torch.cuda.current_stream(self.dev).cuda_stream

    def __exit__(self, *exc):
        global _cur_dev
        _cur_dev = self.prev
        return self.ctx.__exit__(*exc)


@functools.lru_cache(maxsize=None)
def shape_supported(F, D):
    return bool(load().gnn_shape_supported(F, D))


def h_stride(F, D):
    s = load().gnn_h_stride(F, D)
    if s == 0:
        raise GnnHipError("no HIP kernel for input_dim=%d hidden_dim=%d" % (F, D))
    return s


def graph_struct(batch):
    i32 = torch.int32
    g = GnnGraph()
    g.X = _dev(batch.X, torch.float32, "X")
    for k in ("src", "dst", "in_ptr", "in_eid", "in_nbr", "out_ptr", "out_eid", "out_nbr"):
        setattr(g, k, _dev(getattr(batch, k), i32, k))
    g.n_hits, g.n_segments = batch.n_hits, batch.n_segments
    g._device = batch.X.device
    devs = {getattr(batch, k).device for k in ("src", "dst", "in_ptr", "in_eid", "in_nbr",
                                               "out_ptr", "out_eid", "out_nbr")}
    if devs != {g._device}:
        raise GnnHipError("the arrays of a batch must live on one device, got %s" % sorted(map(str, devs)))
    return g


def raw_graph_struct(batch):
    """gnn_graph_t of a batch WITHOUT its segment lists (all six pointers NULL): what gnn_segclf_forward_events takes
    for a never-seen batch - it builds the lists in LDS."""
    dev = batch.X.device
    g = GnnGraph()
    g.X = _dev(batch.X, torch.float32, "X")
    g.src, g.dst = _dev(batch.src, torch.int32, "src"), _dev(batch.dst, torch.int32, "dst")
    if batch.src.device != dev or batch.dst.device != dev:
        raise GnnHipError("the arrays of a batch must live on one device")
    g.n_hits, g.n_segments = batch.n_hits, batch.n_segments
    g._device = dev
    return g


def cached_graph_struct(batch):
    """graph_struct(batch), built once per batch, device and X: device pointers are stable while the batch lives."""
    return batch.derived("features", "gstruct", graph_struct)


def params_struct(weights, F, D, flags=0):
    """weights: the ten effective (masked) tensors in state_dict order."""
    p = GnnParams()
    C = F + D
    shapes = ((D, F), (D,), (D, 2 * C), (D,), (1, D), (1,), (D, 3 * C), (D,), (D, D), (D,))
    if len(weights) != 10:
        raise GnnHipError("expected the ten weight tensors in state_dict order, got %d" % len(weights))
    for name, w, shp in zip(("Win", "bin", "W1", "b1", "W2", "b2", "W3", "b3", "W4", "b4"), weights, shapes):
        n = 1
        for d in shp:
            n *= d
        if torch.is_tensor(w) and w.numel() != n:
            # the kernels index the tensors as [D, ...] rows of (F, D): a mismatch is an out-of-bounds read
            raise GnnHipError("%s has %d elements, but input_dim=%d hidden_dim=%d needs shape %s"
                              % (name, w.numel(), F, D, shp))
        setattr(p, name, _dev(w, torch.float32, name))
    p.F, p.D, p.flags = F, D, flags
    devs = {w.device for w in weights}
    if len(devs) != 1:
        raise GnnHipError("the weight tensors must live on one device, got %s" % sorted(map(str, devs)))
    p._device = devs.pop()
    return p


def exp_product_bound(weights, F, D, x_absmax):
    """max |P'|, |Q'| bound (python float; synchronises).  <= 60 permits GNN_FLAG_EXP_PRODUCT."""
    out = torch.empty(1, dtype=torch.float32, device=x_absmax.device)
    p = params_struct(weights, F, D)
    with _on(x_absmax, p) as st:
        _check(load().gnn_exp_product_bound(ctypes.byref(p), _dev(x_absmax, torch.float32, "x_absmax"),
                                            out.data_ptr(), st))
    return float(out.item())


def input_fwd(X, Win, bin_):
    """[n_hits, F] -> H [n_hits, ldh] = [tanh(Win X + bin) | X | 0]."""
    n, F = X.shape
    D = Win.shape[0]
    ldh = h_stride(F, D)
    H = torch.empty((n, ldh), dtype=torch.float32, device=X.device)
    with _on(X) as st:
        _check(load().gnn_input_fwd(_dev(X, torch.float32, "X"), _dev(Win, torch.float32, "Win"),
                                    _dev(bin_, torch.float32, "bin"), H.data_ptr(), n, F, D, ldh,
                                    st))
    return H


def edge_fwd(H, src, dst, W1, b1, W2, b2, F, D):
    """H [n_hits, ldh] (ldh >= C), src/dst int32 [n_segments] -> e [n_segments]."""
    n, ldh = H.shape
    E = src.shape[0]
    e = torch.empty(E, dtype=torch.float32, device=H.device)
    pq = torch.empty((max(n, 1), 2 * D), dtype=torch.float32, device=H.device)
    with _on(H) as st:
        _check(load().gnn_edge_fwd(_dev(H, torch.float32, "H"), ldh, _dev(src, torch.int32, "src"),
                                   _dev(dst, torch.int32, "dst"), _dev(W1, torch.float32, "W1"),
                                   _dev(b1, torch.float32, "b1"), _dev(W2, torch.float32, "W2"),
                                   _dev(b2, torch.float32, "b2"), e.data_ptr(), pq.data_ptr(),
                                   n, E, F, D, st))
    return e


def node_fwd(H, e, batch, W3, b3, W4, b4, F, D):
    """H [n_hits, ldh], e [n_segments] -> Hnext [n_hits, ldh] = [H' | X | 0]."""
    n, ldh = H.shape
    # (the kernel writes the h_stride(F, D) floats of every row, 0-pad included; a wider row's tail is the caller's)
    Hn = torch.empty_like(H) if ldh == h_stride(F, D) else torch.zeros_like(H)
    g = graph_struct(batch)
    with _on(H, g) as st:
        _check(load().gnn_node_fwd(_dev(H, torch.float32, "H"), ldh, _dev(e, torch.float32, "e"),
                                   ctypes.byref(g), _dev(W3, torch.float32, "W3"),
                                   _dev(b3, torch.float32, "b3"), _dev(W4, torch.float32, "W4"),
                                   _dev(b4, torch.float32, "b4"), Hn.data_ptr(), F, D, st))
    return Hn


def workspace_bytes(n_hits, n_segments, F, D):
    return int(load().gnn_forward_workspace_bytes(n_hits, n_segments, F, D))


def segclf_forward(batch, weights, F, D, n_iters, out=None, workspace=None, trace=False):
    """Whole SegmentClassifier forward on an index-form batch.

    Returns scores [n_segments] (and, with trace=True, e_trace [(T+1), E] and
    H_trace [(T+1), N, C])."""
    dev = batch.X.device
    E, N = batch.n_segments, batch.n_hits
    if not shape_supported(F, D):
        raise GnnHipError("no HIP kernel for input_dim=%d hidden_dim=%d" % (F, D))
    need = workspace_bytes(N, E, F, D)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.empty(E, dtype=torch.float32, device=dev)
    et = Ht = None
    if trace:
        et = torch.empty((n_iters + 1, E), dtype=torch.float32, device=dev)
        Ht = torch.empty((n_iters + 1, N, F + D), dtype=torch.float32, device=dev)
    g = graph_struct(batch)
    p = params_struct(weights, F, D)
    with _on(batch.X, g, p) as st:
        _check(load().gnn_segclf_forward(ctypes.byref(g), ctypes.byref(p), n_iters,
                                         _dev(out, torch.float32, "out"),
                                         et.data_ptr() if trace else None,
                                         Ht.data_ptr() if trace else None,
                                         workspace.data_ptr(), workspace.numel(), st))
    return (out, et, Ht) if trace else out


@functools.lru_cache(maxsize=None)
def events_supported(F, D, max_hits, max_segments):
    """True if graphs of at most that size fit the one-workgroup-per-graph kernel."""
    return bool(load().gnn_events_supported(F, D, max_hits, max_segments))


# Beyond this many segments per graph the one-workgroup-per-graph kernels lose to the tiled pipeline /
# per-pass kernels even when a graph fits their LDS (tools/cliff_probe.py: 256 x (300 hits, 2000 segments)
# 0.119 ms against 0.069; 256 x (150, 1000) 0.050 against 0.066)
EVENTS_MAX_SEGMENTS = 1200


def events_preferred(F, D, layout, backward=False):
    """Should a batch with this event layout take the one-launch kernels?  (They must be able to - LDS -
    and the graphs must be small enough to be worth a workgroup each.)"""
    if layout is None or layout.max_segments > EVENTS_MAX_SEGMENTS or D > 16:
        return False                 # (wide hidden layers: one toy graph 0.123 ms in one workgroup, 0.089 ms tiled)
    if not events_supported(F, D, layout.max_hits, layout.max_segments):
        return False
    return (not backward) or events_backward_supported(F, D, layout.max_hits, layout.max_segments)


def segclf_forward_events(batch, layout, weights, F, D, n_iters, out=None, params=None):
    """Whole forward in one launch, one workgroup per graph (small events); `layout` is
    `batch.event_layout()`.  Returns scores [n_segments], bit-identical to segclf_forward."""
    dev = batch.X.device
    if out is None:
        out = torch.empty(batch.n_segments, dtype=torch.float32, device=dev)
    # a batch nobody has asked the segment lists of (a never-seen event): the kernel builds them in LDS itself;
    # one graph: no offset arrays either - nothing is prepared or uploaded for a single fresh event
    g = (cached_graph_struct(batch) if batch.derived("device", "csr") is not None else
         batch.derived("features", "gstruct_raw", raw_graph_struct))
    p = params if params is not None else params_struct(weights, F, D)
    with _on(batch.X, g, p) as st:
        if batch.n_graphs == 1:
            hp = sp = None
        else:
            hp, sp = layout.ptrs(dev)
            hp, sp = _dev(hp, torch.int32, "hit_ptr"), _dev(sp, torch.int32, "seg_ptr")
        _check(load().gnn_segclf_forward_events(
            ctypes.byref(g), ctypes.byref(p), hp, sp, batch.n_graphs, layout.max_hits,
            layout.max_segments, n_iters, _dev(out, torch.float32, "out"), st))
    return out


def segclf_forward_train(batch, weights, F, D, n_iters, layout=None):
    """Training forward: returns (e_all [(T+1), E], H_all [(T+1), N, ldh], Q_all [T, N, D]); scores =
    e_all[-1].  Q_all (the node networks' hidden layers) is empty on the one-launch route, whose
    backward keeps everything in LDS.
    `layout` (batch.event_layout() of a batch of small graphs): one launch for the whole forward."""
    dev = batch.X.device
    E, N = batch.n_segments, batch.n_hits
    ldh = h_stride(F, D)
    e_all = torch.empty((n_iters + 1, E), dtype=torch.float32, device=dev)
    H_all = torch.empty((n_iters + 1, N, ldh), dtype=torch.float32, device=dev)
    if layout is not None:
        g = cached_graph_struct(batch)
        p = params_struct(weights, F, D)
        with _on(batch.X, g, p) as st:
            _check(load().gnn_segclf_forward_train_events(
                ctypes.byref(g), ctypes.byref(p), _dev(layout.hit_ptr, torch.int32, "hit_ptr"),
                _dev(layout.seg_ptr, torch.int32, "seg_ptr"), batch.n_graphs, layout.max_hits,
                layout.max_segments, n_iters, _dev(e_all, torch.float32, "e_all"),
                _dev(H_all, torch.float32, "H_all"), st))
        return e_all, H_all, torch.empty((0, N, D), dtype=torch.float32, device=dev)
    Q_all = torch.empty((n_iters, N, D), dtype=torch.float32, device=dev)
    ws = torch.empty(workspace_bytes(N, E, F, D), dtype=torch.uint8, device=dev)
    g = cached_graph_struct(batch)
    p = params_struct(weights, F, D)
    with _on(batch.X, g, p) as st:
        _check(load().gnn_segclf_forward_train(ctypes.byref(g), ctypes.byref(p), n_iters,
                                               e_all.data_ptr(), H_all.data_ptr(), Q_all.data_ptr(),
                                               ws.data_ptr(), ws.numel(), st))
    return e_all, H_all, Q_all


def segclf_forward_train_fused(batch, weights, F, D, n_iters, want_out=True):
    """The training forward of a PLAN-SPACE batch (HitGraphBatch.level_ordered) on the fused tile kernels of the
    plan it was made from.  Returns (e_all, H_all, Q_all, e_out) - the first three as segclf_forward_train gives
    them for this batch (row T of e_all by k_edge_tw, in this batch's segment order), e_out the final scores in the
    CALLER's segment order (None with want_out=False: a loss taken in this batch's order needs no second copy) - or
    None when this batch or shape has no fused training forward (call_route.fused_train_available)."""
    from .call_route import fused_train_available
    return segclf_forward_train_twin(batch, weights, F, D, n_iters, want_out) if fused_train_available(batch, F, D) else None


def segclf_forward_train_twin(twin, weights, F, D, n_iters, want_out=True):
    """segclf_forward_train_fused for a twin that is known to have the fused training forward."""
    n_valid = twin.derived("device", "n_valid", lambda t: int((t.src >= 0).sum().item()))      # once per batch
    return segclf_forward_train_plan(twin._fused, twin.in_ptr, n_valid, weights, F, D, n_iters, tw_src=twin.src,
                                     tw_dst=twin.dst, want_out=want_out)


def segclf_backward(batch, weights, F, D, n_iters, e_all, H_all, grad_out, into=None, Q_all=None):
    """Gradients of the ten (effective) weight tensors, in state_dict order (`into`: ten tensors the
    gradients are ADDED into instead of a fresh zero buffer; `Q_all`: the hidden layers kept by
    segclf_forward_train - without them the node passes are walked a second time)."""
    if Q_all is not None and Q_all.numel() != n_iters * batch.n_hits * D:
        Q_all = None
    dev = batch.X.device
    if into is not None:
        grads, gs = list(into), _grads_into(into)
    else:       # one zero-filled buffer, ten views (one memset launch instead of ten)
        grads, gs = _grad_views(weights, dev)
    need = int(load().gnn_backward_workspace_bytes(batch.n_hits, batch.n_segments, F, D))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    g = cached_graph_struct(batch)
    p = params_struct(weights, F, D)
    with _on(batch.X, g, p) as st:
        _check(load().gnn_segclf_backward(ctypes.byref(g), ctypes.byref(p), n_iters,
                                          _dev(e_all, torch.float32, "e_all"),
                                          _dev(H_all, torch.float32, "H_all"),
                                          _dev(Q_all, torch.float32, "Q_all") if Q_all is not None and Q_all.numel() else None,
                                          _dev(grad_out, torch.float32, "grad_out"),
                                          ctypes.byref(gs), ws.data_ptr(), ws.numel(), st))
    return grads


def _head_check(Wo, bo, F, D):
    if Wo.numel() != F + D or bo.numel() != 1:
        raise GnnHipError("the output network needs Wo [1, %d] and bo [1], got %s and %s"
                          % (F + D, tuple(Wo.shape), tuple(bo.shape)))


def nodeclf_forward(batch, weights, Wo, bo, F, D, n_iters, workspace=None, trace=False):
    """NodeClassifier forward (gnn_nodeclf_forward): hit scores y [n_hits] (and, with trace=True,
    H_trace [(T+1), N, C]).  `weights`: the trunk's ten effective tensors; Wo [1, C], bo [1]."""
    dev = batch.X.device
    N, E = batch.n_hits, batch.n_segments
    if not shape_supported(F, D):
        raise GnnHipError("no HIP kernel for input_dim=%d hidden_dim=%d" % (F, D))
    _head_check(Wo, bo, F, D)
    need = workspace_bytes(N, E, F, D)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    y = torch.empty(N, dtype=torch.float32, device=dev)
    Ht = torch.empty((n_iters + 1, N, F + D), dtype=torch.float32, device=dev) if trace else None
    g = graph_struct(batch)
    p = params_struct(weights, F, D)
    with _on(batch.X, g, p) as st:
        _check(load().gnn_nodeclf_forward(ctypes.byref(g), ctypes.byref(p), _dev(Wo, torch.float32, "Wo"),
                                          _dev(bo, torch.float32, "bo"), n_iters, y.data_ptr(),
                                          Ht.data_ptr() if trace else None, workspace.data_ptr(), workspace.numel(),
                                          st))
    return (y, Ht) if trace else y


def nodeclf_forward_train(batch, weights, Wo, bo, F, D, n_iters, keep_q=True):
    """NodeClassifier training forward: (e_all [T, E], H_all [(T+1), N, ldh], Q_all [T, N, D] or None, y [N])."""
    dev = batch.X.device
    E, N = batch.n_segments, batch.n_hits
    _head_check(Wo, bo, F, D)
    ldh = h_stride(F, D)
    e_all = torch.empty((n_iters, E), dtype=torch.float32, device=dev)
    H_all = torch.empty((n_iters + 1, N, ldh), dtype=torch.float32, device=dev)
    Q_all = torch.empty((n_iters, N, D), dtype=torch.float32, device=dev) if keep_q else None
    y = torch.empty(N, dtype=torch.float32, device=dev)
    ws = torch.empty(workspace_bytes(N, E, F, D), dtype=torch.uint8, device=dev)
    g = cached_graph_struct(batch)
    p = params_struct(weights, F, D)
    with _on(batch.X, g, p) as st:
        _check(load().gnn_nodeclf_forward_train(ctypes.byref(g), ctypes.byref(p), _dev(Wo, torch.float32, "Wo"),
                                                _dev(bo, torch.float32, "bo"), n_iters, e_all.data_ptr(),
                                                H_all.data_ptr(), Q_all.data_ptr() if keep_q else None,
                                                y.data_ptr(), ws.data_ptr(), ws.numel(), st))
    return e_all, H_all, Q_all, y


def nodeclf_backward(batch, weights, Wo, bo, F, D, n_iters, e_all, H_all, y, grad_y, Q_all=None):
    """Gradients of the trunk's ten tensors (state_dict order) and of Wo, bo: (grads, gWo, gbo).
    `Q_all` None: the backward walks the node passes a second time instead of reading the kept layers."""
    dev = batch.X.device
    _head_check(Wo, bo, F, D)
    grads, gs = _grad_views(list(weights) + [Wo, bo], dev)
    gWo, gbo = grads[10], grads[11]
    need = int(load().gnn_backward_workspace_bytes(batch.n_hits, batch.n_segments, F, D))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    g = cached_graph_struct(batch)
    p = params_struct(weights, F, D)
    with _on(batch.X, g, p) as st:
        _check(load().gnn_nodeclf_backward(ctypes.byref(g), ctypes.byref(p), _dev(Wo, torch.float32, "Wo"),
                                           _dev(bo, torch.float32, "bo"), n_iters, _dev(e_all, torch.float32, "e_all"),
                                           _dev(H_all, torch.float32, "H_all"),
                                           _dev(Q_all, torch.float32, "Q_all") if Q_all is not None else None,
                                           _dev(y, torch.float32, "y"), _dev(grad_y, torch.float32, "grad_y"),
                                           ctypes.byref(gs), gWo.data_ptr(), gbo.data_ptr(), ws.data_ptr(),
                                           ws.numel(), st))
    return grads[:10], gWo, gbo


def dense_to_index(Ri, Ro):
    """Dense [B, N, E] float32 incidence matrices on the device -> (src, dst int32 [B*E], flags int32 [1]);
    asynchronous - the caller decides whether to read the flags back."""
    B, N, E = Ri.shape
    src = torch.empty(B * E, dtype=torch.int32, device=Ri.device)
    dst = torch.empty(B * E, dtype=torch.int32, device=Ri.device)
    flags = torch.empty(1, dtype=torch.int32, device=Ri.device)
    with _on(Ri) as st:
        _check(load().gnn_dense_to_index(_dev(Ri, torch.float32, "Ri"), _dev(Ro, torch.float32, "Ro"), B, N, E,
                                         src.data_ptr(), dst.data_ptr(), flags.data_ptr(), st))
    return src, dst, flags


def csr_build(src, dst, n_hits):
    """The two segment lists of a batch on the device (gnn_csr_build): (in_ptr, in_eid, in_nbr, out_ptr, out_eid,
    out_nbr, status) - eid / nbr arrays of n_segments entries (the lists, then -1), status int32 [1] on the device
    (bit 0: malformed endpoints).  Asynchronous, no read-back - the caller decides whether to look at the status."""
    dev, i32 = src.device, torch.int32
    E = int(src.numel())
    ptrs = torch.empty((2, n_hits + 1), dtype=i32, device=dev)
    lists = torch.empty((4, max(E, 1)), dtype=i32, device=dev)
    status = torch.empty(1, dtype=i32, device=dev)
    need = int(load().gnn_csr_build_workspace_bytes(n_hits, E))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    with _on(src) as st:
        _check(load().gnn_csr_build(_dev(src, i32, "src"), _dev(dst, i32, "dst"), n_hits, E, ptrs[0].data_ptr(),
                                    lists[0].data_ptr(), lists[1].data_ptr(), ptrs[1].data_ptr(), lists[2].data_ptr(),
                                    lists[3].data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), st))
    return ptrs[0], lists[0][:E], lists[1][:E], ptrs[1], lists[2][:E], lists[3][:E], status


def _grad_views(weights, dev):
    """One zero-filled flat buffer, ten views shaped like the weights (state_dict order)."""
    flat = torch.zeros(sum(w.numel() for w in weights), dtype=torch.float32, device=dev)
    grads, o = [], 0
    for w in weights:
        grads.append(flat[o:o + w.numel()].view_as(w))
        o += w.numel()
    gs = GnnGrads()
    for name, t in zip(("Win", "bin", "W1", "b1", "W2", "b2", "W3", "b3", "W4", "b4"), grads):
        setattr(gs, name, t.data_ptr())
    return grads, gs


def edge_bwd(H, batch, weights, F, D, e, grad_e):
    """Backward of EdgeNetwork.forward: (grad_H [n_hits, ldh], [gW1, gb1, gW2, gb2]).
    `weights`: the ten effective tensors (only the edge network's four are read)."""
    dev = H.device
    grads, gs = _grad_views(weights, dev)
    gH = torch.zeros_like(H)
    ws = torch.empty(int(load().gnn_backward_workspace_bytes(batch.n_hits, batch.n_segments, F, D)),
                     dtype=torch.uint8, device=dev)
    g = cached_graph_struct(batch)
    p = params_struct(weights, F, D)
    with _on(H, g, p) as st:
        _check(load().gnn_edge_bwd(_dev(H, torch.float32, "H"), H.shape[1], ctypes.byref(g), ctypes.byref(p),
                                   _dev(e, torch.float32, "e"), _dev(grad_e, torch.float32, "grad_e"),
                                   _dev(gH, torch.float32, "grad_H"), ctypes.byref(gs), ws.data_ptr(), ws.numel(), st))
    return gH, grads[2:6]


def node_bwd(H, e, Hn, batch, weights, F, D, grad_Hn):
    """Backward of NodeNetwork.forward: (grad_H [n_hits, ldh], grad_e [n_segments], [gW3, gb3, gW4, gb4])."""
    dev = H.device
    grads, gs = _grad_views(weights, dev)
    gH = torch.empty_like(H)
    ge = torch.empty(batch.n_segments, dtype=torch.float32, device=dev)
    ws = torch.empty(int(load().gnn_backward_workspace_bytes(batch.n_hits, batch.n_segments, F, D)),
                     dtype=torch.uint8, device=dev)
    g = cached_graph_struct(batch)
    p = params_struct(weights, F, D)
    with _on(H, g, p) as st:
        _check(load().gnn_node_bwd(_dev(H, torch.float32, "H"), H.shape[1], _dev(e, torch.float32, "e"),
                                   _dev(Hn, torch.float32, "Hnext"), ctypes.byref(g), ctypes.byref(p),
                                   _dev(grad_Hn, torch.float32, "grad_Hnext"), _dev(gH, torch.float32, "grad_H"),
                                   _dev(ge, torch.float32, "grad_e"), ctypes.byref(gs), ws.data_ptr(), ws.numel(), st))
    return gH, ge, grads[6:10]


@functools.lru_cache(maxsize=None)
def events_backward_supported(F, D, max_hits, max_segments):
    """True if graphs of at most that size fit the one-launch backward (one workgroup per graph)."""
    return bool(load().gnn_events_backward_supported(F, D, max_hits, max_segments))


def _grads_into(into):
    """GnnGrads over ten caller-owned tensors (the backward ADDS into them)."""
    gs = GnnGrads()
    for name, t in zip(("Win", "bin", "W1", "b1", "W2", "b2", "W3", "b3", "W4", "b4"), into):
        setattr(gs, name, _dev(t, torch.float32, "grad " + name))
    return gs


def segclf_backward_events(batch, layout, weights, F, D, n_iters, e_all, H_all, grad_out, into=None):
    """segclf_backward for a batch of small graphs in ONE launch (`layout` = batch.event_layout()).
    `into`: ten tensors the gradients are ADDED into (e.g. the views of a GradBucket) instead of a
    fresh zero buffer."""
    dev = batch.X.device
    if into is not None:
        grads, gs = list(into), _grads_into(into)
    else:
        grads, gs = _grad_views(weights, dev)
    ws = torch.empty(int(load().gnn_backward_events_workspace_bytes(batch.n_graphs, F, D)), dtype=torch.uint8,
                     device=dev)
    g = cached_graph_struct(batch)
    p = params_struct(weights, F, D)
    with _on(batch.X, g, p) as st:
        _check(load().gnn_segclf_backward_events(
            ctypes.byref(g), ctypes.byref(p), _dev(layout.hit_ptr, torch.int32, "hit_ptr"),
            _dev(layout.seg_ptr, torch.int32, "seg_ptr"), batch.n_graphs, layout.max_hits, layout.max_segments,
            n_iters, _dev(e_all, torch.float32, "e_all"), _dev(H_all, torch.float32, "H_all"),
            _dev(grad_out, torch.float32, "grad_out"), ctypes.byref(gs), ws.data_ptr(), ws.numel(), st))
    return grads


def bce_loss(e, y, scale, want_grad=True):
    """(loss [1], dLoss/de [n] or None): nn.BCELoss value and gradient in one pass (HIP)."""
    n = e.numel()
    dev = e.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    grad = torch.empty(n, dtype=torch.float32, device=dev) if want_grad else None
    ws = torch.empty(1024, dtype=torch.float32, device=dev)         # GNN_BCE_WORKSPACE_BYTES
    with _on(e) as st:
        _check(load().gnn_bce_loss(_dev(e, torch.float32, "scores"), _dev(y, torch.float32, "targets"), n,
                                   float(scale), loss.data_ptr(), grad.data_ptr() if want_grad else None,
                                   ws.data_ptr(), st))
    return loss, grad


@functools.lru_cache(maxsize=None)
def plan_shape_supported(F, D):
    return bool(load().gnn_plan_shape_supported(F, D))


def plan_limits(F, D):
    """Tile / chunk sizes and LDS window budgets the plan builder must respect (no GPU needed)."""
    out = (_i32 * 4)()
    _check(load().gnn_plan_limits(F, D, out))
    return {"tile_hits": out[0], "iter_records": out[1], "chunk_segments": out[2],
            "edge_records": out[3]}


# gnn_plan_route: the names of the GNN_ROUTE_* fields, in order, and of the codes of the first, second, third and
# fifth (include/gnn_hip.h)
ROUTE_FIELDS = ("records", "input", "family", "fuse_first", "edge", "pack", "iter_lds", "iter2_lds", "cap_a", "cap_b",
                "edge_lds", "wide_window")
ROUTE_NAMES = {"records": ("fp32", "bf16", "exact"),
               "input": (None, "k_input4", "k_input4_bf", "k_input4_x"),
               "family": ("k_iter", "k_iter2", "k_iter_w", "k_iter_wx"),
               "edge": ("k_edge", "k_edge_w")}
_ROUTE_ENUMS = {"records": "GNN_REC_", "input": "GNN_INPUT_", "family": "GNN_FAMILY_", "edge": "GNN_EDGE_"}
if len(ROUTE_FIELDS) != GNN_ROUTE_FIELDS or any(len(ROUTE_NAMES[k]) != sum(n.startswith(prefix) for n in _abi.__all__)
                                                for k, prefix in _ROUTE_ENUMS.items()):
    raise GnnHipError("ROUTE_FIELDS / ROUTE_NAMES do not name what the GNN_ROUTE_* enums of include/gnn_hip.h hold")


def plan_route(plan, F, D, n_iters, flags=0, training=False):
    """The kernels the fused forward (`training`: the fused training forward) takes for this plan - a GnnPlan, or a
    plan object on the GPU -, shape, flags and the route switches of the environment, as the library decides them
    (gnn_plan_route; no GPU needed for a GnnPlan).  A dict over ROUTE_FIELDS: kernel choices by name, `fuse_first`
    and `pack` as bools, sizes as ints.  None: the shape has no fused training forward."""
    g = plan if isinstance(plan, GnnPlan) else plan_struct(plan)
    p = GnnParams()
    p.F, p.D, p.flags = F, D, flags
    out = (_i32 * len(ROUTE_FIELDS))()
    rc = load().gnn_plan_route(ctypes.byref(g), ctypes.byref(p), n_iters, int(training), out)
    if rc == GNN_ERR_UNSUPPORTED and training and plan_shape_supported(F, D):
        return None
    _check(rc)
    route = dict(zip(ROUTE_FIELDS, out))
    for k, names in ROUTE_NAMES.items():
        route[k] = names[route[k]]
    route["fuse_first"], route["pack"] = bool(route["fuse_first"]), bool(route["pack"])
    return route


def plan_struct(plan):
    g = GnnPlan()
    g.X = _dev(plan.X, torch.float32, "plan.X")
    for k in ("src", "dst", "in_off", "in_nbr", "out_off", "out_nbr", "tiles", "chunks",
              "in_off16", "in_nbr16", "out_off16", "out_nbr16", "sched_a", "sched_b", "sd16"):
        setattr(g, k, _dev(getattr(plan, k), torch.int32, "plan." + k))
    g.n_pad, g.n_segments = plan.n_pad, plan.n_segments
    g.n_tiles, g.n_chunks = plan.n_tiles, plan.n_chunks
    g.iter_lds_records, g.edge_lds_rows = plan.iter_lds_records, plan.edge_lds_rows
    g.n_lds_tiles, g.tile_hits_max = plan.n_lds_tiles, plan.tile_hits_max
    g.iter_lds_in, g.iter_lds_out = plan.iter_lds_in, plan.iter_lds_out
    g.max_list_steps = plan.max_list_steps
    g._device = plan.X.device
    return g


def plan_workspace_bytes(n_hits, n_segments, F, D):
    return int(load().gnn_plan_workspace_bytes(n_hits, n_segments, F, D))


def cached_plan_struct(plan):
    return plan.derived("features", "struct", plan_struct)


def segclf_forward_plan(plan, weights, F, D, n_iters, out=None, workspace=None, flags=0,
                        params=None):
    """Whole SegmentClassifier forward on a planned batch (fused pipeline) -> scores [E].
    `params`: a GnnParams built earlier from the same `weights` (skips re-validation)."""
    dev = plan.X.device
    need = plan.derived("structure", ("ws_need", F, D))
    if need is None:
        if not plan_shape_supported(F, D):
            raise GnnHipError("no fused HIP kernel for input_dim=%d hidden_dim=%d" % (F, D))
        need = plan_workspace_bytes(plan.n_pad, plan.n_segments, F, D)
        plan.remember("structure", ("ws_need", F, D), need)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.empty(plan.n_segments, dtype=torch.float32, device=dev)
    g = cached_plan_struct(plan)
    p = params if params is not None else params_struct(weights, F, D, flags)
    p.flags = flags
    with _on(plan.X, g, p) as st:
        _check(load().gnn_segclf_forward_plan(ctypes.byref(g), ctypes.byref(p), n_iters,
                                              _dev(out, torch.float32, "out"),
                                              workspace.data_ptr(), workspace.numel(), st))
    return out


def segclf_forward_train_plan(plan, seg_ptr, n_segments_valid, weights, F, D, n_iters, flags=0, workspace=None,
                              tw_src=None, tw_dst=None, want_out=True):
    """The training forward on a planned batch (fused tile kernels; gnn_segclf_forward_train_plan).
    `seg_ptr` int32 [n_pad + 1]: CSR pointer over end hits of the plan-space batch the backward runs on;
    `tw_src` / `tw_dst` int32 [E]: that batch's segment endpoints (plan hit ids, -1 = padded).
    Returns (e_all [(T + 1), E] in that batch's segment order - row T filled when tw_src / tw_dst are given, else
    the caller's to fill from e_out -, H_all [(T + 1), n_pad, ldh], Q_all [T, n_pad, D], e_out [E] in the plan's
    segment order or None with want_out=False).  A shape without a fused training forward is an error like any other:
    whether there is one is decided before the call (call_route.fused_train_available)."""
    dev = plan.X.device
    E, Np = plan.n_segments, plan.n_pad
    ldh = h_stride(F, D)
    need = plan_workspace_bytes(Np, E, F, D)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    if tw_src is None and not want_out:
        raise GnnHipError("segclf_forward_train_plan: the final scores are wanted in at least one order")
    # (padded segments are in no hit's list: their entries of rows 0 .. T-1 are never written nor read by the
    # backward's walks; zeros keep them defined)
    e_all = (torch.zeros if n_segments_valid < E else torch.empty)((n_iters + 1, E), dtype=torch.float32, device=dev)
    H_all = torch.empty((n_iters + 1, Np, ldh), dtype=torch.float32, device=dev)
    Q_all = torch.empty((n_iters, Np, D), dtype=torch.float32, device=dev)
    e_out = torch.empty(E, dtype=torch.float32, device=dev) if want_out else None
    g = cached_plan_struct(plan)
    p = params_struct(weights, F, D, flags)
    with _on(plan.X, g, p) as st:
        _check(load().gnn_segclf_forward_train_plan(ctypes.byref(g), ctypes.byref(p), n_iters,
                                                    _dev(seg_ptr, torch.int32, "seg_ptr"),
                                                    None if tw_src is None else _dev(tw_src, torch.int32, "tw_src"),
                                                    None if tw_dst is None else _dev(tw_dst, torch.int32, "tw_dst"),
                                                    e_all.data_ptr(), H_all.data_ptr(),
                                                    Q_all.data_ptr(), None if e_out is None else e_out.data_ptr(),
                                                    workspace.data_ptr(), workspace.numel(), st))
    return e_all, H_all, Q_all, e_out


def plan_build_workspace_bytes(n_hits, n_segments, chunk_segments):
    return int(load().gnn_plan_build_workspace_bytes(n_hits, n_segments, chunk_segments))


def plan_build_sizes(src, dst, hit_ptr, n_hits, n_segments, n_graphs, tile_hits, iter_records,
                     chunk_segments, edge_records, workspace, seg_ptr=None, max_graph_hits=0, max_graph_segments=0):
    """Stage 1 of the GPU plan builder (csrc/plan_build.hip).  Returns a GnnPlanSizes read back from
    the device - the ONE host synchronisation of a plan build.  With `seg_ptr` (device int64 [G+1]) the
    graph-local form runs (gnn_plan_build_sizes_graphs); status bit GNN_PLAN_ST_FAST_MISS = call again without."""
    sizes = torch.zeros(ctypes.sizeof(GnnPlanSizes) // 8, dtype=torch.int64, device=src.device)
    with _on(src) as st:
        ptrs = (_dev(src, torch.int32, "src"), _dev(dst, torch.int32, "dst"), _dev(hit_ptr, torch.int64, "hit_ptr"))
        rest = (n_hits, n_segments, n_graphs, tile_hits, iter_records, chunk_segments, edge_records,
                workspace.data_ptr(), workspace.numel(), sizes.data_ptr(), st)
        if seg_ptr is not None:
            _check(load().gnn_plan_build_sizes_graphs(*ptrs, _dev(seg_ptr, torch.int64, "seg_ptr"), int(max_graph_hits),
                                                      int(max_graph_segments), *rest))
        else:
            _check(load().gnn_plan_build_sizes(*ptrs, *rest))
    return _read_back(GnnPlanSizes, sizes)[0]


def graph_build_sizes(r, phi, z, layer, event_ptr, pairs, n_layers, n_phi_sectors, cuts):
    """Stage 1 of the graph builder (csrc/graph_build.hip): (workspace, GnnGraphBuildSizes, hit_ptr, seg_ptr) - the
    sizes struct and both offset arrays come back in ONE read-back.  pairs: host int32 [P, 2]; cuts: (phi_slope_max,
    phi_slope_outer_max, z0_max)."""
    dev, n, E = r.device, int(r.shape[0]), int(event_ptr.shape[0]) - 1
    pairs = np.ascontiguousarray(pairs, dtype=np.int32)
    pp = pairs.ctypes.data if pairs.size else None
    G = E * n_phi_sectors
    ws = _workspace(dev, load().gnn_graph_build_workspace_bytes(n, E, pp, pairs.shape[0], n_layers, n_phi_sectors))
    nw = ctypes.sizeof(GnnGraphBuildSizes) // 8
    out = torch.empty(nw + 2 * (G + 1), dtype=torch.int64, device=dev)
    with _on(r) as st:
        _check(load().gnn_graph_build_sizes(
            *_rphiz(r, phi, z), _dev(layer, torch.int32, "layer"), n, _dev(event_ptr, torch.int64, "event_ptr"), E, pp,
            pairs.shape[0], n_layers, n_phi_sectors, *cuts, ws.data_ptr(), ws.numel(), out.data_ptr(),
            out[nw:].data_ptr(), out[nw + G + 1:].data_ptr(), st))
    sizes, host = _read_back(GnnGraphBuildSizes, out)
    return ws, sizes, host[nw:nw + G + 1].copy(), host[nw + G + 1:].copy()


def graph_build_fill(ws, sizes, particle_id, event_ptr, pairs, n_layers, n_phi_sectors, cuts, feature_scale, n_hits):
    """Stage 2: (X [N, 3], src, dst [E] int32, y [E] or None, hit_index [N] int64), N and E from `sizes`."""
    dev = ws.device
    N, E = int(sizes.n_hits), int(sizes.n_segments)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32)
    X = torch.empty((N, 3), dtype=torch.float32, device=dev)
    src = torch.empty(E, dtype=torch.int32, device=dev)
    dst = torch.empty(E, dtype=torch.int32, device=dev)
    y = None if particle_id is None else torch.empty(E, dtype=torch.float32, device=dev)
    hit_index = torch.empty(N, dtype=torch.int64, device=dev)
    with _on(ws) as st:
        _check(load().gnn_graph_build_fill(
            None if particle_id is None else _dev(particle_id, torch.int64, "particle_id"), n_hits,
            int(event_ptr.shape[0]) - 1, pairs.ctypes.data if pairs.size else None, pairs.shape[0], n_layers,
            n_phi_sectors, *cuts, *feature_scale, ctypes.byref(sizes), ws.data_ptr(), ws.numel(), X.data_ptr(), src.data_ptr(), dst.data_ptr(),
            None if y is None else y.data_ptr(), hit_index.data_ptr(), st))
    return X, src, dst, y, hit_index


def hit_samples_sizes(r, phi, z, layer, particle_id, event_ptr, n_det_layers, n_layer_hits):
    """Stage 1 of the hit-sample builder (csrc/hit_samples.hip): (workspace, GnnHitSamplesSizes) - the sizes come
    back in ONE read-back."""
    dev, n, E = r.device, int(r.shape[0]), int(event_ptr.shape[0]) - 1
    ws = _workspace(dev, load().gnn_hit_samples_workspace_bytes(n, E, n_det_layers, n_layer_hits))
    out = torch.empty(ctypes.sizeof(GnnHitSamplesSizes) // 8, dtype=torch.int64, device=dev)
    with _on(r) as st:
        _check(load().gnn_hit_samples_sizes(
            *_rphiz(r, phi, z), _dev(layer, torch.int32, "layer"), _dev(particle_id, torch.int64, "particle_id"), n,
            _dev(event_ptr, torch.int64, "event_ptr"), E, n_det_layers, n_layer_hits, ws.data_ptr(), ws.numel(),
            out.data_ptr(), st))
    return ws, _read_back(GnnHitSamplesSizes, out)[0]


def hit_samples_fill(ws, sizes, r, phi, z, particle_id, n_events, n_det_layers, n_layer_hits, n_seed_layers,
                     feature_scale):
    """Stage 2: (X [N, 4], y [N], hit_index [N] int64, src, dst [E] int32, keys [S, 2] int64), S, N and E from
    `sizes`."""
    dev = ws.device
    S, N, E = int(sizes.n_samples), int(sizes.n_hits), int(sizes.n_segments)
    X = torch.empty((N, 4), dtype=torch.float32, device=dev)
    y = torch.empty(N, dtype=torch.float32, device=dev)
    hit_index = torch.empty(N, dtype=torch.int64, device=dev)
    src = torch.empty(E, dtype=torch.int32, device=dev)
    dst = torch.empty(E, dtype=torch.int32, device=dev)
    keys = torch.empty((S, 2), dtype=torch.int64, device=dev)
    with _on(ws) as st:
        _check(load().gnn_hit_samples_fill(
            *_rphiz(r, phi, z), _dev(particle_id, torch.int64, "particle_id"), int(r.shape[0]), n_events, n_det_layers,
            n_layer_hits, n_seed_layers, *feature_scale, ctypes.byref(sizes), ws.data_ptr(), ws.numel(), X.data_ptr(),
            y.data_ptr(), hit_index.data_ptr(), src.data_ptr(), dst.data_ptr(), keys.data_ptr(), st))
    return X, y, hit_index, src, dst, keys


def event_graphs_sizes(r, phi, z, volid, layid, barcode, event_ptr, cuts, bounds):
    """Stage 1 of the full-event graph builder (csrc/event_graphs.hip): (workspace, GnnEventGraphsSizes, hit_ptr,
    seg_ptr, event_index) - the sizes struct and both offset arrays come back in ONE read-back; event_index stays on
    the device.  cuts: (dphi_max, dz_max); bounds: (n_nodes_min, n_nodes_max, n_edges_max) as the library takes them."""
    dev, n, E = r.device, int(r.shape[0]), int(event_ptr.shape[0]) - 1
    ws = _workspace(dev, load().gnn_event_graphs_workspace_bytes(n, E))
    nw = ctypes.sizeof(GnnEventGraphsSizes) // 8
    out = torch.empty(nw + 3 * (E + 1), dtype=torch.int64, device=dev)
    with _on(r) as st:
        _check(load().gnn_event_graphs_sizes(
            *_rphiz(r, phi, z), _dev(volid, torch.int32, "volid"), _dev(layid, torch.int32, "layid"),
            _dev(barcode, torch.int64, "barcode"), n, _dev(event_ptr, torch.int64, "event_ptr"), E, cuts[0], cuts[1], bounds[0], bounds[1], bounds[2],
            ws.data_ptr(), ws.numel(), out.data_ptr(), out[nw:].data_ptr(), out[nw + E + 1:].data_ptr(),
            out[nw + 2 * (E + 1):].data_ptr(), st))
    sizes, host = _read_back(GnnEventGraphsSizes, out[:nw + 2 * (E + 1)])
    G = int(sizes.n_graphs)
    o = nw + 2 * (E + 1)
    return ws, sizes, host[nw:nw + G + 1].copy(), host[nw + E + 1:nw + E + 2 + G].copy(), out[o:o + G].clone()


def event_graphs_fill(ws, sizes, r, phi, z, barcode, n_events, cuts, feature_scale):
    """Stage 2: (X [N, 3], src, dst [S] int32, y [S], hit_index [N] int64, layer [N] int32), N and S from `sizes`."""
    dev = ws.device
    N, S = int(sizes.n_hits), int(sizes.n_segments)
    X = torch.empty((N, 3), dtype=torch.float32, device=dev)
    src = torch.empty(S, dtype=torch.int32, device=dev)
    dst = torch.empty(S, dtype=torch.int32, device=dev)
    y = torch.empty(S, dtype=torch.float32, device=dev)
    hit_index = torch.empty(N, dtype=torch.int64, device=dev)
    layer = torch.empty(N, dtype=torch.int32, device=dev)
    with _on(ws) as st:
        _check(load().gnn_event_graphs_fill(
            *_rphiz(r, phi, z), _dev(barcode, torch.int64, "barcode"), int(r.shape[0]), n_events, cuts[0], cuts[1],
            *feature_scale, ctypes.byref(sizes), ws.data_ptr(), ws.numel(), X.data_ptr(), src.data_ptr(),
            dst.data_ptr(), y.data_ptr(), hit_index.data_ptr(), layer.data_ptr(), st))
    return X, src, dst, y, hit_index, layer


SELECT_HITS_MAX_LAYERS = GNN_SELECT_HITS_MAX_LAYERS


def select_hits_sizes(hits, truth, particles, event_ptrs, barrel_layers, pt_min, no_missing_hits):
    """Stage 1 of the hit selection (csrc/select_hits.hip): (workspace, GnnSelectHitsSizes, event_ptr of the selected
    hits as a host int64 array) - both come back in ONE read-back.  hits: (hit_id int64, x, y, volume_id, layer_id),
    truth: (hit_id, particle_id), particles: (particle_id, px, py), all device columns; event_ptrs: the three tables'
    device int64 [E + 1]; barrel_layers: host int32 [L, 2]."""
    hid, x, y, vol, lay = hits
    thid, tpid = truth
    pid, px, py = particles
    dev, n, nt, npart = x.device, int(x.shape[0]), int(thid.shape[0]), int(pid.shape[0])
    E = int(event_ptrs[0].shape[0]) - 1
    tab = np.ascontiguousarray(barrel_layers, dtype=np.int32).reshape(-1, 2)
    ws = _workspace(dev, load().gnn_select_hits_workspace_bytes(n, nt, npart, E))
    nw = ctypes.sizeof(GnnSelectHitsSizes) // 8
    out = torch.empty(nw + E + 1, dtype=torch.int64, device=dev)
    i64, f32, i32 = torch.int64, torch.float32, torch.int32
    with _on(x) as st:
        _check(load().gnn_select_hits_sizes(
            _dev(hid, i64, "hits hit_id"), _dev(x, f32, "x"), _dev(y, f32, "y"), _dev(vol, i32, "volume_id"),
            _dev(lay, i32, "layer_id"), n, _dev(event_ptrs[0], i64, "hits event_ptr"),
            _dev(thid, i64, "truth hit_id"), _dev(tpid, i64, "truth particle_id"), nt,
            _dev(event_ptrs[1], i64, "truth event_ptr"), _dev(pid, i64, "particles particle_id"), _dev(px, f32, "px"),
            _dev(py, f32, "py"), npart, _dev(event_ptrs[2], i64, "particles event_ptr"), E, tab.ctypes.data,
            tab.shape[0], float(pt_min), int(bool(no_missing_hits)), ws.data_ptr(), ws.numel(), out.data_ptr(),
            out[nw:].data_ptr(), st))
    sizes, host = _read_back(GnnSelectHitsSizes, out)
    return ws, sizes, host[nw:].copy()


def select_hits_fill(ws, sizes, hid, x, y, z, phi, n_truth, n_particles, n_events, no_missing_hits):
    """Stage 2: (r, phi, z float32, layer int32, particle_id, hit_id, row int64), n_kept entries each."""
    dev, K = ws.device, int(sizes.n_kept)
    f32, i64 = torch.float32, torch.int64
    r, ophi, oz = (torch.empty(K, dtype=f32, device=dev) for _ in range(3))
    layer = torch.empty(K, dtype=torch.int32, device=dev)
    opid, ohid, row = (torch.empty(K, dtype=i64, device=dev) for _ in range(3))
    with _on(ws) as st:
        _check(load().gnn_select_hits_fill(
            _dev(hid, i64, "hits hit_id"), _dev(x, f32, "x"), _dev(y, f32, "y"), _dev(z, f32, "z"),
            None if phi is None else _dev(phi, f32, "phi"), int(x.shape[0]), n_truth, n_particles, n_events,
            int(bool(no_missing_hits)), ctypes.byref(sizes), ws.data_ptr(), ws.numel(), r.data_ptr(), ophi.data_ptr(),
            oz.data_ptr(), layer.data_ptr(), opid.data_ptr(), ohid.data_ptr(), row.data_ptr(), st))
    return r, ophi, oz, layer, opid, ohid, row


def _emtf_hits(cols, n_rows):
    """GnnEmtfHits of one source's validated device columns (muon_graph._columns)."""
    h = GnnEmtfHits()
    for field, name in (("z", "vh_sim_z"), ("theta", "vh_sim_theta"), ("phi", "vh_sim_phi"), ("r", "vh_sim_r")):
        setattr(h, field, _dev(cols[name], torch.float32, name))
    for field, name in (("bend", "vh_bend"), ("tp1", "vh_sim_tp1"), ("tp2", "vh_sim_tp2"), ("station", "vh_station"),
                        ("ring", "vh_ring"), ("type", "vh_type")):
        setattr(h, field, _dev(cols[name], torch.int32, name))
    h.event_ptr = _dev(cols["event_ptr"], torch.int64, "event_ptr")
    h.n_rows = n_rows
    return h


def _muon_graph_out(dev, n_hits, n_segments, n_graphs):
    """Device arrays of one muon graph build and the GnnMuonGraphOut pointing at them."""
    t = {"X": torch.empty((n_hits, 11), dtype=torch.float32, device=dev),
         "src": torch.empty(n_segments, dtype=torch.int32, device=dev),
         "dst": torch.empty(n_segments, dtype=torch.int32, device=dev),
         "y": torch.empty(n_segments, dtype=torch.float32, device=dev),
         "hit_source": torch.empty(n_hits, dtype=torch.int32, device=dev),
         "hit_row": torch.empty(n_hits, dtype=torch.int64, device=dev),
         "entry": torch.empty(n_graphs, dtype=torch.int64, device=dev),
         "pt": torch.empty(n_graphs, dtype=torch.float32, device=dev),
         "eta": torch.empty(n_graphs, dtype=torch.float32, device=dev),
         "flags": torch.empty(n_graphs, dtype=torch.int32, device=dev),
         "graph_hits": torch.empty(n_graphs, dtype=torch.int32, device=dev),
         "graph_segments": torch.empty(n_graphs, dtype=torch.int32, device=dev)}
    o = GnnMuonGraphOut()
    for k, v in t.items():
        setattr(o, k, v.data_ptr() if v.numel() else None)
    return t, o


def _muon_graphs(t, hit_ptr, seg_ptr, layout, entry_start, status=None, layout_ptrs=None):
    from .hitgraph import HitGraphBatch
    from .muon_graph import MG_GRAPH_PRESENT, MG_GRAPH_VP_MISSING, MG_GRAPH_WRITTEN, MuonGraphs
    batch = HitGraphBatch._from_device_arrays(t["X"], t["src"], t["dst"], t["y"], hit_ptr, seg_ptr, layout_ptrs=layout_ptrs)
    f = t["flags"]
    return MuonGraphs(batch, t["entry"], t["pt"], t["eta"], (f & MG_GRAPH_WRITTEN) != 0,
                      (f & MG_GRAPH_VP_MISSING) != 0, t["hit_source"], t["hit_row"], layout=layout,
                      present=(f & MG_GRAPH_PRESENT) != 0, n_hits=t["graph_hits"], n_segments=t["graph_segments"],
                      status=status, entry_start=entry_start)


def _muon_graph_begin(mu, pu, n_entries, n_mu, n_pu, muon_only, vp, entry_start):
    """What both muon graph builds start with, inside `_on`: (workspace, the entry points' leading arguments muon, pu,
    n_entries, muon_only, their arguments vp_pt, vp_eta, n_vp, entry_start)."""
    ws = _workspace(mu["vh_sim_z"].device, load().gnn_muon_graph_workspace_bytes(n_entries))
    hits = (ctypes.byref(_emtf_hits(mu, n_mu)), ctypes.byref(_emtf_hits(pu, n_pu)), n_entries, int(muon_only))
    vps = (_dev(vp[0], torch.float32, "vp_pt"), _dev(vp[1], torch.float32, "vp_eta"), int(vp[0].shape[0]), entry_start)
    return ws, hits, vps


def muon_graph_flat(mu, pu, n_entries, n_mu, n_pu, muon_only, vp, entry_start):
    """The muon graph builder's two calls (csrc/muon_graph.hip) around ONE read-back of the sizes and offsets."""
    from .muon_graph import _raise_status
    dev = mu["vh_sim_z"].device
    E = n_entries
    nw = ctypes.sizeof(GnnMuonGraphSizes) // 8
    out = torch.empty(nw + 2 * (E + 1), dtype=torch.int64, device=dev)
    with _on(dev) as st:
        ws, hits, vps = _muon_graph_begin(mu, pu, E, n_mu, n_pu, muon_only, vp, entry_start)
        _check(load().gnn_muon_graph_sizes(*hits, ws.data_ptr(), ws.numel(), out.data_ptr(), out[nw:].data_ptr(),
                                           out[nw + E + 1:].data_ptr(), st))
        sizes, host = _read_back(GnnMuonGraphSizes, out)
        _raise_status(int(sizes.status))
        G = int(sizes.n_graphs)
        t, o = _muon_graph_out(dev, int(sizes.n_hits), int(sizes.n_segments), G)
        _check(load().gnn_muon_graph_fill(*hits, *vps, ctypes.byref(sizes), ws.data_ptr(), ws.numel(),
                                          ctypes.byref(o), st))
    hit_ptr = host[nw:nw + G + 1].copy() if G else np.zeros(1, np.int64)
    seg_ptr = host[nw + E + 1:nw + E + 2 + G].copy() if G else np.zeros(1, np.int64)
    return _muon_graphs(t, hit_ptr, seg_ptr, "flat", entry_start)


def muon_graph_padded(mu, pu, n_entries, n_mu, n_pu, muon_only, vp, entry_start):
    """The padded build (gnn_muon_graph_padded): fixed slots, no read-back, no host synchronisation."""
    from .muon_graph import MAX_GRAPH_HITS, MAX_GRAPH_SEGMENTS
    dev = mu["vh_sim_z"].device
    E = n_entries
    status = torch.empty(1, dtype=torch.int32, device=dev)
    t, o = _muon_graph_out(dev, E * MAX_GRAPH_HITS, E * MAX_GRAPH_SEGMENTS, E)
    with _on(dev) as st:
        ws, hits, vps = _muon_graph_begin(mu, pu, E, n_mu, n_pu, muon_only, vp, entry_start)
        _check(load().gnn_muon_graph_padded(*hits, *vps, ws.data_ptr(), ws.numel(), ctypes.byref(o),
                                            status.data_ptr(), st))
        step = torch.arange(E + 1, dtype=torch.int32, device=dev)
        ptrs = torch.stack([step * MAX_GRAPH_HITS, step * MAX_GRAPH_SEGMENTS])
    hit_ptr = np.arange(E + 1, dtype=np.int64) * MAX_GRAPH_HITS
    seg_ptr = np.arange(E + 1, dtype=np.int64) * MAX_GRAPH_SEGMENTS
    return _muon_graphs(t, hit_ptr, seg_ptr, "padded", entry_start, status=status, layout_ptrs=ptrs)


def plan_build_fill(X, src, dst, n_hits, n_segments, chunk_segments, sizes, workspace, arrays):
    """Stage 2: `arrays` maps the GnnPlanOut field names to the tensors to fill (src_abs, dst_abs,
    level optional)."""
    out = GnnPlanOut()
    with _on(X) as st:
        for name, _ in GnnPlanOut._fields_:
            t = arrays.get(name)
            if t is not None:
                setattr(out, name, _dev(t, torch.float32 if name in ("X", "x_absmax") else torch.int32, name))
        _check(load().gnn_plan_build_fill(
            _dev(X, torch.float32, "X"), X.shape[1], _dev(src, torch.int32, "src"),
            _dev(dst, torch.int32, "dst"), n_hits, n_segments, chunk_segments, ctypes.byref(sizes),
            workspace.data_ptr(), workspace.numel(), ctypes.byref(out), st))


def metrics_bins(key_shift):
    """Histogram bins per class at this key shift (csrc/metrics.hip); 0 for a shift outside [10, 23]."""
    return int(load().gnn_metrics_bins(key_shift))


def segment_metrics_update(e, y, src, thresholds, key_shift, counts, hist, status, seg_ptr=None, per_graph=None):
    """One pass of gnn_segment_metrics_update: ADDS into counts [T + 1, 2] and hist [2, n_bins] (int64 views of the
    caller's counters), ORs status [1] int32, WRITES per_graph [G, T + 1, 2] when seg_ptr [G + 1] int64 is given.
    thresholds: host sequence of floats.  Asynchronous: nothing is read back."""
    n = int(e.numel())
    th = np.ascontiguousarray(thresholds, dtype=np.float32)
    G = 0 if seg_ptr is None else int(seg_ptr.numel()) - 1
    need = int(load().gnn_metrics_workspace_bytes(n, th.size, key_shift, G))
    with _on(e) as st:
        ws = torch.empty(need, dtype=torch.uint8, device=e.device) if need else None
        _check(load().gnn_segment_metrics_update(
            _dev(e, torch.float32, "scores"), _dev(y, torch.float32, "targets"),
            None if src is None else _dev(src, torch.int32, "src"), n, th.ctypes.data if th.size else None, th.size,
            key_shift, _dev(counts, torch.int64, "counts"), _dev(hist, torch.int64, "hist"),
            None if seg_ptr is None else _dev(seg_ptr, torch.int64, "seg_ptr"), G,
            None if per_graph is None else _dev(per_graph, torch.int64, "per_graph"),
            _dev(status, torch.int32, "status"), None if ws is None else ws.data_ptr(), need, st))


# ---- track candidates and their matching (csrc/track_build.hip) ---------------------------------------------------------
TRACKS_MODES = {"components": GNN_TRACKS_COMPONENTS, "best": GNN_TRACKS_BEST}


def track_build_labels(src, dst, scores, n_hits, hit_ptr, threshold, mode, min_hits):
    """gnn_track_build_labels: (workspace, root [n_hits] int32, track_of_hit [n_hits] int32, sizes [4] int64 =
    n_tracks, hits in tracks, kept segments, status) - all on the device, asynchronous, nothing read back.
    hit_ptr: device int64 [G + 1]."""
    dev, i32 = scores.device, torch.int32
    E, G = int(scores.numel()), int(hit_ptr.numel()) - 1
    ws = _workspace(dev, load().gnn_track_build_workspace_bytes(n_hits, E))
    root = torch.empty(n_hits, dtype=i32, device=dev)
    track_of_hit = torch.empty(n_hits, dtype=i32, device=dev)
    sizes = torch.empty(4, dtype=torch.int64, device=dev)
    with _on(scores) as st:
        _check(load().gnn_track_build_labels(
            _dev(src, i32, "src"), _dev(dst, i32, "dst"), _dev(scores, torch.float32, "scores"), E, n_hits,
            _dev(hit_ptr, torch.int64, "hit_ptr"), G, float(threshold), TRACKS_MODES[mode], int(min_hits),
            ws.data_ptr(), ws.numel(), root.data_ptr(), track_of_hit.data_ptr(), sizes.data_ptr(), st))
    return ws, root, track_of_hit, sizes


def track_build_lists(ws, track_of_hit, hit_ptr, n_tracks, n_track_hits):
    """gnn_track_build_lists from the host copy of the sizes: (track_ptr [n_tracks + 1], track_hits [n_track_hits],
    track_graph [n_tracks], graph_track_ptr [G + 1]), int32."""
    dev, i32 = track_of_hit.device, torch.int32
    n, G = int(track_of_hit.numel()), int(hit_ptr.numel()) - 1
    track_ptr = torch.empty(n_tracks + 1, dtype=i32, device=dev)
    track_hits = torch.empty(n_track_hits, dtype=i32, device=dev)
    track_graph = torch.empty(n_tracks, dtype=i32, device=dev)
    graph_track_ptr = torch.empty(G + 1, dtype=i32, device=dev)
    with _on(track_of_hit) as st:
        _check(load().gnn_track_build_lists(
            _dev(track_of_hit, i32, "track_of_hit"), n, _dev(hit_ptr, torch.int64, "hit_ptr"), G, n_tracks, n_track_hits,
            ws.data_ptr(), ws.numel(), track_ptr.data_ptr(), track_hits.data_ptr(), track_graph.data_ptr(),
            graph_track_ptr.data_ptr(), st))
    return track_ptr, track_hits, track_graph, graph_track_ptr


def track_match(track_of_hit, particle_id, hit_ptr, track_ptr, n_tracks, min_hits):
    """gnn_track_match: (majority_particle int64, majority_hits, particle_hits, matched int32 - [n_tracks] each -
    counts [4] int64), on the device, asynchronous."""
    dev, i32, i64 = track_of_hit.device, torch.int32, torch.int64
    n, G = int(track_of_hit.numel()), int(hit_ptr.numel()) - 1
    ws = _workspace(dev, load().gnn_track_match_workspace_bytes(n, n_tracks))
    maj = torch.empty(n_tracks, dtype=i64, device=dev)
    maj_hits, part_hits, matched = (torch.empty(n_tracks, dtype=i32, device=dev) for _ in range(3))
    counts = torch.empty(4, dtype=i64, device=dev)
    with _on(track_of_hit) as st:
        _check(load().gnn_track_match(
            _dev(track_of_hit, i32, "track_of_hit"), _dev(particle_id, i64, "particle_id"), n,
            _dev(hit_ptr, i64, "hit_ptr"), G, _dev(track_ptr, i32, "track_ptr"), n_tracks, int(min_hits), ws.data_ptr(),
            ws.numel(), maj.data_ptr(), maj_hits.data_ptr(), part_hits.data_ptr(), matched.data_ptr(), counts.data_ptr(),
            st))
    return maj, maj_hits, part_hits, matched, counts


def track_fit(track_ptr, track_hits, x, y, z, max_hits):
    """gnn_track_fit (csrc/track_fit.hip): (moments float64 [n_tracks, 13], params float64 [n_tracks, 8], n_fit int32
    [n_tracks], status int32 [n_tracks]) on the device, asynchronous, nothing read back.  track_ptr, track_hits: device
    int32; x, y, z: device float64 [n_hits]."""
    dev, i32, f64 = track_ptr.device, torch.int32, torch.float64
    n_tracks, n_track_hits, n = int(track_ptr.numel()) - 1, int(track_hits.numel()), int(x.numel())
    if int(y.numel()) != n or int(z.numel()) != n or n_tracks < 0:
        raise GnnHipError("track_fit: x, y and z must have one entry per hit, track_ptr at least one")
    moments = torch.empty((n_tracks, 13), dtype=f64, device=dev)
    params = torch.empty((n_tracks, 8), dtype=f64, device=dev)
    n_fit = torch.empty(n_tracks, dtype=i32, device=dev)
    status = torch.empty(n_tracks, dtype=i32, device=dev)
    with _on(track_ptr) as st:
        _check(load().gnn_track_fit(
            _dev(track_ptr, i32, "track_ptr"), _dev(track_hits, i32, "track_hits"), n_tracks, n_track_hits,
            _dev(x, f64, "x"), _dev(y, f64, "y"), _dev(z, f64, "z"), n, int(max_hits), moments.data_ptr(),
            params.data_ptr(), n_fit.data_ptr(), status.data_ptr(), st))
    return moments, params, n_fit, status


# ---- choosing the graph builder's arguments (csrc/graph_build.hip gnn_cut_study, csrc/layer_census.hip) -----------------
def cut_study(r, phi, z, layer, particle_id, event_ptr, pairs, n_layers, n_phi_sectors, slope_edges, z0_edges):
    """gnn_cut_study: int64 [P * 2 * (NS + 1) * (NZ + 1) + 1] on the device, the counts and then the status word;
    asynchronous, nothing read back.  pairs: host int32 [P, 2]; the edges: device float32."""
    dev, n, E = r.device, int(r.shape[0]), int(event_ptr.shape[0]) - 1
    pairs = np.ascontiguousarray(pairs, dtype=np.int32)
    pp = pairs.ctypes.data if pairs.size else None
    NS, NZ = int(slope_edges.numel()), int(z0_edges.numel())
    ws = _workspace(dev, load().gnn_cut_study_workspace_bytes(n, E, pp, pairs.shape[0], n_layers, n_phi_sectors, NS, NZ))
    m = pairs.shape[0] * 2 * (NS + 1) * (NZ + 1)
    out = torch.empty(m + 1, dtype=torch.int64, device=dev)
    with _on(r) as st:
        _check(load().gnn_cut_study(
            *_rphiz(r, phi, z), _dev(layer, torch.int32, "layer"), _dev(particle_id, torch.int64, "particle_id"), n,
            _dev(event_ptr, torch.int64, "event_ptr"), E, pp, pairs.shape[0], n_layers, n_phi_sectors,
            _dev(slope_edges, torch.float32, "phi_slope_edges"), NS, _dev(z0_edges, torch.float32, "z0_edges"), NZ,
            ws.data_ptr(), ws.numel(), out.data_ptr(), out[m:].data_ptr(), st))
    return out


def layer_census(r, layer, particle_id, event_ptr, n_layers, skip_particle_id):
    """gnn_layer_census: int64 [L * L + 1] on the device, the table and then the status word; asynchronous."""
    dev, n, E = r.device, int(r.shape[0]), int(event_ptr.shape[0]) - 1
    ws = _workspace(dev, load().gnn_layer_census_workspace_bytes(n, E, n_layers))
    m = n_layers * n_layers
    out = torch.empty(m + 1, dtype=torch.int64, device=dev)
    with _on(r) as st:
        _check(load().gnn_layer_census(
            _dev(r, torch.float32, "r"), _dev(layer, torch.int32, "layer"),
            _dev(particle_id, torch.int64, "particle_id"), n, _dev(event_ptr, torch.int64, "event_ptr"), E, n_layers,
            int(skip_particle_id is not None), int(skip_particle_id or 0), ws.data_ptr(), ws.numel(), out.data_ptr(),
            out[m:].data_ptr(), st))
    return out


# ---- graph-convolution classifiers (csrc/gcn.hip) ---------------------------------------------------------------------
def gcn_supported(N, F, max_width, list_width):
    return bool(load().gnn_gcn_supported(N, F, max_width, list_width))


def gcn_require(N, F, max_width, list_width):
    """Raises with the limit the shape misses (gnn_last_error names it)."""
    lib = load()
    if not lib.gnn_gcn_supported(N, F, max_width, list_width):
        raise GnnHipError("no HIP kernels for this shape: %s" % lib.gnn_last_error().decode())


def gcn_compress(a):
    """Dense fp32 [B, N, N] on the device -> (row_cnt, row_idx, row_val, col_cnt, col_idx, col_val, W, status):
    the counts [B, N] int32, the lists [B, N, W] (zero-padded), W >= 1 the widest list.  ONE read-back (W and the
    status word, bit 0 = a non-finite entry) between the counting and the filling launches."""
    B, N = int(a.shape[0]), int(a.shape[1])
    dev = a.device
    lib = load()
    with _on(a) as st:
        ap = _dev(a, torch.float32, "a")
        row_cnt = torch.empty((B, N), dtype=torch.int32, device=dev)
        col_cnt = torch.empty((B, N), dtype=torch.int32, device=dev)
        info = torch.empty(2, dtype=torch.int32, device=dev)
        _check(lib.gnn_gcn_compress_count(ap, B, N, row_cnt.data_ptr(), col_cnt.data_ptr(), info.data_ptr(), st))
        width, status = (int(v) for v in info.cpu().numpy())
        W = max(1, width)
        idx = torch.zeros((2, B, N, W), dtype=torch.int32, device=dev)
        val = torch.zeros((2, B, N, W), dtype=torch.float32, device=dev)
        if status == 0:
            _check(lib.gnn_gcn_compress_fill(ap, B, N, W, idx[0].data_ptr(), val[0].data_ptr(), idx[1].data_ptr(),
                                             val[1].data_ptr(), st))
    return row_cnt, idx[0], val[0], col_cnt, idx[1], val[1], W, status


def gcn_adj_struct(adj):
    """gnn_gcn_adj_t of a SparseAdjacency (or a batch slice of one: the lists of a slice are views)."""
    s = GnnGcnAdj()
    for n in ("row_cnt", "row_idx", "col_cnt", "col_idx"):
        setattr(s, n, _dev(getattr(adj, n), torch.int32, n))
    s.row_val = _dev(adj.row_val, torch.float32, "row_val")
    s.col_val = _dev(adj.col_val, torch.float32, "col_val")
    s.B, s.N, s.W = len(adj), adj.n_nodes, adj.width
    return s


def gcn_net_struct(F, dims, residual, self_int, Wf, bf, layers, Wc, bc):
    """gnn_gcn_net_t: `layers` = [(Wn, bn, Wg)] (GraphConvSelfInt) or [(None, bl, Wl)] (GraphConv), float32 device
    tensors; the gradient offsets follow the module's parameter order."""
    if len(dims) - 1 > GNN_GCN_MAX_LAYERS:
        raise GnnHipError("no HIP kernels for this shape: %d graph-convolution layers, the kernels take at most %d"
                          % (len(dims) - 1, GNN_GCN_MAX_LAYERS))
    s = GnnGcnNet()
    f32 = torch.float32
    s.Wf, s.bf = _dev(Wf, f32, "feature_extractor.weight"), _dev(bf, f32, "feature_extractor.bias")
    s.Wc, s.bc = _dev(Wc, f32, "classifier.weight"), _dev(bc, f32, "classifier.bias")
    s.off_f, s.off_bf = 0, Wf.numel()
    off = Wf.numel() + bf.numel()
    for l, (Wn, bn, Wg) in enumerate(layers):
        cin = dims[l] + (F if residual else 0)
        if tuple(Wg.shape) != (dims[l + 1], cin) or bn.numel() != dims[l + 1] or \
                (Wn is not None and Wn.shape != Wg.shape):
            raise GnnHipError("layer %d: weight shapes do not match hidden_dims" % l)
        if Wn is not None:
            s.Wn[l], s.off_n[l] = _dev(Wn, f32, "node_mod.weight"), off
            off += Wn.numel()
            s.bn[l], s.off_b[l] = _dev(bn, f32, "node_mod.bias"), off
            s.Wg[l], s.off_g[l] = _dev(Wg, f32, "neighbor_mod.weight"), off + bn.numel()
        else:
            s.Wg[l], s.off_g[l] = _dev(Wg, f32, "linear.weight"), off
            s.bn[l], s.off_b[l] = _dev(bn, f32, "linear.bias"), off + Wg.numel()
        off += bn.numel() + Wg.numel()
    s.off_c, s.off_bc = off, off + Wc.numel()
    s.n_params = off + Wc.numel() + 1
    for l, d in enumerate(dims):
        s.dims[l] = d
    s.n_dims, s.F, s.residual, s.max_width = len(dims), F, int(bool(residual)), max(dims)
    return s


def gcn_forward(adj, net, x, train):
    """Logits [B, N] in one launch; with `train` also H_all [B, n_dims, N, max_width], the post-ReLU h of every
    layer (columns past a layer's width are not written)."""
    B, N = len(adj), adj.n_nodes
    gcn_require(N, net.F, net.max_width, adj.width)
    with _on(x) as st:
        a = gcn_adj_struct(adj)
        out = torch.empty((B, N), dtype=torch.float32, device=x.device)
        H_all = torch.empty((B, net.n_dims, N, net.max_width), dtype=torch.float32, device=x.device) if train else None
        _check(load().gnn_gcn_forward(ctypes.byref(a), ctypes.byref(net), _dev(x, torch.float32, "x"), out.data_ptr(),
                                      None if H_all is None else H_all.data_ptr(), st))
    return out, H_all


def gcn_backward(adj, net, x, H_all, grad_out):
    """The flat gradient [n_params] (module parameter order): one backward launch and one fixed-order reduction."""
    lib = load()
    with _on(x) as st:
        a = gcn_adj_struct(adj)
        need = int(lib.gnn_gcn_backward_workspace_bytes(len(adj), net.n_params))
        ws = _workspace(x.device, need)
        grads = torch.empty(net.n_params, dtype=torch.float32, device=x.device)
        _check(lib.gnn_gcn_backward(ctypes.byref(a), ctypes.byref(net), _dev(x, torch.float32, "x"),
                                    _dev(H_all, torch.float32, "H_all"), _dev(grad_out, torch.float32, "grad_out"),
                                    grads.data_ptr(), ws.data_ptr(), ws.numel(), st))
    return grads


GNN_TOY_NORMS = {None: GNN_TOY_NORM_NONE, "row": GNN_TOY_NORM_ROW, "kw": GNN_TOY_NORM_KW}


def toy_list_width(kind, L, T, norm=None):
    """The list width of a toy builder, min(2 T [+ 1 for "kw"], nodes); raises with the limit the shape misses."""
    lib = load()
    W = int(lib.gnn_toy_graphs_list_width(kind, L, T, GNN_TOY_NORMS[norm]))
    if W == 0:
        raise GnnHipError("no HIP kernels for this shape: %s" % lib.gnn_last_error().decode())
    return W


def toy_segment_graphs(hit_x, hit_y, det_r, L, T, two_sigma2):
    """gnn_toy_segment_graphs: (X [E, S, 5], y [E, S], row_cnt [E, S], row_idx, row_val [E, S, W]); one launch, nothing
    read back.  hit_x float32 [E, L T], hit_y int32 [E, L T], det_r float32 [L], all on one device."""
    E, dev = int(hit_x.shape[0]), hit_x.device
    S, W = T * T * (L - 1), toy_list_width(GNN_TOY_SEGMENTS, L, T)
    with _on(hit_x) as st:
        X = torch.empty((E, S, 5), dtype=torch.float32, device=dev)
        y = torch.empty((E, S), dtype=torch.float32, device=dev)
        cnt = torch.empty((E, S), dtype=torch.int32, device=dev)
        idx = torch.empty((E, S, W), dtype=torch.int32, device=dev)
        val = torch.empty((E, S, W), dtype=torch.float32, device=dev)
        _check(load().gnn_toy_segment_graphs(_dev(hit_x, torch.float32, "hit_x"), _dev(hit_y, torch.int32, "hit_y"),
                                             _dev(det_r, torch.float32, "det_r"), E, L, T, two_sigma2, X.data_ptr(),
                                             y.data_ptr(), cnt.data_ptr(), idx.data_ptr(), val.data_ptr(), st))
    return X, y, cnt, idx, val


def toy_hit_graphs(hit_x, hit_y, det_r, r_norm, table, L, T, seed_size, norm, target):
    """gnn_toy_hit_graphs: (X [E, N, 3], y0 [E, N], row_cnt, row_idx, row_val, col_cnt, col_idx, col_val, n_isolated
    int64 [1] on the device); one launch, nothing read back.  hit_x, det_r float64, r_norm float32 [L], table float64
    [2 T + 2] (None for norm None)."""
    E, dev = int(hit_x.shape[0]), hit_x.device
    N, W = L * T, toy_list_width(GNN_TOY_HITS, L, T, norm)
    with _on(hit_x) as st:
        X = torch.empty((E, N, 3), dtype=torch.float32, device=dev)
        y0 = torch.empty((E, N), dtype=torch.float32, device=dev)
        cnt = torch.empty((2, E, N), dtype=torch.int32, device=dev)
        idx = torch.empty((2, E, N, W), dtype=torch.int32, device=dev)
        val = torch.empty((2, E, N, W), dtype=torch.float32, device=dev)
        n_iso = torch.empty(1, dtype=torch.int64, device=dev)
        _check(load().gnn_toy_hit_graphs(_dev(hit_x, torch.float64, "hit_x"), _dev(hit_y, torch.int32, "hit_y"),
                                         _dev(det_r, torch.float64, "det_r"), _dev(r_norm, torch.float32, "r_norm"),
                                         None if table is None else _dev(table, torch.float64, "norm_table"), E, L, T,
                                         seed_size, GNN_TOY_NORMS[norm], target, X.data_ptr(), y0.data_ptr(),
                                         cnt[0].data_ptr(), idx[0].data_ptr(), val[0].data_ptr(), cnt[1].data_ptr(),
                                         idx[1].data_ptr(), val[1].data_ptr(), n_iso.data_ptr(), st))
    return X, y0, cnt[0], idx[0], val[0], cnt[1], idx[1], val[1], n_iso


# ---- the per-iteration segment classifier (include/gnn_hip_iter.h, csrc/iter_events.hip) ---------------------------------
@functools.lru_cache(maxsize=None)
def iter_events_supported(F, D, max_hits, max_segments, backward=False):
    """True if graphs of at most that size fit the one-launch per-iteration kernels (the backward too, if asked)."""
    return bool(load().gnn_iter_events_supported(F, D, max_hits, max_segments, int(bool(backward))))


def iter_params_struct(win, bin_, edge_sets, node_sets, out_set, F, D, shared=False):
    """gnn_iter_params_t over float32 device tensors: edge_sets / node_sets are n_iters lists of the four tensors of
    one network (layer 0 weight, bias, layer 2 weight, bias), out_set the output network's four.  The struct keeps
    the tensors alive (`_keep`)."""
    C, T = F + D, len(edge_sets)
    if T > GNN_ITER_MAX or len(node_sets) != T:
        raise GnnHipError("expected at most %d edge sets and as many node sets, got %d and %d"
                          % (GNN_ITER_MAX, T, len(node_sets)))
    p = GnnIterParams()
    keep = []

    def put(dst, name, t, shape):
        n = 1
        for d in shape:
            n *= d
        if not torch.is_tensor(t) or t.numel() != n:
            # the kernels index the tensors as rows of (F, D): a mismatch is an out-of-bounds read
            raise GnnHipError("%s has %s elements, but input_dim=%d hidden_dim=%d needs shape %s"
                              % (name, t.numel() if torch.is_tensor(t) else "no", F, D, shape))
        setattr(dst, name.split(".")[-1], _dev(t, torch.float32, name))
        keep.append(t)

    put(p, "Win", win, (D, F))
    put(p, "bin", bin_, (D,))
    e_shapes, n_shapes = ((D, 2 * C), (D,), (1, D), (1,)), ((D, 3 * C), (D,), (D, D), (D,))
    for i in range(T):
        for name, t, shp in zip(("Wa", "ba", "Wb", "bb"), edge_sets[i], e_shapes):
            put(p.edge[i], "edge[%d].%s" % (i, name), t, shp)
        for name, t, shp in zip(("Wa", "ba", "Wb", "bb"), node_sets[i], n_shapes):
            put(p.node[i], "node[%d].%s" % (i, name), t, shp)
    for name, t, shp in zip(("Wa", "ba", "Wb", "bb"), out_set, e_shapes):
        put(p.out, "out.%s" % name, t, shp)
    p.F, p.D, p.n_iters, p.shared = F, D, T, int(bool(shared))
    devs = {t.device for t in keep}
    if len(devs) != 1:
        raise GnnHipError("the weight tensors must live on one device, got %s" % sorted(map(str, devs)))
    p._device, p._keep = devs.pop(), keep
    return p


def _iter_ptrs(batch, layout):
    return _dev(layout.hit_ptr, torch.int32, "hit_ptr"), _dev(layout.seg_ptr, torch.int32, "seg_ptr")


def iter_forward_events(batch, layout, ip, train=False):
    """The per-iteration forward in one launch (`layout` = batch.event_layout(), `ip` = iter_params_struct(...)):
    scores [n_segments], or with train=True (e_all [(T+1), E], H_all [(T+1), N, ldh]) - scores = e_all[-1]."""
    dev = batch.X.device
    E, N, T = batch.n_segments, batch.n_hits, ip.n_iters
    out = e_all = H_all = None
    if train:
        e_all = torch.empty((T + 1, E), dtype=torch.float32, device=dev)
        H_all = torch.empty((T + 1, N, h_stride(ip.F, ip.D)), dtype=torch.float32, device=dev)
    else:
        out = torch.empty(E, dtype=torch.float32, device=dev)
    g = cached_graph_struct(batch)
    with _on(batch.X, g, ip) as st:
        hp, sp = _iter_ptrs(batch, layout)
        _check(load().gnn_iter_forward_events(
            ctypes.byref(g), ctypes.byref(ip), hp, sp, batch.n_graphs, layout.max_hits, layout.max_segments,
            out.data_ptr() if out is not None else None, e_all.data_ptr() if train else None,
            H_all.data_ptr() if train else None, st))
    return (e_all, H_all) if train else out


def iter_backward_events(batch, layout, ip, e_all, H_all, grad_out):
    """The flat gradient (state_dict order; gnn_iter_grad_floats) of the per-iteration model in one launch and a fold."""
    dev = batch.X.device
    lib = load()
    flat = torch.empty(int(lib.gnn_iter_grad_floats(ip.F, ip.D, ip.n_iters, ip.shared)), dtype=torch.float32, device=dev)
    ws = _workspace(dev, lib.gnn_iter_backward_workspace_bytes(batch.n_graphs, ip.F, ip.D, ip.n_iters))
    g = cached_graph_struct(batch)
    with _on(batch.X, g, ip) as st:
        hp, sp = _iter_ptrs(batch, layout)
        _check(lib.gnn_iter_backward_events(
            ctypes.byref(g), ctypes.byref(ip), hp, sp, batch.n_graphs, layout.max_hits, layout.max_segments,
            _dev(e_all, torch.float32, "e_all"), _dev(H_all, torch.float32, "H_all"),
            _dev(grad_out, torch.float32, "grad_out"), flat.data_ptr(), ws.data_ptr(), ws.numel(), st))
    return flat


def iter_input_bwd(X, H0, gH0, F, D):
    """Gradients of the input network from dLoss/dH0: flat [D*F + D] = gWin [D, F] then gbin [D] (gnn_iter_input_bwd)."""
    n = X.shape[0]
    lib = load()
    flat = torch.empty(D * F + D, dtype=torch.float32, device=X.device)
    ws = _workspace(X.device, lib.gnn_iter_input_bwd_workspace_bytes(n, F, D))
    with _on(X) as st:
        _check(lib.gnn_iter_input_bwd(_dev(X, torch.float32, "X"), _dev(H0, torch.float32, "H0"), H0.shape[1],
                                      _dev(gH0, torch.float32, "grad_H0"), gH0.shape[1], n, F, D, flat.data_ptr(),
                                      ws.data_ptr(), ws.numel(), st))
    return flat


# ---- the fixed-point forward (include/gnn_hip_fixed.h, csrc/fixed_point.hip) -------------------------------------------
@functools.lru_cache(maxsize=None)
def fx_supported(F, D, total_bits, int_bits, table_bits):
    return bool(load().gnn_fx_supported(F, D, total_bits, int_bits, table_bits))


def fx_workspace_bytes(n_hits, n_segments, F, D):
    return int(load().gnn_fx_workspace_bytes(n_hits, n_segments, F, D))


def fx_format_struct(total_bits, int_bits, rounding, overflow, table_bits):
    return GnnFxFormat(total_bits, int_bits, GNN_FX_ROUNDING[rounding], GNN_FX_OVERFLOW[overflow], table_bits)


def fx_params_struct(weights, F, D):
    """gnn_fx_params_t over the ten quantised weight tensors (int32, state_dict order); keeps them alive (`_keep`)."""
    p = GnnFxParams()
    C = F + D
    shapes = ((D, F), (D,), (D, 2 * C), (D,), (1, D), (1,), (D, 3 * C), (D,), (D, D), (D,))
    if len(weights) != 10:
        raise GnnHipError("expected the ten weight tensors in state_dict order, got %d" % len(weights))
    for name, w, shp in zip(("Win", "bin", "W1", "b1", "W2", "b2", "W3", "b3", "W4", "b4"), weights, shapes):
        n = 1
        for d in shp:
            n *= d
        if not torch.is_tensor(w) or w.numel() != n:
            # the kernels index the tensors as [D, ...] rows of (F, D): a mismatch is an out-of-bounds read
            raise GnnHipError("%s has %s elements, but input_dim=%d hidden_dim=%d needs shape %s"
                              % (name, w.numel() if torch.is_tensor(w) else "no", F, D, shp))
        setattr(p, name, _dev(w, torch.int32, name))
    p.F, p.D = F, D
    devs = {w.device for w in weights}
    if len(devs) != 1:
        raise GnnHipError("the weight tensors must live on one device, got %s" % sorted(map(str, devs)))
    p._device, p._keep = devs.pop(), list(weights)
    return p


def fx_tables_struct(tanh_table, sigmoid_table, table_bits):
    """gnn_fx_tables_t over the two int32 device tables of 2^table_bits entries; keeps them alive (`_keep`)."""
    t = GnnFxTables()
    for name, tab in (("tanh_table", tanh_table), ("sigmoid_table", sigmoid_table)):
        if not torch.is_tensor(tab) or tab.numel() != 1 << table_bits:
            raise GnnHipError("%s must hold 2^%d entries" % (name, table_bits))       # (the kernels copy that many)
        setattr(t, name, _dev(tab, torch.int32, name))
    if tanh_table.device != sigmoid_table.device:
        raise GnnHipError("the two tables must live on one device")
    t._device, t._keep = tanh_table.device, (tanh_table, sigmoid_table)
    return t


def fx_forward(batch, params, fmt, tables, n_iters, trace=False, workspace=None):
    """gnn_fx_forward on an index-form batch (`params` = fx_params_struct(...), `fmt` = fx_format_struct(...), `tables`
    = fx_tables_struct(...)): (raw int32 [E], scores float32 [E], counts int64 [T+1, 6], e_trace int32 [T+1, E] or
    None, H_trace int32 [T+1, N, C] or None)."""
    dev = batch.X.device
    E, N, F, D = batch.n_segments, batch.n_hits, params.F, params.D
    if not fx_supported(F, D, fmt.total_bits, fmt.int_bits, fmt.table_bits):
        raise GnnHipError("no fixed-point kernel for input_dim=%d hidden_dim=%d at total_bits=%d int_bits=%d "
                          "table_bits=%d" % (F, D, fmt.total_bits, fmt.int_bits, fmt.table_bits))
    need = fx_workspace_bytes(N, E, F, D)
    if workspace is None or workspace.numel() < need:
        workspace = _workspace(dev, need)
    raw = torch.empty(E, dtype=torch.int32, device=dev)
    scores = torch.empty(E, dtype=torch.float32, device=dev)
    counts = torch.empty((n_iters + 1, GNN_FX_STAGES), dtype=torch.int64, device=dev)     # (the call zeroes them)
    et = Ht = None
    if trace:
        et = torch.empty((n_iters + 1, E), dtype=torch.int32, device=dev)
        Ht = torch.empty((n_iters + 1, N, F + D), dtype=torch.int32, device=dev)
    g = graph_struct(batch)
    with _on(batch.X, g, params, tables) as st:
        _check(load().gnn_fx_forward(ctypes.byref(g), ctypes.byref(params), ctypes.byref(fmt), ctypes.byref(tables),
                                     n_iters, raw.data_ptr(), scores.data_ptr(), counts.data_ptr(),
                                     et.data_ptr() if trace else None, Ht.data_ptr() if trace else None,
                                     _dev(workspace, torch.uint8, "workspace"), workspace.numel(), st))
    return raw, scores, counts, et, Ht


# ---- its one-launch form for small graphs (include/gnn_hip_fixed_events.h, csrc/fixed_events.hip) -----------------------
@functools.lru_cache(maxsize=None)
def fxev_lds_bytes(F, D, table_bits, max_hits, max_segments):
    """Bytes of LDS a workgroup of gnn_fxev_forward needs for graphs of at most that size (0: arguments it refuses)."""
    return int(load().gnn_fxev_lds_bytes(F, D, table_bits, max_hits, max_segments))


@functools.lru_cache(maxsize=None)
def fxev_supported(F, D, table_bits, max_hits, max_segments):
    """True if graphs of at most that size fit the one-launch fixed-point kernel."""
    return bool(load().gnn_fxev_supported(F, D, table_bits, max_hits, max_segments))


def fxev_forward(batch, layout, params, fmt, tables, n_iters, trace=False):
    """gnn_fxev_forward on a block-diagonal batch of small graphs (`layout` = batch.event_layout(); `params`, `fmt`,
    `tables` as fx_forward takes them): (raw int32 [E], scores float32 [E], counts int64 [T+1, 6], graph_overflows int64
    [n_graphs], e_trace int32 [T+1, E] or None, H_trace int32 [T+1, N, C] or None)."""
    dev = batch.X.device
    E, N, F, D = batch.n_segments, batch.n_hits, params.F, params.D
    raw = torch.empty(E, dtype=torch.int32, device=dev)
    scores = torch.empty(E, dtype=torch.float32, device=dev)
    counts = torch.empty((n_iters + 1, GNN_FX_STAGES), dtype=torch.int64, device=dev)     # (the call zeroes them)
    per_graph = torch.empty(batch.n_graphs, dtype=torch.int64, device=dev)
    et = Ht = None
    if trace:
        et = torch.empty((n_iters + 1, E), dtype=torch.int32, device=dev)
        Ht = torch.empty((n_iters + 1, N, F + D), dtype=torch.int32, device=dev)
    g = cached_graph_struct(batch)
    with _on(batch.X, g, params, tables) as st:
        hp, sp = _iter_ptrs(batch, layout)
        _check(load().gnn_fxev_forward(ctypes.byref(g), ctypes.byref(params), ctypes.byref(fmt), ctypes.byref(tables),
                                       hp, sp, batch.n_graphs, layout.max_hits, layout.max_segments, n_iters,
                                       raw.data_ptr(), scores.data_ptr(), counts.data_ptr(), per_graph.data_ptr(),
                                       et.data_ptr() if trace else None, Ht.data_ptr() if trace else None, st))
    return raw, scores, counts, per_graph, et, Ht


class profile:
    """Context manager: per-kernel HIP-event timings of everything launched inside.

    with _lib.profile(64) as prof: ...; prof.records -> [(kernel_name, ms), ...]"""

    def __init__(self, capacity=256):
        self.capacity = capacity
        self.records = []

    def __enter__(self):
        _check(load().gnn_profile_begin(self.capacity))
        return self

    def __exit__(self, *exc):
        names = (ctypes.c_char_p * self.capacity)()
        ms = (ctypes.c_float * self.capacity)()
        n = load().gnn_profile_end(names, ms, self.capacity)
        if n < 0:
            _check(n)
        self.records = [(names[i].decode(), float(ms[i])) for i in range(min(n, self.capacity))]
        return False
