"""Autograd bridge: makes the HIP forward differentiable w.r.t. the module's parameters so that
`loss.backward()` in the reference's training loop (gnn/estimator.py:57-58) works unchanged.

The training forward keeps every iteration's hit features and edge scores; the backward is
explicit HIP kernels (csrc/backward.hip).  Masks stay in autograd: the Function's inputs are the
EFFECTIVE weights `W * mask` computed with torch ops, so d/dW picks up the mask exactly like
gnn/model.py:30 does.  X gets no gradient (the reference never asks for one).
"""
import torch

from . import _lib
from .call_route import refuse_unsupported, training_route


def _trunk_weights(model):
    """The ten tensors of the trunk in state_dict order, masks applied WITH torch ops (see above)."""
    lin = model.input_network[0]
    en, nn_ = model.edge_network.network, model.node_network.network
    return [lin.weight, lin.bias,
            en[0].effective_weight(), en[0].bias, en[2].effective_weight(), en[2].bias,
            nn_[0].effective_weight(), nn_[0].bias, nn_[2].effective_weight(), nn_[2].bias]


# ---- one training forward / backward pair on a call_route.Route: what _SegClf and GradBucket.step both run ------------
def train_forward(route, w, F, D, n_iters, want_out=True):
    """(e_all, H_all, Q_all, e_out) on route.batch: e_out - the final scores in the CALLER's segment order - only from
    the twin's fused forward, and only when wanted (a loss taken in the twin's order needs no second copy)."""
    if route.kind == "twin":                # the fused tile kernels of the plan the twin was made from
        return _lib.segclf_forward_train_twin(route.batch, w, F, D, n_iters, want_out=want_out)
    # small graphs (the reference's muon events, route.layout): the whole forward in one launch; else per module
    return _lib.segclf_forward_train(route.batch, w, F, D, n_iters, layout=route.layout) + (None,)


def train_backward(route, w, F, D, n_iters, e_all, H_all, Q_all, grad_e, into=None):
    """The ten gradients (`into`: added into these ten tensors); grad_e in route.batch's segment order."""
    if route.kind == "events":              # the whole backward in one launch
        return _lib.segclf_backward_events(route.batch, route.layout, w, F, D, n_iters, e_all, H_all, grad_e, into=into)
    return _lib.segclf_backward(route.batch, w, F, D, n_iters, e_all, H_all, grad_e, into=into, Q_all=Q_all)


class _SegClf(torch.autograd.Function):
    @staticmethod
    def forward(ctx, route, F, D, n_iters, *weights):
        w = [t.detach().to(torch.float32).contiguous() for t in weights]
        e_all, H_all, Q_all, e_out = train_forward(route, w, F, D, n_iters)
        ctx.route, ctx.F, ctx.D, ctx.n_iters = route, F, D, n_iters
        ctx.save_for_backward(e_all, H_all, Q_all, *w)
        if e_out is not None:
            return e_out                                 # already in the caller's segment order
        rank = route.batch.seg_rank                      # level-ordered twin: back to the caller's segment order
        return e_all[n_iters].clone() if rank is None else e_all[n_iters].index_select(0, rank)

    @staticmethod
    def backward(ctx, grad_out):
        e_all, H_all, Q_all, *w = ctx.saved_tensors
        go = grad_out.to(torch.float32).contiguous()
        order = ctx.route.batch.seg_order
        if order is not None:
            go = go.index_select(0, order)
        grads = train_backward(ctx.route, list(w), ctx.F, ctx.D, ctx.n_iters, e_all, H_all, Q_all, go)
        return (None, None, None, None) + tuple(grads)


def segclf_apply(model, batch):
    """Differentiable forward of `model` (a gnn_fpga_amd SegmentClassifier) on `batch`."""
    F, D = model.input_dim, model.hidden_dim
    refuse_unsupported("SegmentClassifier.forward", batch.X, F, D, training=True)
    e = _SegClf.apply(training_route(model, batch), F, D, model.n_iters, *_trunk_weights(model))
    if batch.dense_shape:
        e = e.view(batch.dense_shape[0], batch.dense_shape[2])
    return e


# ---- the sub-modules on their own (reference gnn/model.py:69-81, 113-125 are ordinary autograd
# modules; the notebooks call them directly: gnn/MPNN_Seg_ACTS_maskedlinear.ipynb cells 42, 46) ------
def _pad_rows(H2, ldh):
    """[n, C] -> [n, ldh] float32 rows, zero-padded to the stride the kernels read (ldh: a multiple of 4 floats; the
    rows may start at any multiple of 4 bytes - include/gnn_hip.h, "Alignment")."""
    Hp = torch.zeros((H2.shape[0], ldh), dtype=torch.float32, device=H2.device)
    Hp[:, :H2.shape[1]] = H2
    return Hp


def _dummy_weights(F, D, dev, edge=None, node=None):
    """The C structs take all ten tensors; a sub-module owns four of them."""
    C = F + D
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)    # noqa: E731
    e = edge if edge is not None else [z(D, 2 * C), z(D), z(1, D), z(1)]
    n = node if node is not None else [z(D, 3 * C), z(D), z(D, D), z(D)]
    return [z(D, F), z(D)] + list(e) + list(n)


class _EdgeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, batch, F, D, H2, W1, b1, W2, b2):
        w = [t.detach().to(torch.float32).contiguous() for t in (W1, b1, W2, b2)]
        Hp = _pad_rows(H2.detach().to(torch.float32), _lib.h_stride(F, D))
        e = _lib.edge_fwd(Hp, batch.src, batch.dst, *w, F, D)
        ctx.batch, ctx.F, ctx.D, ctx.C = batch, F, D, H2.shape[1]
        ctx.save_for_backward(Hp, e, *w)
        return e.clone()

    @staticmethod
    def backward(ctx, ge):
        Hp, e, *w = ctx.saved_tensors
        gH, gw = _lib.edge_bwd(Hp, ctx.batch, _dummy_weights(ctx.F, ctx.D, Hp.device, edge=w), ctx.F, ctx.D, e,
                               ge.to(torch.float32).contiguous())
        return (None, None, None, gH[:, :ctx.C].contiguous()) + tuple(gw)


class _NodeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, batch, F, D, H2, e, W3, b3, W4, b4):
        w = [t.detach().to(torch.float32).contiguous() for t in (W3, b3, W4, b4)]
        Hp = _pad_rows(H2.detach().to(torch.float32), _lib.h_stride(F, D))
        ev = e.detach().to(torch.float32).contiguous().reshape(-1)
        Hn = _lib.node_fwd(Hp, ev, batch, *w, F, D)
        ctx.batch, ctx.F, ctx.D, ctx.C = batch, F, D, H2.shape[1]
        ctx.save_for_backward(Hp, ev, Hn, *w)
        return Hn[:, :D].clone()

    @staticmethod
    def backward(ctx, gHn):
        Hp, ev, Hn, *w = ctx.saved_tensors
        g = _pad_rows(gHn.to(torch.float32), Hp.shape[1])
        gH, ge, gw = _lib.node_bwd(Hp, ev, Hn, ctx.batch, _dummy_weights(ctx.F, ctx.D, Hp.device, node=w), ctx.F,
                                   ctx.D, g)
        return (None, None, None, gH[:, :ctx.C].contiguous(), ge) + tuple(gw)


# ---- NodeClassifier (gnn/MPNN_HitClassifier.ipynb cell 21): the trunk's training forward with the output network in
# place of the final edge pass, and the backward seeded from the hit scores' gradient ----------------------------
class _NodeClf(torch.autograd.Function):
    @staticmethod
    def forward(ctx, batch, F, D, n_iters, *weights):
        w = [t.detach().to(torch.float32).contiguous() for t in weights]
        e_all, H_all, Q_all, y = _lib.nodeclf_forward_train(batch, w[:10], w[10], w[11], F, D, n_iters)
        ctx.batch, ctx.F, ctx.D, ctx.n_iters = batch, F, D, n_iters
        ctx.save_for_backward(e_all, H_all, Q_all, y, *w)
        return y.clone()

    @staticmethod
    def backward(ctx, grad_y):
        e_all, H_all, Q_all, y, *w = ctx.saved_tensors
        gy = grad_y.to(torch.float32).contiguous()
        grads, gWo, gbo = _lib.nodeclf_backward(ctx.batch, w[:10], w[10], w[11], ctx.F, ctx.D, ctx.n_iters, e_all,
                                                H_all, y, gy, Q_all=Q_all)
        return (None, None, None, None) + tuple(grads) + (gWo, gbo)


def nodeclf_apply(model, batch):
    """Differentiable forward of `model` (a gnn_fpga_amd NodeClassifier) on `batch`: hit scores [n_hits]."""
    F, D = model.input_dim, model.hidden_dim
    refuse_unsupported("NodeClassifier.forward", batch.X, F, D, training=True)
    out = model.output_network[0]
    weights = _trunk_weights(model) + [out.weight, out.bias]
    return _NodeClf.apply(batch, F, D, model.n_iters, *weights)


# ---- graph-convolution classifiers (gnn/GCN_Seg_Toy2D.ipynb cells 20-21, gnn/GCN_Toy2D.ipynb cells 11-14): the whole
# model forward in one launch (csrc/gcn.hip) keeping every layer's post-ReLU h, the backward in one launch plus one
# fixed-order reduction over the graphs.  No gradient for x or the adjacency -----------------------------------------
def _gcn_net(model, params):
    """gnn_gcn_net_t of a GCN/GCRNBinaryClassifier over `params` (its parameters, module order, detached)."""
    from .gcn import GraphConvSelfInt
    it = iter(params)
    Wf, bf = next(it), next(it)
    self_int = all(isinstance(gc, GraphConvSelfInt) for gc in model.gc_layers)
    layers = []
    for _ in model.gc_layers:
        if self_int:
            Wn, bn, Wg = next(it), next(it), next(it)          # node_mod.weight, node_mod.bias, neighbor_mod.weight
            layers.append((Wn, bn, Wg))
        else:
            Wl, bl = next(it), next(it)                        # linear.weight, linear.bias
            layers.append((None, bl, Wl))
    Wc, bc = next(it), next(it)
    return _lib.gcn_net_struct(model.input_dim, model.hidden_dims, model.residual, self_int, Wf, bf, layers, Wc, bc)


class _Gcn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, adj, x, *params):
        w = [t.detach().to(torch.float32).contiguous() for t in params]
        net = _gcn_net(model, w)
        out, H_all = _lib.gcn_forward(adj, net, x, train=True)
        ctx.model, ctx.adj, ctx.shapes = model, adj, [p.shape for p in params]
        ctx.save_for_backward(x, H_all, *w)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, H_all, *w = ctx.saved_tensors
        net = _gcn_net(ctx.model, w)
        flat = _lib.gcn_backward(ctx.adj, net, x, H_all, grad_out.to(torch.float32).contiguous())
        grads, off = [], 0
        for k, t in enumerate(w):                              # (the flat gradient is in module parameter order)
            grads.append(flat[off:off + t.numel()].view(ctx.shapes[k]))
            off += t.numel()
        return (None, None, None) + tuple(grads)


def gcn_apply(model, x, a):
    """Forward of a gnn_fpga_amd GCN/GCRNBinaryClassifier: logits [B, N].  `a`: a SparseAdjacency (fast) or a dense
    [B, N, N] tensor (compressed on every call: slow).  Differentiable w.r.t. the parameters in training mode."""
    from .gcn import GraphConv, GraphConvSelfInt, SparseAdjacency, compress_adjacency
    name = type(model).__name__
    if not torch.is_tensor(x) or not x.is_cuda:
        raise _lib.GnnHipError("%s.forward needs tensors on a ROCm device; there is no CPU path" % name)
    if x.requires_grad:
        raise _lib.GnnHipError("%s: x requires grad, and the kernels have no gradient for it" % name)
    if not isinstance(a, SparseAdjacency):
        a = compress_adjacency(a)                     # (raises for CPU tensors and for a.requires_grad)
    if x.dim() != 3 or x.shape[2] != model.input_dim or x.shape[0] != len(a) or x.shape[1] != a.n_nodes:
        raise _lib.GnnHipError("%s: x %s does not match input_dim %d and the adjacency %s"
                               % (name, tuple(x.shape), model.input_dim, a.shape))
    if a.device != x.device:
        raise _lib.GnnHipError("%s: x is on %s, the adjacency on %s" % (name, x.device, a.device))
    kinds = {type(gc) for gc in model.gc_layers}
    if len(kinds) > 1 or not kinds <= {GraphConv, GraphConvSelfInt}:
        raise _lib.GnnHipError("%s: the layers must all be GraphConv or all GraphConvSelfInt" % name)
    x = x.to(torch.float32).contiguous()
    params = list(model.parameters())
    _lib.gcn_require(a.n_nodes, model.input_dim, max(model.hidden_dims), a.width)
    if model.training and torch.is_grad_enabled() and any(p.requires_grad for p in params):
        return _Gcn.apply(model, a, x, *params)
    w = [p.detach().to(torch.float32).contiguous() for p in params]
    return _lib.gcn_forward(a, _gcn_net(model, w), x, train=False)[0]


def gcn_forward_layers(model, x, a):
    """(logits [B, N], [h_0 .. h_L]) - the post-ReLU h of every layer, [B, N, hidden_dims[l]], as the training
    forward keeps them (what the tests compare with the reference's per-layer activations)."""
    from .gcn import SparseAdjacency, compress_adjacency
    if not isinstance(a, SparseAdjacency):
        a = compress_adjacency(a)
    w = [p.detach().to(torch.float32).contiguous() for p in model.parameters()]
    out, H_all = _lib.gcn_forward(a, _gcn_net(model, w), x.to(torch.float32).contiguous(), train=True)
    return out, [H_all[:, l, :, :d] for l, d in enumerate(model.hidden_dims)]
