"""The toy MPNN notebook's classifiers and data cells (reference gnn/MPNN_Seg_Toy2D.ipynb), HIP forward and backward.

Cell 14 defines two segment classifiers.  `SegmentClassifier` gives every iteration its own `edge_networks[i]` and
`node_networks[i]` and scores with a separate `output_network` (4 + 8 T + 2 state_dict tensors: 86 and 68 267
parameters at the notebook's input_dim 2, hidden_dim 32, n_iters 10); `SegmentClassifier2` shares one edge and one
node network across the iterations (the ten keys of `model.SegmentClassifier`, no masks).  Both are drop-ins here:
same constructor signatures, sub-module trees and state_dict keys, so a checkpoint of either loads.

Routes, decided once per call by `call_route.choose_iter` and left on the model as `_route.kind`:

  "iter_events"  the whole forward - and, when training, the whole backward - in ONE launch, one workgroup per graph,
                 a different weight set staged into LDS per pass (csrc/iter_events.hip).  Taken when `use_events` is
                 set, 0 < n_graphs <= call_route.EVENTS_MAX_GRAPHS, the batch is block-diagonal
                 (`batch.event_layout()`), n_iters <= _lib.GNN_ITER_MAX and the largest graph fits one workgroup's
                 LDS (`_lib.iter_events_supported`; with 4 segments per hit: 49 hits when training at hidden_dim 32,
                 96 for inference; 176 and 316 at hidden_dim 8).
  "per_module"   otherwise: the notebook's forward written with `model.EdgeNetwork` / `model.NodeNetwork` (HIP forward
                 and backward each) and gnn_input_fwd; every shape of the per-module kernels at every size.

"iter_events" is the default wherever it can run: tools/toy_mpnn_probe.py measured it faster than "per_module" at both
shapes it timed (profiles/toy_mpnn_probe.txt, one MI355X, HIP-event medians) - the notebook's batch of 32 events at
hidden_dim 32, n_iters 10: 0.36 against 1.06 ms per inference forward, 2.03 against 6.54 ms per training step; 512
muon-size graphs at input_dim 11, hidden_dim 8, n_iters 3: 0.12 against 0.40 ms and 1.04 against 2.12 ms.

`build_toy_mpnn_graphs` is cells 8, 11 and 12 on the device: hits -> X = [x, r], the all-pairs-of-adjacent-layers
segments in np.where's order, the edge labels and the segment lists, as a `HitGraphBatch` in event layout.
`synth.toy_mpnn_graphs_from_hits` is its numpy specification.  There is no CPU path: CPU tensors raise.
"""
from collections import namedtuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib, synth
from .call_route import iter_route, refuse_unsupported
from .hitgraph import HitGraphBatch
from .model import EdgeNetwork, NodeNetwork, _as_batch, _require_tanh
from .toy_graphs import _det_r, _hits

ToyMpnnGraphs = namedtuple("ToyMpnnGraphs", ["batch", "y"])


class _InputFn(torch.autograd.Function):
    """input_network and the shortcut (cell 14): X [N, F] -> [tanh(Win X + bin) | X] [N, C]; HIP both ways."""

    @staticmethod
    def forward(ctx, X, Win, bin_):
        F, D = X.shape[1], Win.shape[0]
        Hp = _lib.input_fwd(X, Win.detach().contiguous(), bin_.detach().contiguous())
        ctx.save_for_backward(X, Hp)
        ctx.F, ctx.D = F, D
        return Hp[:, :F + D].clone()

    @staticmethod
    def backward(ctx, gH):
        X, Hp = ctx.saved_tensors
        F, D = ctx.F, ctx.D
        flat = _lib.iter_input_bwd(X, Hp, gH.to(torch.float32).contiguous(), F, D)
        return None, flat[:D * F].view(D, F), flat[D * F:]


class _IterFn(torch.autograd.Function):
    """The one-launch route: forward keeps every pass's scores and hit rows (the scores handed to autograd are a copy
    of the last row: a second, small launch), backward hands out views of one flat gradient buffer in state_dict
    order.  The pointer struct is rebuilt per call (136 pointers, host side; inside the probe's step times)."""

    @staticmethod
    def forward(ctx, model, batch, layout, *params):
        ip = model._iter_params([p.detach() for p in params])
        e_all, H_all = _lib.iter_forward_events(batch, layout, ip, train=True)
        ctx.batch, ctx.layout, ctx.ip = batch, layout, ip
        ctx.sizes = [p.numel() for p in params]
        ctx.shapes = [p.shape for p in params]
        ctx.save_for_backward(e_all, H_all)
        return e_all[ip.n_iters].clone()

    @staticmethod
    def backward(ctx, grad_out):
        e_all, H_all = ctx.saved_tensors
        flat = _lib.iter_backward_events(ctx.batch, ctx.layout, ctx.ip, e_all, H_all,
                                         grad_out.to(torch.float32).contiguous())
        grads = [g.view(s) for g, s in zip(flat.split(ctx.sizes), ctx.shapes)]
        return (None, None, None) + tuple(grads)


class _IterClassifier(nn.Module):
    """What the two classes share: inputs, the route, the one-launch call and the traces."""

    # True: batches of small graphs take the one-launch kernels ("iter_events") wherever they can run - measured 3 times
    # faster than "per_module" at the notebook's shape and at muon size (profiles/toy_mpnn_probe.txt).
    use_events = True

    def _common(self, input_dim, hidden_dim, n_iters, hidden_activation):
        _require_tanh(hidden_activation)
        self.n_iters = n_iters
        self.input_dim, self.hidden_dim = input_dim, hidden_dim
        self.input_network = nn.Sequential(nn.Linear(input_dim, hidden_dim), hidden_activation())
        self._route = None      # the kind of the last call's call_route.Route (tests / diagnostics)

    def __getstate__(self):
        st = self.__dict__.copy()
        st["_route"] = None
        return st

    def _f32_params(self):
        return [p for p in self.parameters()]

    def _iter_params(self, params):
        """gnn_iter_params_t over `params`, the model's tensors in state_dict order."""
        raise NotImplementedError

    def forward(self, inputs, trace=False):
        """Apply forward pass of the model: inputs = [X, Ri, Ro] or a HitGraphBatch.  trace=True (inference):
        (scores, e_trace [(T+1), E], H_trace [(T+1), N, C]) - every pass's scores and hit rows."""
        batch = inputs if isinstance(inputs, HitGraphBatch) else _as_batch(*inputs)
        params = self._f32_params()
        training = torch.is_grad_enabled() and any(p.requires_grad for p in params)
        refuse_unsupported("%s.forward" % type(self).__name__, batch.X, self.input_dim, self.hidden_dim, training)
        if any(p.dtype != torch.float32 or p.device != batch.X.device for p in params):
            raise _lib.GnnHipError("%s: the parameters must be float32 on the batch's device (%s)"
                                   % (type(self).__name__, batch.X.device))
        route = iter_route(self, batch, training)
        if trace and training:
            raise _lib.GnnHipError("trace=True is an inference call: wrap it in torch.no_grad()")
        if route.kind == "iter_events":
            if training:
                out = _IterFn.apply(self, batch, route.layout, *params)
            else:
                ip = self._iter_params([p.detach() for p in params])
                if trace:
                    e_all, H_all = _lib.iter_forward_events(batch, route.layout, ip, train=True)
                    out = (e_all[self.n_iters], e_all, H_all[:, :, :self.input_dim + self.hidden_dim].contiguous())
                else:
                    out = _lib.iter_forward_events(batch, route.layout, ip)
        else:
            out = self._per_module(batch, trace)
        e = out[0] if trace else out
        if batch.dense_shape:
            e = e.view(batch.dense_shape[0], batch.dense_shape[2])
        return (e, out[1], out[2]) if trace else e

    def _nets(self):
        """[(edge network, node network) per iteration], the network of the final edge pass."""
        raise NotImplementedError

    def _per_module(self, batch, trace):
        """Cell 14's forward, module by module on the per-module kernels (differentiable: every module has its HIP
        backward)."""
        lin = self.input_network[0]
        X = batch.X
        H = _InputFn.apply(X, lin.weight, lin.bias)
        pairs, last = self._nets()
        es, Hs = [], [H]
        for edge, node in pairs:
            e = edge(H, batch).reshape(-1)
            H = torch.cat([node(H, e, batch), X], dim=-1)
            if trace:
                es.append(e)
                Hs.append(H)
        e = last(H, batch).reshape(-1)
        return (e, torch.stack(es + [e]), torch.stack(Hs)) if trace else e


class SegmentClassifier(_IterClassifier):
    """Cell 14's `SegmentClassifier`: a network pair per iteration and an output network of its own."""

    def __init__(self, input_dim=2, hidden_dim=8, n_iters=3, hidden_activation=nn.Tanh):
        super(SegmentClassifier, self).__init__()
        self._common(input_dim, hidden_dim, n_iters, hidden_activation)
        self.edge_networks = nn.ModuleList(
            [EdgeNetwork(input_dim + hidden_dim, hidden_dim, hidden_activation) for i in range(n_iters)])
        self.node_networks = nn.ModuleList(
            [NodeNetwork(input_dim + hidden_dim, hidden_dim, hidden_activation) for i in range(n_iters)])
        self.output_network = EdgeNetwork(input_dim + hidden_dim, hidden_dim, hidden_activation)

    def _nets(self):
        return list(zip(self.edge_networks, self.node_networks)), self.output_network

    def _iter_params(self, params):
        T = self.n_iters
        edge = [params[2 + 4 * i:6 + 4 * i] for i in range(T)]
        node = [params[2 + 4 * T + 4 * i:6 + 4 * T + 4 * i] for i in range(T)]
        return _lib.iter_params_struct(params[0], params[1], edge, node, params[2 + 8 * T:6 + 8 * T], self.input_dim,
                                       self.hidden_dim)


class SegmentClassifier2(_IterClassifier):
    """Cell 14's `SegmentClassifier2`: one edge network (the final pass's too) and one node network for all
    iterations - `model.SegmentClassifier`'s arithmetic on the one-launch per-iteration kernels, every pass pointing
    at the same weight set; the opt-in one-launch route at hidden_dim 32."""

    def __init__(self, input_dim=2, hidden_dim=8, n_iters=3, hidden_activation=nn.Tanh):
        super(SegmentClassifier2, self).__init__()
        self._common(input_dim, hidden_dim, n_iters, hidden_activation)
        self.edge_network = EdgeNetwork(input_dim + hidden_dim, hidden_dim, hidden_activation)
        self.node_network = NodeNetwork(input_dim + hidden_dim, hidden_dim, hidden_activation)

    def _nets(self):
        return [(self.edge_network, self.node_network)] * self.n_iters, self.edge_network

    def _iter_params(self, params):
        T = self.n_iters
        return _lib.iter_params_struct(params[0], params[1], [params[2:6]] * T, [params[6:10]] * T, params[2:6],
                                       self.input_dim, self.hidden_dim, shared=True)


def build_toy_mpnn_graphs(hit_x, hit_y, det_r=synth.TOY_DET_R):
    """The inputs of gnn/MPNN_Seg_Toy2D.ipynb, cells 8, 11 and 12, on the device: hit_x floating-point [E, L * T]
    positions sorted within each layer (layer-major) and hit_y integer [E, L * T] track labels, as `sort_toy_tracks`
    (the notebook's generate_data) gives them.

    Returns ToyMpnnGraphs(batch, y): `batch` a HitGraphBatch of E graphs in event layout with X [E L T, 2] = (x, r)
    in float32 (cell 12), the T^2 (L - 1) segments of every event in cell 11's np.where(d == 1) order - segment
    (l T + a) T + b joins hit a of layer l to hit b of layer l + 1 - and the segment lists; y [E T^2 (L - 1)] float32
    = the two hits carry the same label (cell 12's ey), also `batch.y`.  Every event has one topology: the lists are
    built once from the shape and tiled.  Nothing is read back."""
    who = "build_toy_mpnn_graphs"
    det = _det_r(det_r)
    L = det.shape[0]
    x, lab, T = _hits(who, hit_x, hit_y, L, (torch.float32, torch.float64), check=False)
    dev, E = x.device, x.shape[0]
    N, S = L * T, T * T * (L - 1)
    src1, dst1 = synth.toy_mpnn_segments(L, T)
    # one event's lists: segments ending at / starting from each hit in ascending segment id (stable sorts)
    oin, oout = np.argsort(dst1, kind="stable"), np.argsort(src1, kind="stable")
    one = np.stack([src1, dst1, oin, src1[oin], oout, dst1[oout]]).astype(np.int64)
    cnt = np.stack([np.bincount(dst1, minlength=N), np.bincount(src1, minlength=N)]).astype(np.int64)
    ptr1 = np.concatenate([np.zeros((2, 1), np.int64), np.cumsum(cnt, axis=1)], axis=1)
    one_d, ptr_d = torch.from_numpy(one).to(dev), torch.from_numpy(ptr1).to(dev)
    ev = torch.arange(E, device=dev, dtype=torch.int64)[:, None]
    hit_off, seg_off = ev * N, ev * S

    def tiled(row, off):
        return (one_d[row][None, :] + off).reshape(-1).to(torch.int32)

    src, dst = tiled(0, hit_off), tiled(1, hit_off)
    in_eid, in_nbr, out_eid, out_nbr = tiled(2, seg_off), tiled(3, hit_off), tiled(4, seg_off), tiled(5, hit_off)
    tail = torch.full((1,), E * S, dtype=torch.int64, device=dev)
    in_ptr = torch.cat([(ptr_d[0][None, :N] + seg_off).reshape(-1), tail]).to(torch.int32)
    out_ptr = torch.cat([(ptr_d[1][None, :N] + seg_off).reshape(-1), tail]).to(torch.int32)
    r = torch.from_numpy(np.repeat(det, T)).to(dev)
    X = torch.stack([x.double(), r[None, :].expand(E, N)], dim=-1).to(torch.float32).reshape(E * N, 2)
    y = (lab[:, one_d[0]] == lab[:, one_d[1]]).to(torch.float32).reshape(-1)
    batch = HitGraphBatch._from_device_arrays(X, src, dst, y, np.arange(E + 1, dtype=np.int64) * N,
                                              np.arange(E + 1, dtype=np.int64) * S)
    batch.remember("device", "csr", (in_ptr, in_eid, in_nbr, out_ptr, out_eid, out_nbr))
    return ToyMpnnGraphs(batch, batch.y)
