"""ORACLE (test infrastructure): index-form restatement of the reference forward in torch, with autograd.

The mathematics of `oracle/index_numpy.py` (reference gnn/model.py:140-156 with the dense one-hot `bmm`s replaced
by what they compute), written with `index_select` / `index_add` so that torch autograd differentiates it:

    bmm(Ro^T, H)[j] = H[src[j]]      bmm(Ri^T, H)[j] = H[dst[j]]        model.py:71-72,114-115
    mi[n] = sum_{j: dst[j]=n} e_j * H[src[j]]                           model.py:117-118
    mo[n] = sum_{j: src[j]=n} e_j * H[dst[j]]                           model.py:116,119
    padded segment (src = dst = -1): gathered rows are 0, contributes nothing to mi / mo,
                                     still scored (sigmoid(W2 tanh(b1) + b2))

Unlike the dense form it costs O(E) per pass, so the backward of detector-size graphs (10^5 - 10^6 segments) runs
on the CPU in seconds: the fp64 "truth" for the training kernels.  Everything runs in the dtype of `params`
(float64 for a reference); gradients come from `loss.backward()` on parameters that require them.
Thread count: torch's own (OMP_NUM_THREADS where it is set).
"""
import torch

from .dense_torch import KEYS  # noqa: F401  (the ten state_dict names `params` is keyed by)


def _w(params, masks, key):
    w = params[key]
    if masks is not None and key in masks:
        w = w * masks[key].to(w.dtype)                   # model.py:30
    return w


class _Index:
    """src / dst as int64 gather indices (padded -> row 0, multiplied by 0) and the valid subset for the sums."""

    def __init__(self, src, dst, dtype):
        src = torch.as_tensor(src).long()
        dst = torch.as_tensor(dst).long()
        valid = src >= 0
        self.E = src.shape[0]
        self.all_valid = bool(valid.all())
        self.gsrc = src.clamp(min=0)
        self.gdst = dst.clamp(min=0)
        self.keep = valid.to(dtype)[:, None]
        self.vsrc = src[valid]
        self.vdst = dst[valid]
        self.valid = valid

    def gather(self, H, idx):
        if H.shape[0] == 0:
            return H.new_zeros((self.E, H.shape[1]))
        g = H.index_select(0, idx)
        return g if self.all_valid else g * self.keep


def _edge(H, ix, params, masks):
    W1 = _w(params, masks, "edge_network.network.0.weight")
    W2 = _w(params, masks, "edge_network.network.2.weight")
    B = torch.cat([ix.gather(H, ix.gsrc), ix.gather(H, ix.gdst)], dim=1)     # out first, then in (model.py:73)
    a = torch.tanh(B @ W1.t() + params["edge_network.network.0.bias"])
    return torch.sigmoid(a @ W2.t() + params["edge_network.network.2.bias"])[:, 0]


def _node(H, e, ix, params, masks):
    W3 = _w(params, masks, "node_network.network.0.weight")
    W4 = _w(params, masks, "node_network.network.2.weight")
    w = e if ix.all_valid else e[ix.valid]
    w = w[:, None]
    mi = H.new_zeros(H.shape).index_add(0, ix.vdst, w * H.index_select(0, ix.vsrc))
    mo = H.new_zeros(H.shape).index_add(0, ix.vsrc, w * H.index_select(0, ix.vdst))
    M = torch.cat([mi, mo, H], dim=1)                                         # model.py:120
    q = torch.tanh(M @ W3.t() + params["node_network.network.0.bias"])
    return torch.tanh(q @ W4.t() + params["node_network.network.2.bias"])


def edge_network(H, src, dst, params, masks=None):
    """EdgeNetwork.forward (model.py:69-81): H [N, C] -> e [E]; padded segments are scored on zero rows."""
    return _edge(H, _Index(src, dst, H.dtype), params, masks)


def node_network(H, e, src, dst, params, masks=None):
    """NodeNetwork.forward (model.py:113-125): H [N, C], e [E] -> H' [N, D] (without the skip concat)."""
    return _node(H, e, _Index(src, dst, H.dtype), params, masks)


def segment_classifier(X, src, dst, params, n_iters, masks=None, trace=None):
    """Edge scores [E] in the dtype of `params`; if `trace` is a dict it receives lists 'e' and 'H'."""
    Win = _w(params, masks, "input_network.0.weight")
    X = torch.as_tensor(X).to(Win.dtype)
    ix = _Index(src, dst, Win.dtype)
    H = torch.cat([torch.tanh(X @ Win.t() + params["input_network.0.bias"]), X], dim=1)   # model.py:144-146
    if trace is not None:
        trace["e"], trace["H"] = [], [H]
    for _ in range(n_iters):                                                  # model.py:148
        e = _edge(H, ix, params, masks)
        H = torch.cat([_node(H, e, ix, params, masks), X], dim=1)             # model.py:152-154
        if trace is not None:
            trace["e"].append(e)
            trace["H"].append(H)
    e = _edge(H, ix, params, masks)                                           # model.py:156
    if trace is not None:
        trace["e"].append(e)
    return e
