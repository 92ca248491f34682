"""fp64 restatement of the hit classifier (gnn/MPNN_HitClassifier.ipynb cells 20-21) in index form, on the CPU.

The notebook's model with dense incidence matrices, restated with segment lists: an edge pass scores segment j
from [H[src j] | H[dst j]], a node pass sums e_j H[src j] into the end hit (mi) and e_j H[dst j] into the start
hit (mo), and the output network scores every hit from [H'_T | X].  Padded segments (src = dst = -1) touch no hit.
torch float64 autograd gives the loss and the twelve gradients of one reference training step
(gnn/estimator.py training_step: BCE + l1 over the node and edge networks' weights).  The host tests pin this
restatement to the reference's own fixtures; the GPU tests compare the HIP kernels against it.
"""
import numpy as np
import torch

KEYS = ["input_network.0.weight", "input_network.0.bias",
        "edge_network.network.0.weight", "edge_network.network.0.bias",
        "edge_network.network.2.weight", "edge_network.network.2.bias",
        "node_network.network.0.weight", "node_network.network.0.bias",
        "node_network.network.2.weight", "node_network.network.2.bias",
        "output_network.0.weight", "output_network.0.bias"]


def _forward(X, src, dst, w, n_iters):
    """-> (hit scores [N], [H_0 .. H_T] each [N, C]); w: the twelve float64 tensors in KEYS order."""
    Win, bin_, W1, b1, W2, b2, W3, b3, W4, b4, Wo, bo = w
    N = X.shape[0]
    ok = src >= 0
    s, d = src[ok], dst[ok]
    H = torch.cat([torch.tanh(X @ Win.T + bin_), X], dim=1)
    Hs = [H]
    for _ in range(n_iters):
        a = torch.tanh(torch.cat([H[s], H[d]], dim=1) @ W1.T + b1)
        e = torch.sigmoid(a @ W2.T + b2)[:, 0]
        mi = torch.zeros_like(H).index_add(0, d, e[:, None] * H[s])
        mo = torch.zeros_like(H).index_add(0, s, e[:, None] * H[d])
        M = torch.cat([mi, mo, H], dim=1)
        H = torch.cat([torch.tanh(torch.tanh(M @ W3.T + b3) @ W4.T + b4), X], dim=1)
        Hs.append(H)
    return torch.sigmoid(H @ Wo.T + bo)[:, 0], Hs


def _tensors(params, requires_grad=False):
    return [torch.tensor(np.asarray(params[k], dtype=np.float64), requires_grad=requires_grad) for k in KEYS]


def forward(X, src, dst, params, n_iters):
    """(scores [N], H [(T+1), N, C]) in float64 numpy."""
    with torch.no_grad():
        y, Hs = _forward(torch.tensor(np.asarray(X, np.float64)), torch.as_tensor(np.asarray(src, np.int64)),
                         torch.as_tensor(np.asarray(dst, np.int64)), _tensors(params), n_iters)
    return y.numpy(), torch.stack(Hs).numpy()


def training_step(X, src, dst, params, n_iters, targets, l1=0.0):
    """(loss, {key: gradient}, scores) of one reference training step: nn.BCELoss (mean over every hit) plus
    l1 * sum |W| over the node and edge networks' two weight matrices each, as gnn/estimator.py forms it."""
    w = _tensors(params, requires_grad=True)
    y, _ = _forward(torch.tensor(np.asarray(X, np.float64)), torch.as_tensor(np.asarray(src, np.int64)),
                    torch.as_tensor(np.asarray(dst, np.int64)), w, n_iters)
    t = torch.tensor(np.asarray(targets, np.float64)).reshape(-1)
    loss = torch.nn.functional.binary_cross_entropy(y, t)
    if l1:
        loss = loss + l1 * sum(w[i].abs().sum() for i in (6, 8)) + l1 * sum(w[i].abs().sum() for i in (2, 4))
    loss.backward()
    grads = {k: (p.grad.numpy() if p.grad is not None else np.zeros(p.shape)) for k, p in zip(KEYS, w)}
    return float(loss.item()), grads, y.detach().numpy()


def upstream_step(X, src, dst, params, n_iters, grad_y, dtype=torch.float64):
    """{key: gradient} of sum(grad_y * y) over the twelve tensors, as float64 arrays: the backward under an arbitrary
    upstream gradient of the hit scores.  `dtype`: what the forward and autograd run in (float32: the fp32 oracle)."""
    w = [torch.tensor(np.asarray(params[k]), dtype=dtype, requires_grad=True) for k in KEYS]
    y, _ = _forward(torch.tensor(np.asarray(X), dtype=dtype), torch.as_tensor(np.asarray(src, np.int64)),
                    torch.as_tensor(np.asarray(dst, np.int64)), w, n_iters)
    (y * torch.tensor(np.asarray(grad_y), dtype=dtype).reshape(-1)).sum().backward()
    return {k: (p.grad.double().numpy() if p.grad is not None else np.zeros(p.shape)) for k, p in zip(KEYS, w)}


def fixture(path):
    """A tests/golden/node_classifier/*.npz as a dict (params / grads as {key: array})."""
    z = np.load(path)
    out = {k: z[k] for k in z.files if "/" not in k}
    out["params"] = {k: z["param/" + k] for k in KEYS}
    out["grads"] = {k: z["grad/" + k] for k in KEYS}
    return out


def segclf_forward(X, src, dst, params, n_iters):
    """SegmentClassifier on the same trunk (the first ten KEYS): final edge pass scores [E] in float64 (padded
    segments score sigmoid(W2 tanh(b1) + b2), as in the reference's dense form)."""
    w = _tensors(dict(params, **{k: np.zeros((1, 1)) for k in KEYS[10:]}))
    y, e = _segclf(torch.tensor(np.asarray(X, np.float64)), torch.as_tensor(np.asarray(src, np.int64)),
                   torch.as_tensor(np.asarray(dst, np.int64)), w, n_iters)
    return e.detach().numpy()


def segclf_training_step(X, src, dst, params, n_iters, targets):
    """(loss, {key: gradient} of the ten trunk tensors) of nn.BCELoss on the segment scores."""
    full = dict(params, **{k: np.zeros((1, 1)) for k in KEYS[10:]})
    w = _tensors(full, requires_grad=True)
    _, e = _segclf(torch.tensor(np.asarray(X, np.float64)), torch.as_tensor(np.asarray(src, np.int64)),
                   torch.as_tensor(np.asarray(dst, np.int64)), w, n_iters)
    loss = torch.nn.functional.binary_cross_entropy(e, torch.tensor(np.asarray(targets, np.float64)).reshape(-1))
    loss.backward()
    return float(loss.item()), {k: p.grad.numpy() for k, p in zip(KEYS[:10], w[:10])}


def _segclf(X, src, dst, w, n_iters):
    Win, bin_, W1, b1, W2, b2, W3, b3, W4, b4 = w[:10]
    _, Hs = _forward(X, src, dst, list(w[:10]) + [torch.zeros(1, X.shape[1] + b1.shape[0], dtype=torch.float64),
                                                  torch.zeros(1, dtype=torch.float64)], n_iters)
    H = Hs[-1]
    ok = (src >= 0)[:, None]
    z = torch.where(ok, torch.cat([H[src.clamp(min=0)], H[dst.clamp(min=0)]], dim=1) @ W1.T + b1, b1.expand(src.shape[0], -1))
    return None, torch.sigmoid(torch.tanh(z) @ W2.T + b2)[:, 0]
