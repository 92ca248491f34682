"""fp64 restatement of gnn/MPNN_Seg_Toy2D.ipynb cell 14 in index form, with autograd (test infrastructure, not product;
imported by test_toy_mpnn_host.py and test_gpu_toy_mpnn.py), and the loader of tests/golden/toy_mpnn.

`forward(params, X, src, dst, T)` takes a state_dict-like mapping in the notebook's keys - `edge_networks.<i>...` /
`node_networks.<i>...` / `output_network...` (SegmentClassifier) or `edge_network...` / `node_network...`
(SegmentClassifier2) - and returns every pass's scores and hit rows.  A padded segment (src = dst = -1) gathers zero
rows, as an all-zero column of Ri / Ro does, and adds nothing to any hit.  `faults` injects the wiring mistakes the
fixtures are built to see (test_toy_mpnn_host.py).
"""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "toy_mpnn")
CASES = ("a_unshared_f2_d32_t10_b4", "b_unshared_f2_d8_t3_b3", "c_unshared_f2_d16_t4_b2", "d_unshared_f2_d8_t0_b2",
         "e_unshared_f2_d8_t1_b2", "f_unshared_f11_d8_t2_ragged", "g_shared_f2_d32_t10_b4")


class Fixture:
    """One case: arrays by name (`fx["X"]`), `params` / `grad64` / `ref_err_grad` by state_dict key."""

    def __init__(self, name):
        self.name = name
        self.a = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
        extra = os.path.join(GOLDEN, name + ".grads.npz")
        if os.path.exists(extra):
            self.a.update(np.load(extra))
        self.keys = [str(k) for k in self.a["keys"]]
        self.F, self.D, self.T = int(self.a["F"]), int(self.a["D"]), int(self.a["T"])
        self.shared = str(self.a["cls"]) == "SegmentClassifier2"
        self.params = {k: self.a["param/" + k] for k in self.keys}
        self.grad64 = {k: self.a["grad64/" + k] for k in self.keys}
        self.ref_err_grad = {k: float(self.a["ref_err_grad/" + k]) for k in self.keys}
        self.B, self.N = self.a["X"].shape[:2]
        self.E = self.a["y"].shape[1]

    def __getitem__(self, k):
        return self.a[k]

    def __contains__(self, k):
        return k in self.a

    def h_passes(self):
        return [t for t in range(self.T + 1) if "H64_%d" % t in self.a]


def _edge(p, pre, H, src, dst):
    ok = (src >= 0).to(H.dtype)[:, None]
    bo, bi = H[src.clamp(min=0)] * ok, H[dst.clamp(min=0)] * ok
    z = torch.tanh(torch.cat([bo, bi], dim=1) @ p[pre + ".network.0.weight"].T + p[pre + ".network.0.bias"])
    return torch.sigmoid(z @ p[pre + ".network.2.weight"].T + p[pre + ".network.2.bias"]).squeeze(-1)


def _node(p, pre, H, e, src, dst):
    ok = src >= 0
    s, d, w = src[ok], dst[ok], e[ok][:, None]
    mi = torch.zeros_like(H).index_add(0, d, w * H[s])
    mo = torch.zeros_like(H).index_add(0, s, w * H[d])
    q = torch.tanh(torch.cat([mi, mo, H], dim=1) @ p[pre + ".network.0.weight"].T + p[pre + ".network.0.bias"])
    return torch.tanh(q @ p[pre + ".network.2.weight"].T + p[pre + ".network.2.bias"])


def names(p, T, faults=()):
    """(edge network of pass t for t in 0..T, node network of pass t for t in 0..T-1) as key prefixes.
    faults: ("swap", t) - passes t and t+1 exchange their edge AND node sets; ("out_for_last",) - output_network
    scores in place of edge_networks[T-1]."""
    if "edge_network.network.0.weight" in p:
        return ["edge_network"] * (T + 1), ["node_network"] * T
    edge = ["edge_networks.%d" % t for t in range(T)] + ["output_network"]
    node = ["node_networks.%d" % t for t in range(T)]
    for f in faults:
        if f[0] == "swap":
            t = f[1]
            edge[t], edge[t + 1] = edge[t + 1], edge[t]
            if t + 1 < T:
                node[t], node[t + 1] = node[t + 1], node[t]
        elif f[0] == "out_for_last":
            edge[T - 1] = "output_network"
    return edge, node


def forward(p, X, src, dst, T, faults=()):
    """p: {key: fp64 tensor}; X [N, F] fp64; src, dst int64 [E] (-1 = padded).  -> ([e_0 .. e_T], [H_0 .. H_T]);
    e_T are the model's scores, H_t = [H' | X]."""
    edge, node = names(p, T, faults)
    H = torch.cat([torch.tanh(X @ p["input_network.0.weight"].T + p["input_network.0.bias"]), X], dim=1)
    es, Hs = [], [H]
    for t in range(T):
        e = _edge(p, edge[t], H, src, dst)
        H = torch.cat([_node(p, node[t], H, e, src, dst), X], dim=1)
        es.append(e)
        Hs.append(H)
    es.append(_edge(p, edge[T], H, src, dst))
    return es, Hs


def run(params, X, src, dst, y, T, faults=(), dtype=torch.float64):
    """numpy in, numpy out: dict(e=[...], H=[...], loss, grads {key: array}) with nn.BCELoss's mean over all segments
    (padded ones included, like the reference's mean over B x E_max).  dtype=torch.float32: the same statements in
    fp32 on the CPU, whose distance from the fp64 run stands in for a fixture's ref_err_* on synthetic inputs."""
    p = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in params.items()}
    Xt = torch.tensor(np.asarray(X), dtype=dtype).reshape(-1, np.asarray(X).shape[-1])
    s, d = (torch.tensor(np.asarray(a).reshape(-1), dtype=torch.int64) for a in (src, dst))
    es, Hs = forward(p, Xt, s, d, T, faults)
    out = dict(e=[e.detach().numpy() for e in es], H=[h.detach().numpy() for h in Hs])
    if y is not None:
        loss = torch.nn.BCELoss()(es[-1], torch.tensor(np.asarray(y).reshape(-1), dtype=dtype))
        loss.backward()
        out["loss"] = float(loss.item())
        out["grads"] = {k: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape)) for k, v in p.items()}
    return out


def rel_err(got, want):
    """Largest error relative to the fp64 tensor's largest entry."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = float(np.abs(want).max()) if want.size else 0.0
    return float(np.abs(got - want).max()) / (scale if scale > 0 else 1.0) if want.size else 0.0


SCORE_BOUND = 1e-5          # absolute, scores and hit rows: the project's score bound


def grad_bound(ref_err):
    """4 x the reference's own fp32 error (two independent fp32 roundings of one value), at least the project's 5e-6."""
    return max(4.0 * float(ref_err), 5e-6)
