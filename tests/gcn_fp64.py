"""The dense formulation of the graph-convolution classifiers, restated with plain torch ops so that it runs in fp32 or
fp64 on any device: what the GPU tests compare the kernels with.  Not a test module.

    h = relu(x Wf^T + bf);  per layer hin = h (GCN) or [h | x] (GCRN)
    GraphConvSelfInt: z = hin Wn^T + bn + (A hin) Wg^T      GraphConv: z = (A hin) Wl^T + bl
    h = relu(z);  out = h Wc^T + bc
"""
import copy
import os

import numpy as np
import torch
import torch.nn as nn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gcn")
ULP16 = 16 * 2.0 ** -24           # the floor of every bound: 16 fp32 ulp, 9.6e-7


class DenseGCN(nn.Module):
    """kind: "gcn" or "gcrn"; conv: "selfint" or "graphconv".  Same sub-module names as the package's modules, so a
    state_dict of either loads into the other."""

    def __init__(self, input_dim, hidden_dims, kind="gcn", conv="selfint"):
        super().__init__()
        self.residual, self.conv = kind == "gcrn", conv
        extra = input_dim if self.residual else 0
        self.feature_extractor = nn.Linear(input_dim, hidden_dims[0])
        layers = []
        for i in range(len(hidden_dims) - 1):
            m = nn.Module()
            if conv == "selfint":
                m.node_mod = nn.Linear(hidden_dims[i] + extra, hidden_dims[i + 1])
                m.neighbor_mod = nn.Linear(hidden_dims[i] + extra, hidden_dims[i + 1], bias=False)
            else:
                m.linear = nn.Linear(hidden_dims[i] + extra, hidden_dims[i + 1])
            layers.append(m)
        self.gc_layers = nn.ModuleList(layers)
        self.classifier = nn.Linear(hidden_dims[-1], 1)

    def forward(self, x, a, keep=None):
        h = torch.relu(self.feature_extractor(x))
        if keep is not None:
            keep.append(h)
        for m in self.gc_layers:
            hin = torch.cat([h, x], dim=-1) if self.residual else h
            ah = torch.matmul(a, hin)
            z = m.node_mod(hin) + m.neighbor_mod(ah) if self.conv == "selfint" else m.linear(ah)
            h = torch.relu(z)
            if keep is not None:
                keep.append(h)
        return self.classifier(h).squeeze(-1)


def run(model, x, a, y=None, dtype=torch.float64, device="cpu"):
    """Logits, per-layer h and - with labels - the mean BCE-with-logits loss and every gradient, as numpy arrays
    computed in `dtype` from the given (fp32) state and inputs."""
    m = copy.deepcopy(model).to(device=device, dtype=dtype)
    m.zero_grad()
    xt = torch.as_tensor(x).to(device=device, dtype=dtype)
    at = torch.as_tensor(a).to(device=device, dtype=dtype)
    hs = []
    out = m(xt, at, keep=hs)
    res = {"logits": out.detach().cpu().numpy(), "h": [h.detach().cpu().numpy() for h in hs]}
    if y is not None:
        loss = nn.BCEWithLogitsLoss()(out, torch.as_tensor(y).to(device=device, dtype=dtype))
        loss.backward()
        res["loss"] = float(loss.item())
        res["grads"] = {n: p.grad.detach().cpu().numpy() for n, p in m.named_parameters()}
    return res


def rel_err(got, want):
    """max |got - want| relative to the largest entry of `want` (1 for an all-zero tensor)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = float(np.abs(want).max()) if want.size else 0.0
    if want.size == 0:
        return 0.0
    return float(np.abs(got - want).max()) / (scale if scale > 0 else 1.0)


def bound(ref_err):
    """4 x the reference's own fp32 distance from fp64 on the same data (the kernels sum in list order and torch's
    matmul in its own: two independent fp32 roundings of one value), with a floor of 16 fp32 ulp."""
    return max(4.0 * float(ref_err), ULP16)


def load_fixture(name):
    """A tests/golden/gcn fixture: dict of arrays, with A rebuilt dense from its coordinate form."""
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        d = {k: z[k] for k in z.files}
    A = np.zeros(tuple(int(v) for v in d["A_shape"]), np.float32)
    A[d["A_batch"], d["A_rows"], d["A_cols"]] = d["A_vals"]
    d["A"] = A
    d["hidden_dims"] = [int(v) for v in d["hidden_dims"]]
    d["kind"], d["conv"] = str(d["kind"]), str(d["conv"])
    return d


def fixture_names():
    return sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz")) if os.path.isdir(GOLDEN) else []


def fixture_model(d, cls=None, **kw):
    """The fixture's model: a DenseGCN, or `cls(input_dim, hidden_dims, **kw)` of the package, with its state loaded."""
    F = int(d["X"].shape[-1])
    m = DenseGCN(F, d["hidden_dims"], d["kind"], d["conv"]) if cls is None else cls(F, d["hidden_dims"], **kw)
    m.load_state_dict({k[len("param/"):]: torch.from_numpy(v.copy()) for k, v in d.items() if k.startswith("param/")})
    return m
