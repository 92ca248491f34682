"""Fixtures for the hit classifier (tests/golden/node_classifier/*.npz), made by RUNNING the reference: the class
cells of gnn/MPNN_HitClassifier.ipynb (EdgeNetwork, NodeNetwork, NodeClassifier - cells 20-21) are read from the
notebook and executed as they are, and gnn/estimator.py's Estimator is imported unmodified.  Nothing of either is
written into the repository.

Per case (hidden_dim D, n_iters T, batch B): the inputs in index form (src, dst int32 of the dense batch's B x E
columns, -1 for padded ones; X; B, N, E), the state_dict (fp32, torch's seeded init), hit labels, the reference's
scores [B, N], per-iteration H' of the node network (forward hooks, small cases), and for training cases the loss
and the twelve gradients, captured inside Estimator.training_step after loss.backward() (a hook on
optimizer.step).  Files are written with fixed zip timestamps: a rerun reproduces them bit for bit.

usage: python tools/gen_nodeclf_golden.py [--reference DIR]
"""
import argparse
import io
import json
import os
import sys
import zipfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "tests", "golden", "node_classifier")

from gnn_fpga_amd import synth  # noqa: E402

# (name, hidden_dim, n_iters, batch, l1, padded, keep per-iteration H)
CASES = [
    ("d8_t0_b2", 8, 0, 2, 0.0, False, True),
    ("d8_t1_b4", 8, 1, 4, 0.0, False, True),
    ("d16_t3_b8", 16, 3, 8, 0.0, False, True),
    ("d64_t7_b32", 64, 7, 32, 0.0, False, False),
    ("d8_t2_b4_l1", 8, 2, 4, 1e-3, False, False),
    ("d8_t2_b6_padded", 8, 2, 6, 0.0, True, True),
]


def load_reference(ref_dir):
    """The notebook's class cells, executed in a namespace of their own, and the reference Estimator."""
    import torch
    import torch.nn as nn
    nb = json.load(open(os.path.join(ref_dir, "gnn", "MPNN_HitClassifier.ipynb")))
    ns = {"torch": torch, "nn": nn, "np": np}
    for cell in nb["cells"]:
        src = "".join(cell["source"])
        if cell["cell_type"] == "code" and src.lstrip().startswith("class "):
            exec(compile(src, "MPNN_HitClassifier.ipynb", "exec"), ns)
    sys.path.insert(0, os.path.join(ref_dir, "gnn"))
    import estimator                                   # gnn/estimator.py, unmodified
    return ns["NodeClassifier"], estimator.Estimator


def padded_samples(B, seed):
    """B graphs of 30-50 hits (3-5 candidates per layer) zero-padded to 50 hits / 225 segment columns."""
    rng = np.random.default_rng(seed)
    X = np.zeros((B, 50, 4), np.float32)
    Ri = np.zeros((B, 50, 225), np.uint8)
    Ro = np.zeros((B, 50, 225), np.uint8)
    y = np.zeros((B, 50), np.uint8)
    for b in range(B):
        k = int(rng.integers(3, 6))
        s = synth.hit_classifier_samples(1, seed=seed * 100 + b, n_layer_hits=k)
        n, e = s.X.shape[1], s.Ri.shape[2]
        X[b, :n], Ri[b, :n, :e], Ro[b, :n, :e], y[b, :n] = s.X[0], s.Ri[0], s.Ro[0], s.y[0]
    return X, Ri, Ro, y


def index_form(Ri, Ro):
    B, N, E = Ri.shape
    src = np.full((B, E), -1, np.int64)
    dst = np.full((B, E), -1, np.int64)
    for b in range(B):
        r, c = np.nonzero(Ro[b])
        src[b, c] = r + b * N
        r, c = np.nonzero(Ri[b])
        dst[b, c] = r + b * N
    return src.reshape(-1).astype(np.int32), dst.reshape(-1).astype(np.int32)


def run_case(NodeClassifier, Estimator, name, D, T, B, l1, padded, keep_h):
    import torch
    import torch.nn as nn
    seed = sum(map(ord, name))
    if padded:
        X, Ri, Ro, y = padded_samples(B, seed)
    else:
        s = synth.hit_classifier_samples(B, seed=seed)
        X, Ri, Ro, y = s.X, s.Ri, s.Ro, s.y
    torch.manual_seed(seed)
    model = NodeClassifier(input_dim=4, hidden_dim=D, n_iters=T)
    sd = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    inputs = [torch.from_numpy(X), torch.from_numpy(Ri.astype(np.float32)), torch.from_numpy(Ro.astype(np.float32))]
    hs = []
    hook = model.node_network.register_forward_hook(lambda m, i, o: hs.append(o.detach().numpy().copy()))
    with torch.no_grad():
        scores = model(inputs).numpy()
    hook.remove()
    src, dst = index_form(Ri, Ro)
    out = {"X": X.reshape(B * 50, 4), "src": src, "dst": dst, "B": np.int64(B), "N": np.int64(50),
           "E": np.int64(225), "n_iters": np.int64(T), "hidden_dim": np.int64(D), "l1": np.float64(l1),
           "y": y.astype(np.float32), "scores": scores, "keys": np.array(list(sd))}
    for k, v in sd.items():
        out["param/" + k] = v
    if keep_h:
        for t, h in enumerate(hs):
            out["H%d" % (t + 1)] = h
    # one reference training step, the gradients taken inside training_step (after loss.backward())
    est = Estimator(model, loss_func=nn.BCELoss(), l1=l1)
    cap = {}
    step = est.optimizer.step

    def grab(*a, **k):
        # (n_iters = 0: the edge and node networks take no part - autograd leaves their .grad None)
        cap["grads"] = {n: (p.grad.detach().numpy().copy() if p.grad is not None
                            else np.zeros(tuple(p.shape), np.float32)) for n, p in model.named_parameters()}
        return step(*a, **k)
    est.optimizer.step = grab
    loss = est.training_step(inputs, torch.from_numpy(y.astype(np.float32)))
    out["loss"] = np.float64(loss.item())
    for n, g in cap["grads"].items():
        out["grad/" + n] = g
    out["node_weight_shapes"] = np.array([list(l.weight.shape) for l in model.node_network.network
                                          if hasattr(l, "weight")])
    out["edge_weight_shapes"] = np.array([list(l.weight.shape) for l in model.edge_network.network
                                          if hasattr(l, "weight")])
    return out


def write_npz(path, arrays):
    """np.savez_compressed with a fixed zip timestamp (reproducible bytes)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("GNN_REFERENCE", "../reference"))
    a = ap.parse_args()
    if not os.path.isdir(os.path.join(a.reference, "gnn")):
        sys.exit("reference checkout not found at %s" % a.reference)
    import torch
    torch.set_num_threads(1)                      # the same sums in the same order on every run
    NodeClassifier, Estimator = load_reference(a.reference)
    os.makedirs(OUT, exist_ok=True)
    for case in CASES:
        arr = run_case(NodeClassifier, Estimator, *case)
        path = os.path.join(OUT, case[0] + ".npz")
        write_npz(path, arr)
        print("%s: %d bytes, loss %.6f" % (path, os.path.getsize(path), float(arr["loss"])))


if __name__ == "__main__":
    main()
