"""Fixtures for the graph-convolution classifiers (tests/golden/gcn/*.npz), made by RUNNING the reference: the class
cells of gnn/GCN_Seg_Toy2D.ipynb (cells 20-22: repeat_module, GraphConv, GraphConvSelfInt, GCNBinaryClassifier,
training_step) and gnn/GCN_Toy2D.ipynb (cells 10, 11, 13-15: the same plus GCRNBinaryClassifier) are read from the
notebooks and executed as they are.  For the segment cases the notebook's own data cells are executed too (cells 3,
4, 7-17 and 24, cell 12's triple loop included, with n_events set to 2-4 and numpy's seed fixed); the hit cases take
synth.toy_hit_graphs, because the hit notebook's data cells need a numpy of their time.  Nothing of either notebook
is written into the repository.

Per case: X, the adjacency in coordinate form (A_batch, A_rows, A_cols, A_vals, A_shape), labels y, the state_dict
(param/<key>, fp32, torch's seeded init), the reference's fp32 logits, the loss and every gradient captured inside
the notebook's training_step after backward() (a hook on optimizer.step), the same model run as .double() on the
same fp32 inputs (logits64, loss64, grad64/<key>, and h64_<l>, the post-ReLU h of every layer, on the small cases),
and ref_err_* = the reference's own fp32 distance from that fp64 run, per tensor, relative to the fp64 tensor's
largest entry.

A fixture must not hide errors behind dead units: the model's seed is the first of 0..31 for which every
graph-convolution layer has between 20 % and 90 % positive ReLU outputs and the logits span at least 0.05; the tool
fails if there is none.  Files are written with fixed zip timestamps and torch runs on one thread: a rerun
reproduces them byte for byte.

usage: python tools/gen_gcn_golden.py [--reference DIR]
"""
import argparse
import copy
import io
import json
import os
import sys
import zipfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "tests", "golden", "gcn")

from gnn_fpga_amd import synth  # noqa: E402

# (name, inputs, batch, kind, conv, hidden_dims, keep per-layer h)
CASES = [
    ("seg_gcn_selfint_16x5_b4", "seg", 4, "gcn", "selfint", [16] * 5, False),
    ("seg_gcn_graphconv_16x5_b2", "seg", 2, "gcn", "graphconv", [16] * 5, True),
    ("seg_gcn_selfint_32_64_32_b2", "seg", 2, "gcn", "selfint", [32, 64, 32], False),
    ("hits_gcrn_selfint_8x12_b8", "row", 8, "gcrn", "selfint", [8] * 12, True),
    ("hits_gcrn_graphconv_8_12_16_b3", "row", 3, "gcrn", "graphconv", [8, 12, 16], True),
    ("hits_gcrn_selfint_32_64x5_32_b2", "row", 2, "gcrn", "selfint", [32, 64, 64, 64, 64, 64, 32], False),
    ("hits_kw_gcn_graphconv_8x3_b3", "kw", 3, "gcn", "graphconv", [8] * 3, True),
    ("hits_gcn_selfint_8_8_b1", "row", 1, "gcn", "selfint", [8, 8], True),
    ("hits_gcn_8_b2", "row", 2, "gcn", "selfint", [8], True),
]


class _NoPlot:
    """Stands in for matplotlib.pyplot in the data cells that draw a histogram."""

    def __getattr__(self, name):
        return lambda *a, **k: None


def _cells(ref_dir, notebook):
    nb = json.load(open(os.path.join(ref_dir, "gnn", notebook)))
    return ["".join(c["source"]) if c["cell_type"] == "code" else "" for c in nb["cells"]]


def load_reference(ref_dir):
    """The notebooks' class cells, each notebook in a namespace of its own."""
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    out = {}
    for key, notebook, cells in (("seg", "GCN_Seg_Toy2D.ipynb", (20, 21, 22)),
                                 ("hits", "GCN_Toy2D.ipynb", (10, 11, 13, 14, 15))):
        src = _cells(ref_dir, notebook)
        ns = {"torch": torch, "nn": nn, "F": F, "np": np}
        for c in cells:
            exec(compile(src[c], "%s cell %d" % (notebook, c), "exec"), ns)
        out[key] = ns
    return out


def segment_inputs(ref_dir, n_events, seed):
    """The segment notebook's own data cells at n_events events: seg_X, seg_A, seg_y."""
    src = _cells(ref_dir, "GCN_Seg_Toy2D.ipynb")
    ns = {"np": np, "plt": _NoPlot(), "print": lambda *a, **k: None}
    np.random.seed(seed)
    for c in (3, 4, 7):
        exec(compile(src[c], "GCN_Seg_Toy2D.ipynb cell %d" % c, "exec"), ns)
    ns["n_events"] = n_events
    for c in (8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 24):
        exec(compile(src[c], "GCN_Seg_Toy2D.ipynb cell %d" % c, "exec"), ns)
    return ns["seg_X"].astype(np.float32), ns["seg_A"].astype(np.float32), ns["seg_y"].astype(np.float32)


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = float(np.abs(want).max())
    return np.float64(float(np.abs(got - want).max()) / (scale if scale > 0 else 1.0))


def forward_layers(model, x, a):
    """(logits, [post-ReLU h of the feature extractor and of every graph-convolution layer]) through forward hooks."""
    import torch
    hs, hooks = [], []
    B, N = x.shape[0], x.shape[1]
    for m in [model.feature_extractor] + list(model.gc_layers):
        hooks.append(m.register_forward_hook(
            lambda mod, i, o: hs.append(torch.relu(o.detach()).reshape(B, N, -1).numpy().copy())))
    with torch.no_grad():
        out = model(x, a).numpy().copy()
    for h in hooks:
        h.remove()
    return out, hs


def run_case(ref, ref_dir, name, inputs, B, kind, conv, dims, keep_h):
    import torch
    import torch.nn as nn
    data_seed = sum(map(ord, name))
    if inputs == "seg":
        X, A, y = segment_inputs(ref_dir, B, data_seed)
        ns = ref["seg"]
    else:
        X, A, y = synth.toy_hit_graphs(B, seed=data_seed, norm=inputs)
        ns = ref["hits"]
    cls = ns["GCRNBinaryClassifier"] if kind == "gcrn" else ns["GCNBinaryClassifier"]
    gc_type = ns["GraphConvSelfInt"] if conv == "selfint" else ns["GraphConv"]
    x, a, yt = torch.from_numpy(X), torch.from_numpy(A), torch.from_numpy(y)
    for seed in range(32):
        torch.manual_seed(seed)
        model = cls(X.shape[-1], dims, gc_type=gc_type)
        logits, hs = forward_layers(model, x, a)
        alive = all(0.2 <= float((h > 0).mean()) <= 0.9 for h in hs[1:])
        if alive and float(logits.max() - logits.min()) >= 0.05:
            break
    else:
        sys.exit("%s: no seed in 0..31 gives live units and a logit span of 0.05" % name)
    sd = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    bi, ri, ci = np.nonzero(A)
    out = {"X": X, "y": y, "A_batch": bi.astype(np.int32), "A_rows": ri.astype(np.int32),
           "A_cols": ci.astype(np.int32), "A_vals": A[bi, ri, ci], "A_shape": np.array(A.shape, np.int64),
           "kind": np.array(kind), "conv": np.array(conv), "hidden_dims": np.array(dims, np.int64),
           "seed": np.int64(seed), "keys": np.array(list(sd)), "logits": logits}
    for k, v in sd.items():
        out["param/" + k] = v
    # the same model in fp64 on the same fp32 inputs
    m64 = copy.deepcopy(model).double()
    logits64, hs64 = forward_layers(m64, x.double(), a.double())
    m64.zero_grad()
    loss64 = nn.BCEWithLogitsLoss()(m64(x.double(), a.double()), yt.double())
    loss64.backward()
    g64 = {n: p.grad.detach().numpy().copy() for n, p in m64.named_parameters()}
    # one reference training step, the gradients taken inside training_step (after loss.backward())
    optimizer = torch.optim.Adam(model.parameters())
    cap, step = {}, optimizer.step

    def grab(*args, **kw):
        cap["grads"] = {n: p.grad.detach().numpy().copy() for n, p in model.named_parameters()}
        return step(*args, **kw)
    optimizer.step = grab
    loss = ns["training_step"](model, [x, a], yt, nn.BCEWithLogitsLoss(), optimizer)
    out["loss"] = np.float64(loss.item())
    out["logits64"], out["loss64"] = logits64, np.float64(loss64.item())
    out["ref_err_logits"] = rel_err(logits, logits64)
    out["ref_err_loss"] = rel_err(out["loss"], out["loss64"])
    for n, g in cap["grads"].items():
        out["grad/" + n], out["grad64/" + n] = g, g64[n]
        out["ref_err_grad/" + n] = rel_err(g, g64[n])
    if keep_h:
        for l, (h, h64) in enumerate(zip(hs, hs64)):
            out["h64_%d" % l] = h64
            out["ref_err_h%d" % l] = rel_err(h, h64)
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
    ref = load_reference(a.reference)
    os.makedirs(OUT, exist_ok=True)
    for case in CASES:
        arr = run_case(ref, a.reference, *case)
        path = os.path.join(OUT, case[0] + ".npz")
        write_npz(path, arr)
        worst = max(float(v) for k, v in arr.items() if k.startswith("ref_err_"))
        print("%s: %d bytes, seed %d, loss %.6f, logit span %.3f, worst ref_err %.2e"
              % (path, os.path.getsize(path), int(arr["seed"]), float(arr["loss"]),
                 float(arr["logits"].max() - arr["logits"].min()), worst))


if __name__ == "__main__":
    main()
