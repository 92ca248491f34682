"""Fixtures for the toy MPNN notebook's classifiers (tests/golden/toy_mpnn/*.npz), made by RUNNING the reference: cell 14
of gnn/MPNN_Seg_Toy2D.ipynb (EdgeNetwork, NodeNetwork, SegmentClassifier, SegmentClassifier2) is read from the
notebook and executed as it is, on the CPU.  The toy cases run the notebook's own data cells too (cell 4's
generate_data, then cells 8, 11 and 12 with cell 7's values at 2-4 events and numpy's seed fixed); generate_data
indexes with lists `tracks[[...]]`, which the numpy of the notebook's time read as tuples: that substitution is made
in memory.  The muon-schema case takes ragged graphs from synth, zero-padded into one dense batch the way
gnn/trainSegmentClassifier.py's merge_graphs pads.  Nothing of the notebook is written into the repository.

Per case: X [B, N, F] (toy cases: also hit_y [B, N], cell 8's labels), the segments in index form (src, dst [B * E] in batch numbering, -1 = a padded column) and, for
the padded case only, the dense Ri / Ro; labels y [B, E]; the state_dict (param/<key>, fp32, torch's seeded init); the
reference's fp32 scores, its loss and every gradient after nn.BCELoss()(model(inputs), y).backward(); the same model
run as .double() on the same fp32 inputs - e64_<t> and H64_<t> of every pass through forward hooks (H = [H' | X]),
loss64, grad64/<key> -; and ref_err_* = the reference's own fp32 distance from that fp64 run, per tensor, relative to
the fp64 tensor's largest entry.  Files are written with fixed zip timestamps and torch runs on one thread: a rerun
reproduces them byte for byte.  A case whose file would pass 1 MiB keeps grad/* and grad64/* in <name>.grads.npz.

usage: python tools/gen_toy_mpnn_golden.py [--reference DIR]
"""
import argparse
import copy
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "toy_mpnn")
NOTEBOOK = "MPNN_Seg_Toy2D.ipynb"
LIMIT = 1 << 20          # bytes: no committed file may be larger than 1 MiB (tests/test_toy_mpnn_host.py checks the same)

from gen_gcn_golden import rel_err, write_npz  # noqa: E402
from gnn_fpga_amd import synth  # noqa: E402

# (name, class, F, D, T, input, batch, H64 passes kept (None: all))
CASES = [
    ("a_unshared_f2_d32_t10_b4", "SegmentClassifier", 2, 32, 10, "toy", 4, (0, 1, 5, 10)),
    ("b_unshared_f2_d8_t3_b3", "SegmentClassifier", 2, 8, 3, "toy", 3, None),
    ("c_unshared_f2_d16_t4_b2", "SegmentClassifier", 2, 16, 4, "toy", 2, None),
    ("d_unshared_f2_d8_t0_b2", "SegmentClassifier", 2, 8, 0, "toy", 2, None),
    ("e_unshared_f2_d8_t1_b2", "SegmentClassifier", 2, 8, 1, "toy", 2, None),
    ("f_unshared_f11_d8_t2_ragged", "SegmentClassifier", 11, 8, 2, "muon", 5, None),
    ("g_shared_f2_d32_t10_b4", "SegmentClassifier2", 2, 32, 10, "toy", 4, (0, 1, 5, 10)),
]


def _cells(ref_dir):
    nb = json.load(open(os.path.join(ref_dir, "gnn", NOTEBOOK)))
    return ["".join(c["source"]) if c["cell_type"] == "code" else "" for c in nb["cells"]]


def _run(src, cell, ns):
    text = "\n".join(ln for ln in src[cell].split("\n") if not ln.startswith("%"))       # (cell 11 starts with %%time)
    exec(compile(text, "%s cell %d" % (NOTEBOOK, cell), "exec"), ns)


def load_classes(ref_dir):
    import torch
    import torch.nn as nn
    ns = {"torch": torch, "nn": nn}
    _run(_cells(ref_dir), 14, ns)
    return ns


def toy_inputs(ref_dir, n_events, seed):
    """Cells 4, 8, 11, 12 at n_events events: X [B, 40, 2], Ri, Ro [B, 40, 144], ey [B, 144], float32, and cell 8's
    hit labels y [B, 40]."""
    src = list(_cells(ref_dir))
    for old in ("tracks[[idx0, idx1, idx2]]", "tracks[[idx0, idx, idx2]]"):
        assert old in src[4], "generate_data changed: %s not found" % old
        src[4] = src[4].replace(old, old.replace("[[", "[(").replace("]]", ")]"))
    ns = {"np": np, "print": lambda *a, **k: None}
    np.random.seed(seed)
    _run(src, 4, ns)
    # cell 7's values (its np.float is gone from numpy)
    ns.update(det_r=np.arange(10, dtype=np.float64), n_det_layers=10, n_events=n_events, n_tracks=4)
    for c in (8, 11, 12):
        _run(src, c, ns)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)      # noqa: E731  (cell 5's np_to_torch)
    return f32(ns["X"]), f32(ns["Ri"]), f32(ns["Ro"]), f32(ns["ey"]), ns["y"].astype(np.int64)


def muon_inputs(seed):
    """Ragged muon-schema graphs (F = 11) as one zero-padded dense batch: unequal sizes, a graph with a single
    segment, one with none, one with an isolated hit."""
    gs = [synth.muon_graph(seed), synth.muon_graph(seed + 1)]
    g = synth.muon_graph(seed + 2)
    gs.append(synth.HitGraph(g.X, g.src[:1], g.dst[:1], g.y[:1]))
    g = synth.muon_graph(seed + 3)
    gs.append(synth.HitGraph(g.X, g.src[:0], g.dst[:0], g.y[:0]))
    g = synth.muon_graph(seed + 4)
    lone = int(g.src[0])
    keep = (g.src != lone) & (g.dst != lone)
    gs.append(synth.HitGraph(g.X, g.src[keep], g.dst[keep], g.y[keep]))
    N, E = max(g.X.shape[0] for g in gs), max(g.src.shape[0] for g in gs)
    X, Ri, Ro, y = [], [], [], []
    for g in gs:
        x, ri, ro = synth.to_dense(g, N, E)
        X.append(x), Ri.append(ri), Ro.append(ro)
        y.append(np.concatenate([g.y, np.zeros(E - g.y.shape[0], np.float32)]))
    return np.stack(X), np.stack(Ri), np.stack(Ro), np.stack(y).astype(np.float32)


def index_form(Ri, Ro):
    """src, dst int32 [B * E] in batch numbering from the dense matrices; -1 where a column is empty."""
    B, N, E = Ri.shape
    off = (np.arange(B) * N)[:, None]
    src = np.where(Ro.sum(axis=1) > 0, Ro.argmax(axis=1) + off, -1)
    dst = np.where(Ri.sum(axis=1) > 0, Ri.argmax(axis=1) + off, -1)
    return src.reshape(-1).astype(np.int32), dst.reshape(-1).astype(np.int32)


def traced(model, inputs):
    """(scores, [e_t], [H_t = [H' | X]]) through forward hooks, in call order."""
    import torch
    X = inputs[0]
    es, hs, hooks = [], [], []
    edges = list(model.edge_networks) + [model.output_network] if hasattr(model, "edge_networks") else [model.edge_network]
    nodes = list(model.node_networks) if hasattr(model, "node_networks") else [model.node_network]
    for m in edges:
        hooks.append(m.register_forward_hook(lambda mod, i, o: es.append(o.detach().numpy().copy())))
    for m in [model.input_network] + nodes:
        hooks.append(m.register_forward_hook(
            lambda mod, i, o: hs.append(torch.cat([o.detach(), X], dim=-1).numpy().copy())))
    with torch.no_grad():
        out = model(inputs).numpy().copy()
    for h in hooks:
        h.remove()
    return out, es, hs


def run_case(ns, ref_dir, name, cls, F, D, T, kind, B, keep_h):
    import torch
    import torch.nn as nn
    seed = sum(map(ord, name))
    X, Ri, Ro, y, hit_y = toy_inputs(ref_dir, B, seed) if kind == "toy" else muon_inputs(seed) + (None,)
    assert X.shape[-1] == F
    torch.manual_seed(seed)
    model = ns[cls](input_dim=F, hidden_dim=D, n_iters=T)
    inputs = [torch.from_numpy(a) for a in (X, Ri, Ro)]
    yt = torch.from_numpy(y)
    sd = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    src, dst = index_form(Ri, Ro)
    out = {"X": X, "src": src, "dst": dst, "y": y, "cls": np.array(cls), "F": np.int64(F), "D": np.int64(D),
           "T": np.int64(T), "keys": np.array(list(sd))}
    if kind != "toy":
        out["Ri"], out["Ro"] = Ri, Ro
    else:
        out["hit_y"] = hit_y                      # cell 8's flattened labels: what cell 12's ey is made from
    for k, v in sd.items():
        out["param/" + k] = v
    scores, es, hs = traced(model, inputs)
    model.zero_grad()
    loss = nn.BCELoss()(model(inputs), yt)
    loss.backward()
    m64 = copy.deepcopy(model).double()
    in64 = [t.double() for t in inputs]
    scores64, es64, hs64 = traced(m64, in64)
    m64.zero_grad()
    loss64 = nn.BCELoss()(m64(in64), yt.double())
    loss64.backward()
    assert len(es64) == T + 1 and len(hs64) == T + 1 and np.array_equal(es64[-1], scores64)
    out["scores"], out["loss"], out["loss64"] = scores, np.float64(loss.item()), np.float64(loss64.item())
    out["ref_err_scores"] = rel_err(scores, scores64)
    out["ref_err_loss"] = rel_err(out["loss"], out["loss64"])
    for t in range(T + 1):
        out["e64_%d" % t] = es64[t]
        out["ref_err_e%d" % t] = rel_err(es[t], es64[t])
        if keep_h is None or t in keep_h:
            out["H64_%d" % t] = hs64[t]
            out["ref_err_H%d" % t] = rel_err(hs[t], hs64[t])
    for (n, p), (_, p64) in zip(model.named_parameters(), m64.named_parameters()):
        g, g64 = p.grad.detach().numpy().copy(), p64.grad.detach().numpy().copy()
        out["grad/" + n], out["grad64/" + n] = g, g64
        out["ref_err_grad/" + n] = rel_err(g, g64)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("GNN_REFERENCE", "../reference"))
    a = ap.parse_args()
    if not os.path.isdir(os.path.join(a.reference, "gnn")):
        sys.exit("reference checkout not found at %s" % a.reference)
    import torch
    torch.set_num_threads(1)                      # the same sums in the same order on every run
    ns = load_classes(a.reference)
    os.makedirs(OUT, exist_ok=True)
    for case in CASES:
        arr = run_case(ns, a.reference, *case)
        path = os.path.join(OUT, case[0] + ".npz")
        write_npz(path, arr)
        if os.path.getsize(path) > LIMIT:         # the notebook's configuration: the gradients go into a file of their own
            grads = {k: v for k, v in arr.items() if k.startswith(("grad/", "grad64/"))}
            write_npz(path, {k: v for k, v in arr.items() if k not in grads})
            write_npz(path[:-4] + ".grads.npz", grads)
            assert max(os.path.getsize(path), os.path.getsize(path[:-4] + ".grads.npz")) <= LIMIT
        worst = max(float(v) for k, v in arr.items() if k.startswith("ref_err_grad"))
        print("%s: %d bytes, %d tensors, loss %.6f, score span %.3f, worst ref_err_grad %.2e"
              % (path, os.path.getsize(path), len(arr["keys"]), float(arr["loss"]),
                 float(arr["scores"].max() - arr["scores"].min()), worst))


if __name__ == "__main__":
    main()
