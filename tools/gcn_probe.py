"""The graph-convolution classifiers (gnn/GCN_Seg_Toy2D.ipynb, gnn/GCN_Toy2D.ipynb) on one GPU.

  1. accuracy: the distance from fp64 the fused kernels reach on every fixture of tests/golden/gcn (logits, loss,
     worst gradient), relative to each tensor's largest entry, beside the reference's own fp32 distance;
  2. timings, HIP-event medians after warm-up, at the two notebook configurations with batches of 32 - segment graphs
     (225 segments, F = 5, GCNBinaryClassifier [16]*5) and hit graphs (40 hits, F = 3, GCRNBinaryClassifier [8]*12):
     forward and training step (forward + BCEWithLogitsLoss + backward + Adam) with a compressed adjacency sliced per
     step (adj[j:j+32], a view) and with dense input (compressed on every call), one evaluation call over the
     notebooks' test sets (3 277 / 6 554 graphs), and the compression of the full training adjacency (29 491 / 58 982
     graphs) - each for the fused path and for the same model restated with plain torch ops (tests/gcn_fp64.py:
     torch.matmul(a, x) per layer, as the notebooks do) on the same GPU; seconds per epoch for both.

The graphs are synth.toy_segment_graphs / toy_hit_graphs; the data sets beyond 1 024 / 8 192 events repeat those
events on the device (the sparsity pattern, which is all the timings depend on, is that of the notebooks' data).

`--trace-only` runs ten training steps per configuration for a `rocprofv3 --kernel-trace --stats` run.
profiles/gcn_probe.txt is `python tools/gcn_probe.py > profiles/gcn_probe.txt`.

usage: python tools/gcn_probe.py [--steps N] [--trace-only]
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import gcn_fp64 as ref  # noqa: E402
from gnn_fpga_amd import synth  # noqa: E402
from gnn_fpga_amd.gcn import (GCNBinaryClassifier, GCRNBinaryClassifier, GraphConv, GraphConvSelfInt,  # noqa: E402
                              compress_adjacency)

DEV = torch.device("cuda:0")
# (name, kind, hidden_dims, events generated, training graphs, test graphs, the notebook's recorded s/epoch)
CONFIGS = [("segment graphs: 225 segments, F = 5, GCNBinaryClassifier [16]*5", "gcn", [16] * 5, 1024, 29491, 3277,
            "21.6-23.3 s (GCN_Seg_Toy2D.ipynb cell 28)"),
           ("hit graphs: 40 hits, F = 3, GCRNBinaryClassifier [8]*12", "gcrn", [8] * 12, 8192, 58982, 6554,
            "about 32 s (GCN_Toy2D.ipynb cell 22)")]


def timed(fn, steps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def train_step(model, opt, x, a, y):
    loss_func = nn.BCEWithLogitsLoss()

    def step():
        model.train()
        model.zero_grad()
        loss = loss_func(model(x, a), y)
        loss.backward()
        opt.step()
    return step


def accuracy(out):
    print("== distance from fp64, relative to each tensor's largest entry: fused kernels | the reference's own fp32",
          file=out)
    for case in ref.fixture_names():
        d = ref.load_fixture(case)
        cls = GCRNBinaryClassifier if d["kind"] == "gcrn" else GCNBinaryClassifier
        m = ref.fixture_model(d, cls, gc_type=GraphConvSelfInt if d["conv"] == "selfint" else GraphConv).to(DEV)
        x, y = torch.from_numpy(d["X"]).to(DEV), torch.from_numpy(d["y"]).to(DEV)
        adj = compress_adjacency(torch.from_numpy(d["A"]).to(DEV))
        m.train()
        logits = m(x, adj)
        loss = nn.BCEWithLogitsLoss()(logits, y)
        loss.backward()
        e_log = ref.rel_err(logits.detach().cpu().numpy(), d["logits64"])
        e_loss = ref.rel_err(loss.item(), d["loss64"])
        worst = max(((ref.rel_err(p.grad.cpu().numpy(), d["grad64/" + n]), float(d["ref_err_grad/" + n]), n)
                     for n, p in m.named_parameters()), key=lambda t: t[0] / ref.bound(t[1]))
        print("  %-34s logits %.2e | %.2e   loss %.2e | %.2e   worst gradient %.2e | %.2e (%s)"
              % (case, e_log, float(d["ref_err_logits"]), e_loss, float(d["ref_err_loss"]), worst[0], worst[1],
                 worst[2]), file=out)


def data(kind, n_events):
    if kind == "gcn":
        parts = [synth.toy_segment_graphs(256, seed=s) for s in range(n_events // 256)]
    else:
        parts = [synth.toy_hit_graphs(n_events, seed=0, norm="row")]
    return [torch.from_numpy(np.concatenate([p[i] for p in parts])).to(DEV) for i in range(3)]


def tiled(t, n):
    reps = (n + t.shape[0] - 1) // t.shape[0]
    return t.repeat(reps, *([1] * (t.dim() - 1)))[:n].contiguous()


def config(cfg, steps, out):
    name, kind, dims, n_gen, n_train, n_test, recorded = cfg
    X, A, Y = data(kind, n_gen)
    F = X.shape[-1]
    torch.manual_seed(0)
    cls = GCRNBinaryClassifier if kind == "gcrn" else GCNBinaryClassifier
    m = cls(F, dims).to(DEV)
    dense = ref.DenseGCN(F, dims, kind, "selfint").to(DEV)
    dense.load_state_dict(m.state_dict())
    x, a, y = X[:32].contiguous(), A[:32].contiguous(), Y[:32].contiguous()
    adj_all = compress_adjacency(A)
    n_batches = (n_train + 31) // 32
    print("== %s, batch 32; list width %d" % (name, adj_all.width), file=out)
    rows = {}
    with torch.no_grad():
        m.eval(), dense.eval()
        rows["fwd"] = timed(lambda: m(x, adj_all[32:64]), steps)
        rows["fwd_dense_in"] = timed(lambda: m(x, a), steps)
        rows["fwd_torch"] = timed(lambda: dense(x, a), steps)
    rows["step"] = timed(train_step(m, torch.optim.Adam(m.parameters()), x, adj_all[32:64], y), steps)
    rows["step_dense_in"] = timed(train_step(m, torch.optim.Adam(m.parameters()), x, a, y), steps)
    rows["step_torch"] = timed(train_step(dense, torch.optim.Adam(dense.parameters()), x, a, y), steps)
    rows["compress32"] = timed(lambda: compress_adjacency(a), steps)
    xt, at = tiled(X, n_test), tiled(A, n_test)
    adj_t = compress_adjacency(at)
    with torch.no_grad():
        m.eval(), dense.eval()
        rows["eval"] = timed(lambda: m(xt, adj_t), max(5, steps // 5), warmup=2)
        rows["eval_dense_in"] = timed(lambda: m(xt, at), max(5, steps // 5), warmup=2)
        rows["eval_torch"] = timed(lambda: dense(xt, at), max(5, steps // 5), warmup=2)
    del xt, at, adj_t
    big = tiled(A, n_train)
    rows["compress_train"] = timed(lambda: compress_adjacency(big), 5, warmup=1)
    gb = big.numel() * 4 / 1e9
    del big
    p = lambda k, label, extra="": print("  %-66s %9.3f ms%s" % (label, rows[k], extra), file=out)    # noqa: E731
    p("fwd", "forward, compressed adjacency (adj[j:j+32], a view)")
    p("fwd_dense_in", "forward, dense adjacency (compressed on every call)")
    p("fwd_torch", "the same model as plain torch ops (torch.matmul(a, x) per layer) forward")
    p("step", "training step, compressed adjacency")
    p("step_dense_in", "training step, dense adjacency (compressed on every call)")
    p("step_torch", "plain torch ops training step")
    p("compress32", "compress_adjacency of one batch of 32 (the per-call cost of dense input)")
    p("eval", "one evaluation call over %d graphs, compressed adjacency" % n_test)
    p("eval_dense_in", "one evaluation call over %d graphs, dense adjacency" % n_test)
    p("eval_torch", "plain torch ops, one evaluation call over %d graphs" % n_test)
    p("compress_train", "compress_adjacency of the training adjacency (%d graphs, %.2f GB)" % (n_train, gb),
      "  (%.0f GB/s of dense input)" % (gb / rows["compress_train"] * 1e3))
    ratio = rows["step_torch"] / rows["step"]
    print("  training step against plain torch ops on this GPU: %.2fx %s"
          % (ratio, "faster" if ratio > 1 else "- the fused step is NOT faster"), file=out)
    print("  one epoch (%d steps): %.2f s fused (compressed once: + %.3f s), %.2f s fused with dense input, %.2f s "
          "plain torch ops; the notebook records %s on an unnamed CPU (context, not a comparison)"
          % (n_batches, n_batches * rows["step"] / 1e3, rows["compress_train"] / 1e3,
             n_batches * rows["step_dense_in"] / 1e3, n_batches * rows["step_torch"] / 1e3, recorded), file=out)


def trace_only():
    """Ten training steps per configuration for rocprofv3 --kernel-trace --stats: per step one k_gcn_fwd, one
    k_gcn_bwd and one k_gcn_reduce beside torch's loss and Adam kernels."""
    for name, kind, dims, _, _, _, _ in CONFIGS:
        X, A, Y = (torch.from_numpy(v).to(DEV) for v in (synth.toy_segment_graphs(32, seed=0) if kind == "gcn"
                                                         else synth.toy_hit_graphs(32, seed=0)))
        torch.manual_seed(0)
        m = (GCRNBinaryClassifier if kind == "gcrn" else GCNBinaryClassifier)(X.shape[-1], dims).to(DEV)
        adj = compress_adjacency(A)
        step = train_step(m, torch.optim.Adam(m.parameters()), X, adj, Y)
        for _ in range(10):
            step()
    torch.cuda.synchronize()
    print("trace run: 1 compression and 10 training steps at each notebook configuration (batch 32)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    if a.trace_only:
        trace_only()
        return
    print("# tools/gcn_probe.py on %s; HIP-event medians of %d calls after warm-up"
          % (torch.cuda.get_device_name(0), a.steps))
    accuracy(sys.stdout)
    sys.stdout.flush()
    for cfg in CONFIGS:
        config(cfg, a.steps, sys.stdout)
        sys.stdout.flush()


if __name__ == "__main__":
    main()
