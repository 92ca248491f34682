"""The hit classifier (gnn/MPNN_HitClassifier.ipynb) on one GPU, timed with HIP events after warm-up (median).

  1. the notebook's configuration (input_dim 4, hidden_dim 64, n_iters 7, batches of 32 samples of 50 hits /
     225 segments): NodeClassifier forward and training step (forward + BCE + backward + Adam), with dense inputs
     (the notebook's [X, Ri, Ro], converted on the device every call) and with index inputs (a HitGraphBatch),
     against the notebook's own model restated with dense matmuls (the oracle's dense EdgeNetwork / NodeNetwork
     plus the output network) on the same GPU; one epoch (1 219 steps, cell 25's 39 008 samples) projected;
  2. c3 x 32 (32 x 10 000 hits / 100 000 segments) with input_dim 4, hidden_dim 8, n_iters 3: NodeClassifier
     against SegmentClassifier with use_plan = False (the same trunk on the same per-module route).

`--trace-only` runs a few calls of each for a `rocprofv3 --kernel-trace --stats` run (kernels per call).
profiles/nodeclf_probe.txt is `python tools/nodeclf_probe.py > profiles/nodeclf_probe.txt`.

usage: python tools/nodeclf_probe.py [--steps N] [--trace-only]
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnn_fpga_amd import HitGraphBatch, synth  # noqa: E402
from gnn_fpga_amd.loss import BCELoss  # noqa: E402
from gnn_fpga_amd.model import NodeClassifier, SegmentClassifier  # noqa: E402
from oracle import dense_torch  # noqa: E402

DEV = torch.device("cuda:0")
EPOCH_STEPS = 1219                      # 39 008 training samples / 32 (cells 13, 25)


class DenseNodeClassifier(nn.Module):
    """The notebook's NodeClassifier with dense incidence matmuls (its own arithmetic), parameters from `src`."""

    def __init__(self, src):
        super().__init__()
        self.keys = list(src.state_dict())
        self.w = nn.ParameterList([nn.Parameter(v.detach().clone()) for v in src.state_dict().values()])
        self.n_iters = src.n_iters

    def forward(self, inputs):
        X, Ri, Ro = inputs
        p = dict(zip(self.keys, self.w))
        H = torch.cat([torch.tanh(F.linear(X, p["input_network.0.weight"], p["input_network.0.bias"])), X], dim=-1)
        for _ in range(self.n_iters):
            e = dense_torch.edge_network(H, Ri, Ro, p)
            H = torch.cat([dense_torch.node_network(H, e, Ri, Ro, p), X], dim=-1)
        return torch.sigmoid(F.linear(H, p["output_network.0.weight"], p["output_network.0.bias"])).squeeze(-1)


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


def train_step(model, opt, loss_func, inputs, y):
    def step():
        opt.zero_grad()
        loss = loss_func(model(inputs), y)
        loss.backward()
        opt.step()
    return step


def notebook_config(steps, out):
    s = synth.hit_classifier_samples(32, seed=0)
    dense = [torch.from_numpy(s.X).to(DEV), torch.from_numpy(s.Ri.astype(np.float32)).to(DEV),
             torch.from_numpy(s.Ro.astype(np.float32)).to(DEV)]
    y = torch.from_numpy(s.y.astype(np.float32)).to(DEV)
    index = HitGraphBatch.from_dense(*dense)
    torch.manual_seed(0)
    m = NodeClassifier(input_dim=4, hidden_dim=64, n_iters=7).to(DEV)
    ref = DenseNodeClassifier(m).to(DEV)
    rows = []
    with torch.no_grad():
        m.eval()
        rows.append(("forward, dense inputs", timed(lambda: m(dense), steps)))
        rows.append(("forward, index inputs", timed(lambda: m(index), steps)))
        rows.append(("notebook model (dense matmul) forward", timed(lambda: ref(dense), steps)))
    m.train()
    opt = torch.optim.Adam(m.parameters())
    rows.append(("training step, dense inputs, gnn_fpga_amd.loss.BCELoss",
                 timed(train_step(m, opt, BCELoss(), dense, y), steps)))
    rows.append(("training step, index inputs, gnn_fpga_amd.loss.BCELoss",
                 timed(train_step(m, opt, BCELoss(), index, y.reshape(-1)), steps)))
    rows.append(("training step, dense inputs, nn.BCELoss", timed(train_step(m, opt, nn.BCELoss(), dense, y), steps)))
    ropt = torch.optim.Adam(ref.parameters())
    rows.append(("notebook model (dense matmul) training step, nn.BCELoss",
                 timed(train_step(ref, ropt, nn.BCELoss(), dense, y), steps)))
    print("== notebook configuration: input_dim 4, hidden_dim 64, n_iters 7, batch 32 x (50 hits, 225 segments)",
          file=out)
    for name, ms in rows:
        print("  %-62s %8.3f ms" % (name, ms), file=out)
    ours, theirs = rows[3][1], rows[6][1]
    print("  training step speed-up against the notebook model on this GPU: %.2fx" % (theirs / ours), file=out)
    print("  one epoch (%d steps, dense inputs): %.2f s here; the notebook records 214-229 s per epoch on a CPU "
          "(cell 30; context, not a same-machine comparison)" % (EPOCH_STEPS, EPOCH_STEPS * ours / 1e3), file=out)


def c3_config(steps, out):
    graphs = [synth.layered_graph(10000, 100000, 4, seed=s) for s in range(32)]
    batch = HitGraphBatch.from_graphs(graphs).to(DEV)
    torch.manual_seed(1)
    n = NodeClassifier(input_dim=4, hidden_dim=8, n_iters=3).to(DEV)
    sc = SegmentClassifier(input_dim=4, hidden_dim=8, n_iters=3).to(DEV)
    sc.load_state_dict({k: v for k, v in n.state_dict().items() if not k.startswith("output_network")})
    sc.use_plan, sc.use_events, sc.level_order_training = False, False, False
    yh = torch.from_numpy((np.random.default_rng(0).random(batch.n_hits) < 0.3).astype(np.float32)).to(DEV)
    ys = torch.from_numpy(np.concatenate([g.y for g in graphs]).astype(np.float32)).to(DEV)
    with torch.no_grad():
        fn = timed(lambda: n.eval()(batch), steps)
        fs = timed(lambda: sc.eval()(batch), steps)
    tn = timed(train_step(n.train(), torch.optim.Adam(n.parameters()), BCELoss(), batch, yh), steps)
    ts = timed(train_step(sc.train(), torch.optim.Adam(sc.parameters()), BCELoss(), batch, ys), steps)
    print("== c3 x 32 (%d hits, %d segments), input_dim 4, hidden_dim 8, n_iters 3; SegmentClassifier with "
          "use_plan = False" % (batch.n_hits, batch.n_segments), file=out)
    print("  %-40s %8.3f ms   SegmentClassifier %8.3f ms   ratio %.3f" % ("forward: NodeClassifier", fn, fs, fn / fs),
          file=out)
    print("  %-40s %8.3f ms   SegmentClassifier %8.3f ms   ratio %.3f" % ("training step: NodeClassifier", tn, ts,
                                                                         tn / ts), file=out)


def trace_only():
    """A few calls of each, one marker line per phase, for rocprofv3 --kernel-trace --stats."""
    s = synth.hit_classifier_samples(32, seed=0)
    batch = HitGraphBatch.from_dense(torch.from_numpy(s.X).to(DEV), torch.from_numpy(s.Ri.astype(np.float32)).to(DEV),
                                     torch.from_numpy(s.Ro.astype(np.float32)).to(DEV))
    y = torch.from_numpy(s.y.astype(np.float32)).reshape(-1).to(DEV)
    for T in (0, 7):
        torch.manual_seed(0)
        m = NodeClassifier(input_dim=4, hidden_dim=64, n_iters=T).to(DEV)
        with torch.no_grad():
            for _ in range(10):
                m.eval()(batch)
        opt = torch.optim.Adam(m.parameters())
        step = train_step(m.train(), opt, BCELoss(), batch, y)
        for _ in range(10):
            step()
    torch.cuda.synchronize()
    print("trace run: 10 forwards and 10 training steps at n_iters 0 and 7 (hidden_dim 64, 32 x 50 hits)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    if a.trace_only:
        trace_only()
        return
    print("# tools/nodeclf_probe.py on %s; HIP-event medians of %d calls after warm-up"
          % (torch.cuda.get_device_name(0), a.steps))
    notebook_config(a.steps, sys.stdout)
    sys.stdout.flush()
    c3_config(a.steps, sys.stdout)


if __name__ == "__main__":
    main()
