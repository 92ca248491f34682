"""The toy MPNN classifiers' routes against each other and against plain torch ops, on the GPU (HIP events).

Two workloads: the notebook's configuration (gnn/MPNN_Seg_Toy2D.ipynb cells 7, 17: batches of 32 events of 40 hits and
144 segments, input_dim 2, hidden_dim 32, n_iters 10) and 512 muon-size graphs (input_dim 11, hidden_dim 8, n_iters 3).
At each, for the per-iteration class and the shared-weight class: the inference forward and one training step
(forward, nn.BCELoss, backward, Adam step) on
  iter_events   the one-launch kernels (csrc/iter_events.hip)
  per_module    the notebook's forward on the per-module kernels
  torch         the same model as plain torch ops on the same GPU, index form (gather, index_add_), restated below
after 10 warm-up calls, 50 timed calls each between two HIP events with a synchronise: median and min in ms.
The notebook records 18.3 - 19.0 s per training epoch of 820 batches (cell 20's output, a 2018 GPU, dense matmuls):
23 ms per training step.

usage: python tools/toy_mpnn_probe.py [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from gnn_fpga_amd import HitGraphBatch, ToySegmentClassifier, ToySegmentClassifier2, synth  # noqa: E402

WARM, REPS = 10, 50


class TorchEdge(nn.Module):
    def __init__(self, C, D):
        super().__init__()
        self.network = nn.Sequential(nn.Linear(2 * C, D), nn.Tanh(), nn.Linear(D, 1), nn.Sigmoid())

    def forward(self, H, src, dst):
        return self.network(torch.cat([H[src], H[dst]], dim=1)).squeeze(-1)


class TorchNode(nn.Module):
    def __init__(self, C, D):
        super().__init__()
        self.network = nn.Sequential(nn.Linear(3 * C, D), nn.Tanh(), nn.Linear(D, D), nn.Tanh())

    def forward(self, H, e, src, dst):
        w = e[:, None]
        mi = torch.zeros_like(H).index_add_(0, dst, w * H[src])
        mo = torch.zeros_like(H).index_add_(0, src, w * H[dst])
        return self.network(torch.cat([mi, mo, H], dim=1))


class TorchClassifier(nn.Module):
    """Cell 14 in index form with torch ops (no padded segments in the probe's batches)."""

    def __init__(self, F, D, T, shared):
        super().__init__()
        C = F + D
        self.input_network = nn.Sequential(nn.Linear(F, D), nn.Tanh())
        n = 1 if shared else T
        self.edges = nn.ModuleList([TorchEdge(C, D) for _ in range(n + (0 if shared else 1))])
        self.nodes = nn.ModuleList([TorchNode(C, D) for _ in range(n)])
        self.T, self.shared = T, shared

    def forward(self, X, src, dst):
        H = torch.cat([self.input_network(X), X], dim=1)
        for i in range(self.T):
            k = 0 if self.shared else i
            e = self.edges[k](H, src, dst)
            H = torch.cat([self.nodes[k](H, e, src, dst), X], dim=1)
        return self.edges[0 if self.shared else self.T](H, src, dst)


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def measure(model, call, y):
    opt = torch.optim.Adam(model.parameters())
    loss_fn = nn.BCELoss()

    def infer():
        with torch.no_grad():
            call()

    def step():
        opt.zero_grad()
        loss_fn(call().reshape(-1), y).backward()
        opt.step()
    model.eval()
    inf = timed(infer)
    model.train()
    return inf, timed(step)


def workload(name, graphs, F, D, T, out):
    batch = HitGraphBatch.from_graphs(graphs).to("cuda")
    y = batch.y
    src, dst = batch.src.long(), batch.dst.long()
    out("%s: %d graphs, %d hits, %d segments, input_dim %d, hidden_dim %d, n_iters %d"
        % (name, batch.n_graphs, batch.n_hits, batch.n_segments, F, D, T))
    out("  %-10s %-12s %22s %22s" % ("class", "route", "inference median / min", "training step median / min"))
    for shared in (False, True):
        cls = ToySegmentClassifier2 if shared else ToySegmentClassifier
        for route in ("iter_events", "per_module", "torch"):
            torch.manual_seed(0)
            if route == "torch":
                m = TorchClassifier(F, D, T, shared).cuda()
                call = lambda m=m: m(batch.X, src, dst)                 # noqa: E731
            else:
                m = cls(F, D, T).cuda()
                m.use_events = route == "iter_events"
                call = lambda m=m: m(batch)                             # noqa: E731
            inf, stp = measure(m, call, y)
            if route != "torch":
                assert m._route.kind == route, (m._route.kind, route)
            out("  %-10s %-12s %10.3f / %8.3f ms %10.3f / %8.3f ms"
                % ("shared" if shared else "unshared", route, inf[0], inf[1], stp[0], stp[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on a GPU; there is nothing to measure without one"
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    out("toy_mpnn_probe: %s, %d warm-up + %d timed calls per figure (HIP events)" % (torch.cuda.get_device_name(0), WARM, REPS))
    workload("notebook", [synth.toy2d_graph(s) for s in range(32)], 2, 32, 10, out)
    workload("muon", [synth.muon_graph(s) for s in range(512)], 11, 8, 3, out)
    out("reference: 18.3 - 19.0 s per epoch of 820 batches of 32 (notebook cell 20's output) = 22 - 23 ms per training step")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
