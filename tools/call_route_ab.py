"""Host overhead of one model call, for A / B runs of two checkouts that share one built library (profiles/call_route_ab.txt):
the eager loops of tools/latency_probe.py on its three launch-bound configurations, and the c3 x 32 training step of
tools/twin_probe.py through autograd and through GradBucket.step.  One process, one line of numbers.
usage: python tools/call_route_ab.py [label]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gnn_fpga_amd import HitGraphBatch, synth, shard
from gnn_fpga_amd.loss import BCELoss
from gnn_fpga_amd.model import SegmentClassifier


def timed(fn, warm, reps):
    for _ in range(warm): fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def forward_us(graphs, F, events, reps=2000):
    torch.manual_seed(0)
    m = SegmentClassifier(input_dim=F, hidden_dim=8, n_iters=3).cuda().eval()
    m.use_events = events
    b = HitGraphBatch.from_graphs(graphs).cuda()
    if not events:
        b.build_plan(8)
    with torch.no_grad():
        return timed(lambda: m(b), 50, reps) * 1e6


C3X32 = [synth.layered_graph(10000, 100000, 3, seed=s) for s in range(32)]


def train_ms(direct, reps=40):
    torch.manual_seed(0)
    m = SegmentClassifier(input_dim=3, hidden_dim=8, n_iters=3).cuda().train()
    b = HitGraphBatch.from_graphs(C3X32).cuda()
    y = (torch.rand(b.n_segments, device="cuda") < 0.3).float()
    bucket = shard.GradBucket(m.parameters())
    loss_fn = BCELoss(reduction="sum")

    def autograd_step():
        bucket.zero()
        loss = loss_fn(m(b), y)
        loss.backward()
        bucket.allreduce(loss.detach(), y.numel())
    return timed((lambda: bucket.step(m, b, y)) if direct else autograd_step, 5, reps) * 1e3


label = sys.argv[1] if len(sys.argv) > 1 else "-"
muon = [synth.muon_graph(0)]
print("%-6s muon_event_us %.2f muon_event_tiled_us %.2f c3_graph_us %.2f train_autograd_ms %.4f train_direct_ms %.4f"
      % (label, forward_us(muon, 11, True), forward_us(muon, 11, False),
         forward_us(C3X32[:1], 3, True, reps=500), train_ms(False), train_ms(True)))
