"""Random batches (graph counts, sizes, layer counts, padded segments, every supported (F, D)) through the three
inference routes - first forward (gnn_csr_build + per-module kernels), fused tile pipeline, one-launch event kernels
where they apply - against each other and, for batches the C oracle finishes quickly, against the oracle: 1e-5."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from gnn_fpga_amd import HitGraphBatch, synth
from gnn_fpga_amd.model import SegmentClassifier
from oracle import index_c

trials = int(sys.argv[1]) if len(sys.argv) > 1 else 80
rng = np.random.default_rng(77)
SHAPES = [(2, 4), (2, 8), (2, 16), (2, 32), (3, 4), (3, 8), (3, 16), (3, 32), (3, 64), (11, 4), (11, 8), (11, 16)]
TOL = 1e-5
t0 = time.time()
worst = {"first_vs_fused": 0.0, "events_vs_fused": 0.0, "oracle": 0.0}
n_oracle = n_events = n_ill = 0
for t in range(trials):
    F, D = SHAPES[t % len(SHAPES)]
    T = int(rng.integers(0, 5))
    kind = int(rng.integers(0, 4))
    if kind == 0:       # many small graphs (event-kernel territory)
        graphs = [synth.layered_graph(int(rng.integers(2, 120)), int(rng.integers(0, 500)), F, n_layers=2,
                                      seed=int(rng.integers(1 << 30))) for _ in range(int(rng.integers(1, 300)))]
    elif kind == 1:     # medium graphs
        graphs = [synth.layered_graph(int(rng.integers(200, 3000)), int(rng.integers(500, 20000)), F,
                                      n_layers=int(rng.integers(2, 14)), seed=int(rng.integers(1 << 30)))
                  for _ in range(int(rng.integers(1, 24)))]
    elif kind == 2:     # detector-size graphs
        graphs = [synth.layered_graph(int(rng.integers(5000, 30000)), int(rng.integers(30000, 250000)), F,
                                      n_layers=int(rng.integers(3, 24)), seed=int(rng.integers(1 << 30)))
                  for _ in range(int(rng.integers(1, 5)))]
    else:               # one graph with few layers: long lists, levels wider than the LDS windows
        graphs = [synth.layered_graph(int(rng.integers(3000, 20000)), int(rng.integers(50000, 300000)), F,
                                      n_layers=int(rng.integers(2, 4)), seed=int(rng.integers(1 << 30)))]
    b = HitGraphBatch.from_graphs(graphs, pad_segments=bool(rng.random() < 0.2))
    src, dst = b.src.numpy().copy(), b.dst.numpy().copy()
    if src.size and rng.random() < 0.5:
        k = rng.random(src.size) < 0.1 * rng.random()
        src[k] = -1
        dst[k] = -1

    def fresh():
        return HitGraphBatch(b.X.numpy(), src, dst, hit_ptr=b.hit_ptr, seg_ptr=b.seg_ptr).cuda()

    torch.manual_seed(t)
    m = SegmentClassifier(input_dim=F, hidden_dim=D, n_iters=T).cuda().eval()
    with torch.no_grad():
        if rng.random() < 0.3:               # larger weights: scores away from 0.5, exp-product bound in play
            for p in m.parameters():
                p.mul_(float(rng.uniform(1.5, 4.0)))
        m.use_events = False
        m.use_plan = False
        e_first = m(fresh()).reshape(-1)
        m.use_plan = True
        e_fused = m(fresh()).reshape(-1)
        d = (e_first - e_fused).abs().max().item() if e_first.numel() else 0.0
        if d >= TOL:
            # which route left the truth?  (or neither: an ill-conditioned network amplifies the 1e-7 of another
            # summation order; then the fp32 oracle is as far from the fp64 one)
            params = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
            r64 = index_c.segment_classifier(b.X.numpy(), src, dst, params, T, f64=True)
            r32 = index_c.segment_classifier(b.X.numpy(), src, dst, params, T)
            print("trial %d F=%d D=%d T=%d kind %d: first vs fused %.2e; vs fp64 oracle: first %.2e fused %.2e fp32 oracle "
                  "%.2e; max |W| %.2f" % (t, F, D, T, kind, d, np.abs(e_first.cpu().numpy() - r64).max(),
                                          np.abs(e_fused.cpu().numpy() - r64).max(), np.abs(r32 - r64).max(),
                                          max(p.abs().max().item() for p in m.parameters())))
            ill = np.abs(r32 - r64).max() > TOL / 4
            assert ill, ("first vs fused", t, F, D, T, kind, d)
            n_ill += 1
            continue
        worst["first_vs_fused"] = max(worst["first_vs_fused"], d)
        m.use_events = True
        e_ev = m(fresh()).reshape(-1)
        if m._route.kind == "events":        # (call_route.choose_inference's answer for this batch)
            n_events += 1
            d = (e_ev - e_fused).abs().max().item() if e_ev.numel() else 0.0
            worst["events_vs_fused"] = max(worst["events_vs_fused"], d)
            assert d < TOL, ("events vs fused", t, F, D, T, kind, d)
    if b.n_segments * (T + 1) * D <= 40e6:   # the oracle on the host: seconds
        n_oracle += 1
        params = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
        ref = index_c.segment_classifier(b.X.numpy(), src, dst, params, T)
        d = float(np.abs(e_fused.cpu().numpy() - ref).max()) if ref.size else 0.0
        if d >= TOL:
            r64 = index_c.segment_classifier(b.X.numpy(), src, dst, params, T, f64=True)
            c = float(np.abs(ref - r64).max())
            print("trial %d F=%d D=%d T=%d kind %d: fused vs fp32 oracle %.2e; vs fp64 oracle: fused %.2e fp32 oracle %.2e"
                  % (t, F, D, T, kind, d, np.abs(e_fused.cpu().numpy() - r64).max(), c))
            assert c > TOL / 4, ("fused vs oracle", t, F, D, T, kind, d)
            n_ill += 1
            continue
        worst["oracle"] = max(worst["oracle"], d)
print("%d random batches, 12 (F, D) shapes, T = 0..4: first-forward route vs fused pipeline max %.2e; event kernels "
      "(%d batches) vs fused %.2e; fused vs the C oracle (%d batches) %.2e - bound 1e-5; %d ill-conditioned networks "
      "(scaled-up weights: the fp32 oracle itself leaves the fp64 one by more than 2.5e-6) set aside; %.0f s"
      % (trials, worst["first_vs_fused"], n_events, worst["events_vs_fused"], n_oracle, worst["oracle"], n_ill,
         time.time() - t0))
