"""The fixed-point forward (gnn_fx_forward, csrc/fixed_point.hip) timed on the GPU beside the float32 per-module forward
(gnn_segclf_forward) and the numpy specification on the host.

Workloads: c3 x 32 and c3 x 256 (bench.py's c3 graphs: 10k hits, 100k segments, input_dim 3, hidden_dim 8, 3
iterations) and one mu200-shaped graph (50k hits, 500k segments, hidden_dim 64, 6 iterations), each in formats (16, 6)
and (24, 8) with 10 table bits.  Per figure: WARM warm-up calls, then REPS calls each between two HIP events with a
synchronise; median and min in ms.  The specification runs once on the host (for c3 x 256 on the first 32 graphs: the
batch is block-diagonal, so its cost per graph does not depend on the batch).  Every timed configuration is first
compared with the specification bit for bit (c3 x 256: on its first 32 graphs' segments).

`--trace-only` runs 3 calls per configuration and nothing else, for `rocprofv3 --kernel-trace --stats`.

usage: python tools/fixed_point_probe.py [--out FILE] [--trace-only] [--small]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from gnn_fpga_amd import FixedPointFormat, HitGraphBatch, _lib, fixed_forward_numpy, quantize_model, synth  # noqa: E402
from gnn_fpga_amd.model import SegmentClassifier  # noqa: E402

WARM, REPS = 3, 15
FORMATS = (FixedPointFormat(16, 6), FixedPointFormat(24, 8))


def timed(fn, warm=WARM, reps=REPS):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def workloads(small):
    k = 20 if small else 1
    return [("c3 x 32", 32 // (8 if small else 1), 10000 // k, 100000 // k, 3, 8, 3),
            ("c3 x 256", 256 // (32 if small else 1), 10000 // k, 100000 // k, 3, 8, 3),
            ("mu200 x 1", 1, 50000 // k, 500000 // k, 3, 64, 6)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--small", action="store_true", help="a rehearsal at a twentieth of the sizes")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fixed_point_probe needs a GPU")
    dev = torch.device("cuda:0")
    lines = ["fixed_point_probe: %s, %d warm-up + %d timed calls per figure (HIP events)"
             % (torch.cuda.get_device_name(0), WARM, REPS)]
    for name, G, n, e, F, D, T in workloads(args.small):
        graphs = [synth.layered_graph(n, e, F, seed=100 + s) for s in range(G)]
        n_spec = min(G, 32 // (8 if args.small else 1))
        batch = HitGraphBatch.from_graphs(graphs).to(dev)
        torch.manual_seed(0)
        model = SegmentClassifier(input_dim=F, hidden_dim=D, n_iters=T).to(dev).eval()
        weights = model.effective_weights()
        host_w = [w.cpu().numpy() for w in weights]
        _ = batch.in_ptr                    # the segment lists: built once, outside every timing
        if args.trace_only:
            for f in FORMATS:
                qm = quantize_model(model, f)
                for _ in range(3):
                    qm(batch)
            for _ in range(3):
                _lib.segclf_forward(batch, weights, F, D, T)
            torch.cuda.synchronize()
            continue
        lines.append("%s: %d graph(s), %d hits, %d segments, input_dim %d, hidden_dim %d, n_iters %d"
                     % (name, G, batch.n_hits, batch.n_segments, F, D, T))
        fp32 = timed(lambda: _lib.segclf_forward(batch, weights, F, D, T))
        lines.append("  float32 per-module (gnn_segclf_forward)   %9.3f / %9.3f ms (median / min)" % fp32)
        sub = HitGraphBatch.from_graphs(graphs[:n_spec])
        for f in FORMATS:
            qm = quantize_model(model, f)
            t0 = time.perf_counter()
            want = fixed_forward_numpy(sub.X.numpy(), sub.src.numpy(), sub.dst.numpy(), host_w, T, f)
            spec_s = time.perf_counter() - t0
            out = qm(batch)
            same = bool(np.array_equal(out.raw[:sub.n_segments].cpu().numpy(), want.raw))
            if n_spec == G:
                same = same and bool(np.array_equal(out.counts.cpu().numpy(), want.counts))
            med, mn = timed(lambda: qm(batch))
            lines.append("  fixed (%2d, %d) tb %d (gnn_fx_forward)       %9.3f / %9.3f ms   %.2f x float32   numpy "
                         "specification %.2f s on %d graph(s)   bit-equal: %s   overflows %d"
                         % (f.total_bits, f.int_bits, f.table_bits, med, mn, med / fp32[0], spec_s, n_spec, same,
                            int(out.counts.sum().item())))
            with _lib.profile(64) as prof:
                qm(batch)
                torch.cuda.synchronize()
            agg = {}
            for k, ms in prof.records:
                agg[k] = agg.get(k, 0.0) + ms
            lines.append("    per kernel, one call (HIP events between launches): "
                         + ", ".join("%s %.3f" % kv for kv in sorted(agg.items(), key=lambda kv: -kv[1])) + " ms")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
