"""Segment metrics on the GPU against the notebooks' host route (DESIGN §4 "k_metrics").

Measures, on one GPU:
  1. SegmentMetrics.update (csrc/metrics.hip) for c3 x 256 (25.6 M segments) and c5 x 8 (4 M), at the default
     resolution (1024 bins per octave) and the finest (8192), on three score shapes: the untrained model's scores
     of a c3 batch (a narrow pile), sigmoid-of-normal scores (a trained model's shape: fakes spread over many
     octaves near 0, trues piled up near 1) and uniform scores (the fewest shared bins); median of HIP-event
     timings; roofline.frac = (8 B per segment, 12 B with src) / time / 8 TB/s;
  2. the host route the notebooks take on the same c3 x 256 scores: read-back, then sklearn's accuracy_score,
     precision_score, recall_score on `e > 0.5` and roc_curve;
  3. evaluate() over an epoch of the c3 shape (256 graphs, batches of 32) against the same loop with torch.cat
     (Estimator.predict).

`--profile-target clustered|onebin` runs only 10 updates of 25.6 M segments (sigmoid-of-normal scores, or one
score value) for the counter runs of tools/metrics_counters.py.  profiles/metrics_probe.txt is
  python tools/metrics_probe.py > profiles/metrics_probe.txt && python tools/metrics_counters.py >> profiles/metrics_probe.txt

usage: python tools/metrics_probe.py [--no-host] [--profile-target clustered|onebin]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnn_fpga_amd import HitGraphBatch, SegmentMetrics, batch_generator, evaluate, synth  # noqa: E402
from gnn_fpga_amd.model import SegmentClassifier  # noqa: E402

HBM_PEAK_GBS = 8000.0


def time_update(m, e, y, batch=None, reps=20):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * reps)]
    for _ in range(3):
        m.update(e, y, batch=batch)
    ms = []
    for r in range(reps):
        ev[2 * r].record()
        m.update(e, y, batch=batch)
        ev[2 * r + 1].record()
    torch.cuda.synchronize()
    ms = [ev[2 * r].elapsed_time(ev[2 * r + 1]) for r in range(reps)]
    m.compute()
    return float(np.median(ms))


def line(label, n, ms, bpseg):
    gbs = n * bpseg / (ms * 1e-3) / 1e9
    print("  %-44s %9.4f ms  %6.2f G segments/s  %7.0f GB/s  roofline.frac %.3f"
          % (label, ms, n / ms / 1e6, gbs, gbs / HBM_PEAK_GBS), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-host", action="store_true", help="skip the sklearn host route")
    ap.add_argument("--profile-target", choices=("clustered", "onebin"), help="only 10 updates, for rocprofv3")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    if args.profile_target:
        profile_target(dev, args.profile_target)
        return
    print("device:", torch.cuda.get_device_name(dev))

    graphs = [synth.layered_graph(10000, 100000, 3, seed=1000 + i) for i in range(256)]
    batch = HitGraphBatch.from_graphs(graphs).to(dev)
    y = batch.y
    model = SegmentClassifier(input_dim=3, hidden_dim=8, n_iters=3).to(dev).eval()
    with torch.no_grad():
        e_model = model(batch)
    torch.cuda.synchronize()
    n = batch.n_segments
    g = torch.Generator(device=dev).manual_seed(1)
    shapes = {"model": e_model,
              "clustered": torch.sigmoid(torch.where(y > 0, 6.0, -7.0) + 3 * torch.randn(n, device=dev, generator=g)),
              "uniform": torch.rand(n, device=dev, generator=g)}
    print("\n1. update, c3 x 256 = %d segments (8 B / segment; with the batch's src 12 B)" % n)
    for bpo in (1024, 8192):
        for name, e in shapes.items():
            m = SegmentMetrics((0.5,), bins_per_octave=bpo, device=dev)
            line("%s, %d bins/octave" % (name, bpo), n, time_update(m, e, y), 8)
        m = SegmentMetrics((0.5,), bins_per_octave=bpo, device=dev)
        line("model, %d bins/octave, with src" % bpo, n, time_update(m, e_model, y, batch), 12)
    m = SegmentMetrics(tuple(np.linspace(0.05, 0.95, 16)), device=dev)
    line("model, 1024 bins/octave, 16 thresholds", n, time_update(m, e_model, y), 8)

    n5 = 8 * 500000
    e5 = shapes["clustered"][:n5].contiguous()
    y5 = y[:n5].contiguous()
    print("\nc5 x 8 = %d segments" % n5)
    for bpo in (1024, 8192):
        m = SegmentMetrics((0.5,), bins_per_octave=bpo, device=dev)
        line("clustered, %d bins/octave" % bpo, n5, time_update(m, e5, y5), 8)

    if not args.no_host:
        print("\n2. host route on the c3 x 256 model scores (read-back + sklearn)")
        try:
            from sklearn.metrics import accuracy_score, precision_score, recall_score, roc_curve
        except ImportError:
            print("  sklearn is not installed here: skipped")
        else:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eh, yh = e_model.cpu().numpy(), y.cpu().numpy()
            t1 = time.perf_counter()
            pred = eh > 0.5
            accuracy_score(yh, pred), precision_score(yh, pred), recall_score(yh, pred)
            t2 = time.perf_counter()
            roc_curve(yh, eh)
            t3 = time.perf_counter()
            print("  read-back %.1f ms, accuracy/precision/recall %.0f ms, roc_curve %.0f ms: %.2f s in all"
                  % (1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2), t3 - t0))
            m = SegmentMetrics((0.5,), device=dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.update(e_model, y)
            m.compute()
            m.roc()
            print("  the same on the GPU (update + compute + roc, synchronised wall clock): %.1f ms"
                  % (1e3 * (time.perf_counter() - t0)))

    print("\n3. an epoch of the c3 shape: 256 graphs, batches of 32, padded layout")
    del batch, shapes, e_model
    gen = batch_generator(graphs, 256, 32, device=dev, layout="padded")
    evaluate(model, gen, 8)                                  # batches built and cached, plans made
    torch.cuda.synchronize()
    for label, fn in (("evaluate (forward + metrics)", lambda: evaluate(model, gen, 8)),
                      ("predict loop (forward + torch.cat)", lambda: predict(model, gen, 8))):
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        print("  %-36s %.2f ms per epoch (median of 5)" % (label, 1e3 * float(np.median(ts))))


def profile_target(dev, kind, n=25600000):
    g = torch.Generator(device=dev).manual_seed(1)
    y = (torch.rand(n, device=dev, generator=g) < 0.3).float()
    if kind == "clustered":
        e = torch.sigmoid(torch.where(y > 0, 6.0, -7.0) + 3 * torch.randn(n, device=dev, generator=g))
    else:
        e = torch.full((n,), 0.375, device=dev)
    m = SegmentMetrics((0.5,), device=dev)
    for _ in range(10):
        m.update(e, y)
    torch.cuda.synchronize()
    print(kind, m.compute()["n"])


def predict(model, gen, n_batches):
    outs = []
    with torch.no_grad():
        for _ in range(n_batches):
            b, _ = next(gen)
            outs.append(model(b))
    return torch.cat(outs)


if __name__ == "__main__":
    main()
