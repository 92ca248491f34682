"""The track fit on the GPU beside the stages before it and the specification on the host (DESIGN §4 "Track fit").

On the c3 x 256 batch of profiles/tracks_probe.txt (256 x synth.layered_graph(10000, 100000), scores from
synth.scores_from_labels, threshold 0.5, min_hits 3), in both modes of build_tracks, on one GPU, medians of HIP-event
timings after warm-up:
  forward  SegmentClassifier(3, 8, 3) on the batch (second forward onwards);
  labels   build_tracks (gnn_track_build_labels);
  fit      Tracks.fit on float64 columns that are on the device (gnn_track_fit alone: the lists exist by then), and
           on float32 columns (the cast to float64 is three torch ops in front of the kernel);
  host     fit_tracks_numpy on the read-back lists, wall clock, for context.
The coordinates are seeded normal columns (300 mm): the kernel's work does not depend on their values, only on the
lists - mode "best" gives 290 k tracks of 3 to 10 hits, mode "components" 258 components of which the cap of 32 hits
leaves almost none to walk.

usage: python tools/track_fit_probe.py [--graphs N] > profiles/track_fit_probe.txt
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnn_fpga_amd import HitGraphBatch, build_tracks, synth  # noqa: E402
from gnn_fpga_amd.model import SegmentClassifier  # noqa: E402
from gnn_fpga_amd.tracks import fit_tracks_numpy  # noqa: E402


def event_median(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * reps)]
    for r in range(reps):
        ev[2 * r].record()
        fn()
        ev[2 * r + 1].record()
    torch.cuda.synchronize()
    return float(np.median([ev[2 * r].elapsed_time(ev[2 * r + 1]) for r in range(reps)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=256, help="c3 graphs in the batch (256: the record's)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    print("device:", torch.cuda.get_device_name(dev))
    graphs = [synth.layered_graph(10000, 100000, 3, seed=1000 + i) for i in range(args.graphs)]
    batch = HitGraphBatch.from_graphs(graphs).to(dev)
    scores = torch.from_numpy(np.concatenate([synth.scores_from_labels(g.y, seed=i) for i, g in enumerate(graphs)])).to(dev)
    del graphs
    rng = np.random.default_rng(8)
    host_cols = [rng.normal(0.0, 300.0, size=batch.n_hits) for _ in range(3)]
    cols64 = [torch.from_numpy(c).to(dev) for c in host_cols]
    cols32 = [c.to(torch.float32) for c in cols64]
    print("c3 x %d: %d graphs, %d hits, %d segments" % (args.graphs, batch.n_graphs, batch.n_hits, batch.n_segments),
          flush=True)
    model = SegmentClassifier(input_dim=batch.n_features, hidden_dim=8, n_iters=3).to(dev).eval()
    with torch.no_grad():
        fwd = event_median(lambda: model(batch))
    print("  forward of the batch                      %9.4f ms" % fwd)
    for mode in ("components", "best"):
        t = build_tracks(batch, scores, 0.5, mode, 3)
        n_tracks, sizes = len(t), t.track_ptr.diff()
        fit = t.fit(*cols64)
        walked = int(sizes[sizes <= 32].sum()) if n_tracks else 0
        print("  mode %-10s tracks %d, hits in tracks %d, walked (tracks of <= 32 hits) %d, status 0: %d"
              % (mode, n_tracks, int(t.track_hits.numel()), walked, int((fit.status == 0).sum())))
        labels = event_median(lambda: build_tracks(batch, scores, 0.5, mode, 3))
        f64 = event_median(lambda: t.fit(*cols64))
        f32 = event_median(lambda: t.fit(*cols32))
        gbs = walked * 28 / (f64 * 1e-3) / 1e9 if f64 > 0 else 0.0
        print("    labels %9.4f ms   fit, float64 columns %9.4f ms (%.2f x the labels, %.2f x the forward; 28 bytes per "
              "walked hit: %.1f GB/s)   fit, float32 columns %9.4f ms" % (labels, f64, f64 / labels, f64 / fwd, gbs, f32),
              flush=True)
        ptr, hits = t.track_ptr.cpu().numpy(), t.track_hits.cpu().numpy()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            spec = fit_tracks_numpy(ptr, hits, *host_cols)
            ts.append(1e3 * (time.perf_counter() - t0))
        same = all(np.array_equal(getattr(fit, k).cpu().numpy(), spec[k], equal_nan=k in ("moments", "params"))
                   for k in ("moments", "params", "n_hits", "status"))
        print("    fit_tracks_numpy on the host %9.2f ms; the kernel's values equal its values: %s" % (np.median(ts), same))


if __name__ == "__main__":
    main()
