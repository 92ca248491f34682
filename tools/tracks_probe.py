"""Track building on the GPU, stage by stage, beside the forward of the same batch and the host route
(DESIGN §4 "Track building").

For each batch - c3 x 32 and c3 x 256 (synth.layered_graph(10000, 100000)), one c3 graph, 512 muon-size graphs -
with scores from the synthetic recipe (synth.scores_from_labels, threshold 0.5, min_hits 3), on one GPU, medians of
HIP-event timings after warm-up:
  labels   build_tracks in both modes (gnn_track_build_labels: asynchronous, nothing read back);
  lists    the first use of the lists: ONE read-back of the sizes + gnn_track_build_lists, synchronised wall clock;
  match    Tracks.match on seeded particle ids (the lists exist by then);
  kernels  the per-kernel split of labels + lists + match from the library's own event profiler, one call each;
  forward  SegmentClassifier(3 or 11, 8, 3) on the same batch (second forward onwards: the batch's plan is built);
  host     for context only: src, dst and the scores read back, scipy's connected_components on the kept segments.

usage: python tools/tracks_probe.py [--no-host] > profiles/tracks_probe.txt
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnn_fpga_amd import HitGraphBatch, _lib, build_tracks, synth  # noqa: E402
from gnn_fpga_amd.model import SegmentClassifier  # noqa: E402


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


def lists_median(make, reps=10, warm=2):
    """Wall clock of the first use of the lists of fresh tracks (the labels are done: synchronised before)."""
    ts = []
    for r in range(warm + reps):
        t = make()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t.track_ptr
        torch.cuda.synchronize()
        if r >= warm:
            ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts))


def kernel_split(fn):
    with _lib.profile() as p:
        fn()
    torch.cuda.synchronize()
    agg = {}
    for name, ms in p.records:
        agg[name] = agg.get(name, 0.0) + ms
    return ", ".join("%s %.3f" % (k, v) for k, v in sorted(agg.items(), key=lambda kv: -kv[1]) if v >= 0.0005)


def probe(label, graphs, dev, host):
    batch = HitGraphBatch.from_graphs(graphs).to(dev)
    scores = torch.from_numpy(np.concatenate([synth.scores_from_labels(g.y, seed=i) for i, g in enumerate(graphs)])).to(dev)
    rng = np.random.default_rng(7)
    pid = torch.from_numpy(rng.integers(-5, 1000, size=batch.n_hits) + 2 ** 40).to(dev)
    print("\n%s: %d graphs, %d hits, %d segments" % (label, batch.n_graphs, batch.n_hits, batch.n_segments), flush=True)
    model = SegmentClassifier(input_dim=batch.n_features, hidden_dim=8, n_iters=3).to(dev).eval()
    with torch.no_grad():
        fwd = event_median(lambda: model(batch))
    print("  forward of the batch                      %9.4f ms" % fwd)
    for mode in ("components", "best"):
        t = build_tracks(batch, scores, 0.5, mode, 3)
        n_tracks, sizes = len(t), t.track_ptr.diff()
        print("  mode %-10s kept %d, tracks %d, largest %d hits" % (mode, int(t.n_kept), n_tracks,
                                                                    int(sizes.max()) if n_tracks else 0))
        labels = event_median(lambda: build_tracks(batch, scores, 0.5, mode, 3))
        lists = lists_median(lambda: build_tracks(batch, scores, 0.5, mode, 3))
        match = event_median(lambda: t.match(pid))
        print("    labels %9.4f ms (%.2f x the forward)   lists + size read-back %9.4f ms   match %9.4f ms"
              % (labels, labels / fwd, lists, match), flush=True)
        try:
            print("    kernels, labels + lists [ms]: " + kernel_split(lambda: build_tracks(batch, scores, 0.5, mode, 3).track_ptr))
            print("    kernels, match [ms]: " + kernel_split(lambda: t.match(pid)))
        except Exception as exc:                         # the split is context: the medians above stand without it
            print("    (no per-kernel split: %s)" % exc)
    if host:
        try:
            from scipy.sparse import coo_matrix
            from scipy.sparse.csgraph import connected_components
        except ImportError:
            print("  host route: scipy is not installed here: skipped")
            return
        ts = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s, d, e = batch.src.cpu().numpy(), batch.dst.cpu().numpy(), scores.cpu().numpy()
            t1 = time.perf_counter()
            keep = (s >= 0) & (e > np.float32(0.5))
            adj = coo_matrix((np.ones(int(keep.sum()), np.int8), (s[keep], d[keep])), shape=(batch.n_hits, batch.n_hits))
            connected_components(adj, directed=False)
            ts.append((1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1)))
        rb, cc = np.median([t[0] for t in ts]), np.median([t[1] for t in ts])
        print("  host route (components only): read-back %.2f ms + scipy connected_components %.2f ms = %.2f ms"
              % (rb, cc, rb + cc))


def cpu_name():
    try:
        with open("/proc/cpuinfo") as fh:
            for ln in fh:
                if ln.startswith("model name"):
                    return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown CPU"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-host", action="store_true", help="skip the scipy host route")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    print("device:", torch.cuda.get_device_name(dev))
    print("host route on: %s, %d threads (torch), scipy single-threaded" % (cpu_name(), torch.get_num_threads()))
    c3 = [synth.layered_graph(10000, 100000, 3, seed=1000 + i) for i in range(256)]
    probe("one c3 graph", c3[:1], dev, not args.no_host)
    probe("c3 x 32", c3[:32], dev, not args.no_host)
    probe("c3 x 256", c3, dev, not args.no_host)
    del c3
    probe("512 muon-size graphs", [synth.muon_graph(seed=i) for i in range(512)], dev, not args.no_host)


if __name__ == "__main__":
    main()
