"""The toy graph builders (gnn_fpga_amd/toy_graphs.py, csrc/toy_graphs.hip) on one GPU, at the notebooks' data set sizes.

  1. the distance between the segment kernel's expf and numpy's float32 exp on every fixture of
     tests/golden/toy_graphs, in ulps, over the entries whose reference is a normal number (the figure
     tests/test_gpu_toy_graphs.py's bound is made of);
  2. both builders at the notebooks' sizes - 32 768 events x (10 layers, 5 tracks) segment graphs
     (gnn/GCN_Seg_Toy2D.ipynb cell 7) and 65 536 x (10, 4) hit graphs (gnn/GCN_Toy2D.ipynb cell 7): HIP-event median,
     fastest and slowest of `--steps` calls after warm-up, the bytes a call writes (computed from the shapes) over that
     time, and that rate beside the float4-copy rate of tools/hbm_copy_probe (run here when it has been built:
     hipcc --offload-arch=gfx950 -O3 -o tools/hbm_copy_probe tools/hbm_copy_probe.hip);
  3. three host-side numbers from the same box: the numpy specification (synth.py) at a size that fits in memory, the
     previous path - the specification's dense adjacency uploaded and compressed by compress_adjacency - and the
     notebooks' own cells as tools/gen_toy_graphs_golden.py --time timed them (tests/golden/toy_graphs/
     reference_time.json; taken on the box that made the fixtures, so context rather than a comparison);
  4. one epoch of each notebook's training loop (batches of 32 over the first 90 % of the events) fed from the built
     lists, adj[j:j+32] per step, timed by a host clock around the loop and a device synchronise.

profiles/toy_graphs_probe.txt is `python tools/toy_graphs_probe.py > profiles/toy_graphs_probe.txt`.

usage: python tools/toy_graphs_probe.py [--steps N]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import toy_graphs_fixtures as fx  # noqa: E402
from gnn_fpga_amd import synth, toy_graphs  # noqa: E402
from gnn_fpga_amd.gcn import GCNBinaryClassifier, GCRNBinaryClassifier, compress_adjacency  # noqa: E402

DEV = torch.device("cuda:0")
FLT_MIN = np.finfo(np.float32).tiny


def timed(fn, steps, warmup=3):
    """HIP-event (median, fastest, slowest) milliseconds of `steps` calls after warm-up."""
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
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def copy_rate():
    """The best float4 copy rate tools/hbm_copy_probe prints (TB/s, read + written bytes), or None."""
    exe = os.path.join(REPO, "tools", "hbm_copy_probe")
    if not os.path.exists(exe):
        return None
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300).stdout
    rates = [float(v) for v in re.findall(r"copy \(1R\+1W\) ([0-9.]+) TB/s", out)]
    return max(rates) if rates else None


def sorted_hits(E, T, seed, chunk=8192):
    """Sorted hits of E seeded events on the device: (hit_x float32 [E, 10 T], hit_y int64)."""
    xs, ys = [], []
    for i in range(0, E, chunk):
        tracks = torch.from_numpy(synth.toy_tracks(min(chunk, E - i), T, seed=seed + i)).to(DEV)
        x, y = toy_graphs.sort_toy_tracks(tracks)
        xs.append(x)
        ys.append(y)
    return torch.cat(xs), torch.cat(ys)


def ulps(out):
    print("== segment kernel values against numpy's float32 exp on the fixtures (reference a normal number): ulps", file=out)
    worst_all = 0
    for shape in fx.SHAPES:
        d = fx.load("seg_" + shape)
        g = toy_graphs.build_toy_segment_graphs(torch.from_numpy(d["hit_x"].copy()).to(DEV),
                                                torch.from_numpy(d["hit_y"].copy()).to(DEV),
                                                det_r=d["det_r"], sigma=float(d["sigma"]))
        D = g.adj.to_dense().cpu().numpy()
        ref, val = d["A_vals"], D[d["A_batch"], d["A_rows"], d["A_cols"]]
        n = ref >= FLT_MIN
        dist = np.abs(val[n].view(np.int32).astype(np.int64) - ref[n].view(np.int32).astype(np.int64))
        small = np.abs(val[~n].astype(np.float64) - ref[~n].astype(np.float64)).max(initial=0.0)
        hist = np.bincount(dist, minlength=1)
        worst_all = max(worst_all, int(dist.max(initial=0)))
        print("  seg_%-8s %5d normal entries: worst %d ulps (histogram %s); %5d sub-normal or zero: worst absolute error "
              "%.3e (FLT_MIN %.3e), sub-normal share of the structural entries %.4f"
              % (shape, int(n.sum()), int(dist.max(initial=0)), hist.tolist(), int((~n).sum()), small, FLT_MIN,
                 float(((ref > 0) & (ref < FLT_MIN)).mean()) if ref.size else 0.0), file=out)
    print("  worst over the fixtures: %d ulps" % worst_all, file=out)


def epoch(model, X, y, adj, n_train):
    """One epoch of the notebooks' loop (Seg cell 27 / Toy2D cell 21): batches of 32, Adam; host seconds."""
    opt = torch.optim.Adam(model.parameters())
    loss_func = nn.BCEWithLogitsLoss()
    model.train()

    def run():
        for j in range(0, n_train, 32):
            k = min(j + 32, n_train)
            model.zero_grad()
            loss_func(model(X[j:k], adj[j:k]), y[j:k]).backward()
            opt.step()
        torch.cuda.synchronize()
    run()                                                                    # warm-up: every shape of the timed loop
    t0 = time.perf_counter()
    run()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    out = sys.stdout
    rate = copy_rate()                                                       # (before this process opens the GPU)
    if not torch.cuda.is_available():
        sys.exit("toy_graphs_probe needs a GPU: nothing here can be measured without one")
    print("# tools/toy_graphs_probe.py on %s; HIP-event median (fastest .. slowest) of %d calls after warm-up"
          % (torch.cuda.get_device_name(0), a.steps), file=out)
    ulps(out)
    ref_time = {}
    path = os.path.join(fx.GOLDEN, "reference_time.json")
    if os.path.exists(path):
        ref_time = json.load(open(path))
    print("== float4 copy of tools/hbm_copy_probe on this GPU: %s"
          % ("%.2f TB/s (bytes read + bytes written)" % rate if rate else "not measured (tools/hbm_copy_probe not built)"),
          file=out)
    for name, E, T, build, key in (
            ("segment graphs, 32768 events x (10, 5): 225 segments, list width 10", 32768, 5,
             lambda x, y: toy_graphs.build_toy_segment_graphs(x, y, check=False), "segments_l10_t5"),
            ("hit graphs, 65536 events x (10, 4), norm_adjacency: 40 hits, list width 8", 65536, 4,
             lambda x, y: toy_graphs.build_toy_hit_graphs(x, y, norm="row", check=False), "hits_l10_t4")):
        seg = key.startswith("seg")
        hx, hy = sorted_hits(E, T, seed=1)
        if not seg:
            hx = hx.double()
        hy32 = hy.to(torch.int32)
        g = build(hx, hy32)
        adj = g.adj
        tensors = [g.X, g[1], adj.row_cnt, adj.row_idx, adj.row_val] + ([] if seg else [adj.col_cnt, adj.col_idx,
                                                                                         adj.col_val])
        written = sum(t.numel() * t.element_size() for t in tensors)
        read = hx.numel() * hx.element_size() + hy32.numel() * 4
        del g, adj, tensors
        med, lo, hi = timed(lambda: build(hx, hy32), a.steps)
        print("== %s" % name, file=out)
        print("  build, one launch, nothing read back      %8.3f ms (%.3f .. %.3f)   %.1f MB written, %.1f MB read: "
              "%.2f TB/s written%s" % (med, lo, hi, written / 1e6, read / 1e6, written / med / 1e9,
                                       ", %.0f %% of the copy rate" % (100 * written / med / 1e9 / rate) if rate else ""),
              file=out)
        checked = ((lambda: toy_graphs.build_toy_segment_graphs(hx, hy32)) if seg
                   else (lambda: toy_graphs.build_toy_hit_graphs(hx, hy32, norm="row")))
        med_c, lo_c, hi_c = timed(checked, a.steps)
        print("  the same with check=True (isfinite, 1 flag read back) %8.3f ms (%.3f .. %.3f)" % (med_c, lo_c, hi_c),
              file=out)
        # host side: the numpy specification, and the previous path (its dense adjacency uploaded and compressed)
        n = 256 if seg else 4096
        x_h, y_h = hx[:n].cpu().numpy(), hy[:n].cpu().numpy()
        spec = ((lambda: synth.toy_segment_graphs_from_hits(x_h, y_h)) if seg
                else (lambda: synth.toy_hit_graphs_from_hits(x_h, y_h, norm="row")))
        spec()
        t0 = time.perf_counter()
        X, A, _ = spec()
        t_spec = time.perf_counter() - t0

        def previous():
            adj = compress_adjacency(torch.from_numpy(A).to(DEV))
            torch.cuda.synchronize()
            return adj
        previous()
        t0 = time.perf_counter()
        previous()
        t_prev = time.perf_counter() - t0
        print("  numpy specification, %d events             %8.3f ms = %.2f us per event -> %.2f s for %d events"
              % (n, t_spec * 1e3, t_spec / n * 1e6, t_spec / n * E, E), file=out)
        print("  previous path: + dense upload + compress_adjacency, %d events (%.0f MB dense)  %8.3f ms = %.2f us per "
              "event -> %.2f s for %d events with the specification's time"
              % (n, A.nbytes / 1e6, t_prev * 1e3, t_prev / n * 1e6, (t_spec + t_prev) / n * E, E), file=out)
        if key in ref_time:
            r = ref_time[key]
            print("  the notebook's own cells (%s), timed at %d events where the fixtures were made: %.1f us per event -> "
                  "%.1f s for %d events" % (r["cells"], r["events"], r["seconds_per_event"] * 1e6,
                                            r["seconds_per_event"] * E, E), file=out)
        print("  this builder: %.3f us per event" % (med * 1e3 / E), file=out)
        # one epoch of the notebook's loop from the built lists
        g = build(hx, hy32)
        torch.manual_seed(0)
        model = (GCNBinaryClassifier(5, [16] * 5) if seg else GCRNBinaryClassifier(3, [8] * 12)).to(DEV)
        n_train = int(0.9 * E)
        t_ep = epoch(model, g.X, g[1], g.adj, n_train)
        print("  one epoch of the notebook's loop from the built lists (%d events, %d steps of 32): %.2f s; building "
              "the whole data set is %.2f %% of it" % (n_train, (n_train + 31) // 32, t_ep, 100 * med / 1e3 / t_ep),
              file=out)
        out.flush()
        del g, hx, hy, hy32


if __name__ == "__main__":
    main()
