"""Build time of build_muon_graphs (csrc/muon_graph.hip) at 1, 512 and 100 000 entries in both layouts, and hits to
scores (build + SegmentClassifier(input_dim=11, hidden_dim=8, n_iters=3) forward) for 1 and 512 entries in both
layouts, with the split between build and forward.  Inputs are synth.emtf_events; every figure is the mean of --reps
runs timed with HIP events after 3 warm-up runs.  The reference's host time per event is read from
tests/golden/muon_graph/reference_time.json (tools/gen_muon_graph_golden.py --time).

usage: python tools/muon_graph_probe.py [--reps N] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from gnn_fpga_amd import build_muon_graphs, synth  # noqa: E402
from gnn_fpga_amd.model import SegmentClassifier  # noqa: E402

DEV = torch.device("cuda:0")


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def inputs(n, seed):
    d = synth.emtf_events(n, seed=seed)
    to = lambda c: {k: torch.from_numpy(v).to(DEV) for k, v in c.items()}  # noqa: E731
    return d, (to(d["muon"]), to(d["pu"]), torch.from_numpy(d["vp_pt"]).to(DEV),
               torch.from_numpy(d["vp_eta"]).to(DEV))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def out(s=""):
        print(s)
        sys.stdout.flush()
        lines.append(s)

    with open(os.path.join(REPO, "tests", "golden", "muon_graph", "reference_time.json")) as f:
        ref = json.load(f)
    out("# tools/muon_graph_probe.py on one MI355X (gfx950), synth.emtf_events inputs; mean of %d runs timed with HIP "
        "events after 3 warm-up runs." % args.reps)
    out("# flat = two calls around one read-back of the sizes; padded = one call, no read-back.  numpy ms: the "
        "specification on the host, one run (not run at 100 000 entries).")
    out("# The reference (prepareMuonGraphs.main, host CPU, pandas): %.1f ms per event (%s)."
        % (ref["ms_per_event"], ref["what"]))
    out()
    out("%-10s %8s %8s %10s %12s %12s %12s" % ("entries", "hits", "segments", "flat ms", "padded ms", "us/entry",
                                               "numpy ms"))
    torch.manual_seed(0)
    model = SegmentClassifier(input_dim=11, hidden_dim=8, n_iters=3).to(DEV).eval()
    for n in (1, 512, 100_000):
        d, a = inputs(n, seed=n)
        reps = args.reps if n < 100_000 else max(args.reps // 5, 5)
        flat_ms = timed(lambda: build_muon_graphs(*a), reps)
        pad_ms = timed(lambda: build_muon_graphs(*a, layout="padded"), reps)
        r = build_muon_graphs(*a)
        host_ms = float("nan")
        if n <= 512:
            t0 = time.perf_counter()
            build_muon_graphs(d["muon"], d["pu"], d["vp_pt"], d["vp_eta"])
            host_ms = 1e3 * (time.perf_counter() - t0)
        out("%-10d %8d %8d %10.3f %12.3f %12.3f %12.1f" % (n, r.batch.n_hits, r.batch.n_segments, flat_ms, pad_ms,
                                                           1e3 * min(flat_ms, pad_ms) / n, host_ms))
    out()
    out("hits to scores: build + forward of a never-seen batch; forward alone on the built batch")
    out("%-10s %-8s %12s %12s %12s" % ("entries", "layout", "build ms", "forward ms", "total ms"))
    with torch.no_grad():
        for n in (1, 512):
            _, a = inputs(n, seed=100 + n)
            for layout in ("flat", "padded"):
                b_ms = timed(lambda: build_muon_graphs(*a, layout=layout), args.reps)
                res = build_muon_graphs(*a, layout=layout)
                f_ms = timed(lambda: model(res.batch), args.reps)
                t_ms = timed(lambda: model(build_muon_graphs(*a, layout=layout).batch), args.reps)
                out("%-10d %-8s %12.3f %12.3f %12.3f" % (n, layout, b_ms, f_ms, t_ms))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
