"""Build time of build_event_graphs (csrc/event_graphs.hip, both calls and the one read-back of the sizes) on
(a) the 5 000-hit event the reference's cell 8 was timed on (tests/golden/event_graphs/reference_time.json, written
by tools/gen_event_graphs_golden.py --time), (b) one event of at least 13 000 hits, which the reference cannot build,
and (c) 4 096 notebook-size events in one call with the notebook's occupancy filter, and the same events from hits
to scores through SegmentClassifier(3, 32, 4).  Inputs are synth.acts_events; every figure is the median of --reps
runs, each timed with its own pair of HIP events, after 3 warm-up runs.  The numpy specification's host time on the
same input is one run.

usage: python tools/event_graphs_probe.py [--reps N] [--builds-only] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from gnn_fpga_amd import build_event_graphs, synth  # noqa: E402
from gnn_fpga_amd.model import SegmentClassifier  # noqa: E402

DEV = torch.device("cuda:0")
NOTEBOOK_BOUNDS = dict(n_nodes_min=50, n_nodes_max=500, n_edges_max=1000)


def timed(fn, reps):
    """Median and spread (min, max) in ms of `reps` runs, each between two HIP events, after 3 warm-up runs."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--builds-only", action="store_true", help="no model: the run a kernel trace is taken from")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def out(s=""):
        print(s)
        sys.stdout.flush()
        lines.append(s)

    with open(os.path.join(REPO, "tests", "golden", "event_graphs", "reference_time.json")) as f:
        ref = json.load(f)
    out("# tools/event_graphs_probe.py on one MI355X (gfx950), synth.acts_events inputs; median (min .. max) of %d runs, "
        "each timed with HIP events, after 3 warm-up runs." % args.reps)
    out("# device ms: build_event_graphs on CUDA tensors, both library calls and the read-back of the sizes between "
        "them.  numpy ms: the specification on the host, one run.")
    out("# The reference (cell 8 construct_graph, host CPU): %.2f s for %d hits and %d segments (%s)."
        % (ref["seconds"], ref["hits"], ref["segments"], ref["what"]))
    out()
    shapes = (("(a) the reference_time.json event", (1, 380, 1350), 11, {}),
              ("(b) one event of 13 000 hits", (1, 1000, 3500), 214, {}),
              ("(c) 4 096 notebook-size events, filter 50 / 500 / 1000", (4096, (4, 40), (10, 100)), 216,
               NOTEBOOK_BOUNDS))
    out("%-56s %8s %7s %8s %9s %30s %10s" % ("input", "rows", "graphs", "hits", "segments", "device ms", "numpy ms"))
    kept = {}
    for name, a, seed, kw in shapes:
        ev = synth.acts_events(*a, seed=seed)
        cols = [torch.from_numpy(c).to(DEV) for c in ev[:6]]
        med, lo, hi = timed(lambda: build_event_graphs(*cols, ev.event_ptr, **kw), args.reps)
        g = build_event_graphs(*cols, ev.event_ptr, **kw)
        t0 = time.perf_counter()
        h = build_event_graphs(*ev, **kw)
        host_ms = 1e3 * (time.perf_counter() - t0)
        assert h.batch.n_segments == g.batch.n_segments and torch.equal(g.batch.src.cpu(), h.batch.src)
        if name.startswith("(a)"):
            assert (g.batch.n_hits, g.batch.n_segments) == (ref["hits"], ref["segments"]), "not the recorded event"
        out("%-56s %8d %7d %8d %9d %30s %10.1f" % (name, ev.r.shape[0], len(g), g.batch.n_hits, g.batch.n_segments,
                                                   "%.3f (%.3f .. %.3f)" % (med, lo, hi), host_ms))
        kept[name[:3]] = (cols, ev.event_ptr, kw)
    if not args.builds_only:
        out()
        out("(c) from hits to scores: build + SegmentClassifier(3, 32, 4) forward of the never-seen batch of all kept "
            "graphs; forward alone on a built batch")
        cols, ep, kw = kept["(c)"]
        torch.manual_seed(0)
        model = SegmentClassifier(input_dim=3, hidden_dim=32, n_iters=4).to(DEV).eval()
        with torch.no_grad():
            b = build_event_graphs(*cols, ep, **kw).batch
            for what, fn in (("build", lambda: build_event_graphs(*cols, ep, **kw)),
                             ("forward alone", lambda: model(b)),
                             ("build + forward", lambda: model(build_event_graphs(*cols, ep, **kw).batch))):
                out("%-20s %30s ms" % ((what,) + ("%.3f (%.3f .. %.3f)" % timed(fn, args.reps),)))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
