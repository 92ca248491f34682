"""Device graph construction (graph_build.build_graphs on csrc/graph_build.hip) on c3-shaped barrel events: build
time for one event and for 256 (synchronised wall clock, median), the plan build the 256-event batch then needs,
hits to scores for one event (build + first forward of the default model route), segment counts, and the numpy
specification's host time for the same event.  The reference's own host time is the one tools/gen_graph_golden.py
--time recorded (tests/golden/graph_build/reference_time.json).

usage: python tools/graph_build_probe.py [--quick] [--out FILE]   (default FILE: profiles/graph_build_probe.txt)
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gnn_fpga_amd import synth  # noqa: E402
from gnn_fpga_amd.graph_build import build_graphs  # noqa: E402
from gnn_fpga_amd.model import SegmentClassifier  # noqa: E402

PAIRS = np.stack([np.arange(9), np.arange(1, 10)], axis=1)


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def on_dev(cols):
    return [torch.from_numpy(c).cuda() for c in cols[:5]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="few repetitions (for a profiler run)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "graph_build_probe.txt"))
    args = ap.parse_args()
    reps = 5 if args.quick else 50
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("graph_build probe on %s" % torch.cuda.get_device_name(0))
    for S in (8, 1):
        cols = synth.barrel_event(1000, 0, seed=11)              # the event reference_time.json was measured on
        r, phi, z, layer, pid = on_dev(cols)
        build = lambda: build_graphs(r, phi, z, layer, PAIRS, particle_id=pid, event_ptr=cols.event_ptr,  # noqa: E731
                                     n_phi_sectors=S)
        for _ in range(3):
            b = build()
        ms1 = median_ms(build, reps)
        say("one c3-shaped event, %d sector(s): %d hits, %d segments (%d true) in %d graphs; device build %.3f ms"
            % (S, b.n_hits, b.n_segments, int(b.y.sum().item()), b.n_graphs, ms1))
        if S == 8:
            t0 = time.perf_counter()
            h = build_graphs(cols.r, cols.phi, cols.z, cols.layer, PAIRS, particle_id=cols.particle_id,
                             n_phi_sectors=S)
            host_ms = (time.perf_counter() - t0) * 1e3
            assert h.n_segments == b.n_segments
            say("  numpy specification on the host, same event: %.1f ms" % host_ms)
            model = SegmentClassifier(input_dim=3, hidden_dim=8, n_iters=4).cuda().eval()

            def hits_to_scores():
                with torch.no_grad():
                    model(build())
            for _ in range(3):
                hits_to_scores()
            say("  hits to scores (build + first forward, use_plan=%r): %.3f ms"
                % (model.use_plan, median_ms(hits_to_scores, reps)))
    cols = synth.barrel_event(1000, 0, n_events=256, seed=12)
    r, phi, z, layer, pid = on_dev(cols)
    build = lambda: build_graphs(r, phi, z, layer, PAIRS, particle_id=pid, event_ptr=cols.event_ptr,  # noqa: E731
                                 n_phi_sectors=8)
    for _ in range(2):
        b = build()
    ms256 = median_ms(build, max(3, reps // 5))

    def plan():
        b.plan = None
        b.build_plan(8)
    plan()
    ms_plan = median_ms(plan, max(3, reps // 5))
    say("256 c3-shaped events, 8 sectors: %d hits, %d segments in %d graphs; device build %.3f ms; the plan build "
        "of that batch %.3f ms" % (b.n_hits, b.n_segments, b.n_graphs, ms256, ms_plan))
    ref = os.path.join(REPO, "tests", "golden", "graph_build", "reference_time.json")
    if os.path.exists(ref):
        rec = json.load(open(ref))
        say("reference construct_graph on a host CPU, same one event (recorded by gen_graph_golden.py --time): "
            "%.3f s, %d segments" % (rec["seconds"], rec["segments"]))
    if not args.quick:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
