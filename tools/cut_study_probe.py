"""The cut study and the layer census on the device (cut_study.study_segment_cuts / count_layer_transitions on
csrc/graph_build.hip gnn_cut_study and csrc/layer_census.hip): synchronised wall-clock time (median, warmed up) for one
c3-shaped event with 8 sectors and with 1, for 256 such events, and for one mu200-sized event (about 15 k hits, 1
sector).  Beside each study time: gnn_graph_build_sizes on the same input (the same staging and the same all-pairs
loop with the cut test where the histogram update is; its pair kernel is k_gb_count), and both pair kernels' own
times from the library's HIP-event profiler in a separate, untimed call.  The reference's host times are the ones
tools/gen_cut_study_golden.py --time recorded (tests/golden/cut_study/reference_time.json).  Nothing is gated.

usage: python tools/cut_study_probe.py [--quick] [--out FILE]   (default FILE: profiles/cut_study_probe.txt)
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

from gnn_fpga_amd import _lib, count_layer_transitions, study_segment_cuts, synth  # noqa: E402

PAIRS = np.stack([np.arange(9), np.arange(1, 10)], axis=1).astype(np.int32)
# the edges a user would scan the builder's default cuts (0.001, 200) with: 24 x 16 cells
SLOPE_EDGES = np.concatenate([np.linspace(1e-4, 2e-3, 20), [3e-3, 5e-3, 1e-2]])
Z0_EDGES = np.concatenate([np.linspace(25.0, 300.0, 12), [400.0, 600.0, 1000.0]])
CUTS = (0.001, 0.001, 200.0)


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def kernel_ms(fn, name):
    with _lib.profile(256) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(ms for k, ms in prof.records if k == name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="few repetitions, nothing written")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cut_study_probe.txt"))
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("cut study probe on %s; %d x %d histogram cells per layer pair and class, 9 adjacent layer pairs"
        % (torch.cuda.get_device_name(0), SLOPE_EDGES.shape[0] + 1, Z0_EDGES.shape[0] + 1))
    shapes = (("one c3-shaped event (barrel_event(1000, 0, seed=11))", (1000, 0, 1, 11), 8, 50),
              ("one c3-shaped event (barrel_event(1000, 0, seed=11))", (1000, 0, 1, 11), 1, 50),
              ("256 c3-shaped events (barrel_event(1000, 0, n_events=256, seed=12))", (1000, 0, 256, 12), 8, 10),
              ("one mu200-sized event (barrel_event(1400, 1000, seed=13))", (1400, 1000, 1, 13), 1, 20))
    for what, (nt, nn, ne, seed), S, reps in shapes:
        if args.quick:
            reps = 3
        cols = synth.barrel_event(nt, nn, n_events=ne, seed=seed)
        r, phi, z, layer, pid = (torch.from_numpy(c).cuda() for c in cols[:5])
        ep = torch.from_numpy(cols.event_ptr).cuda()

        def study():
            return study_segment_cuts(r, phi, z, layer, PAIRS, pid, event_ptr=cols.event_ptr, n_phi_sectors=S,
                                      phi_slope_edges=SLOPE_EDGES, z0_edges=Z0_EDGES)

        def sizes():
            return _lib.graph_build_sizes(r, phi, z, layer, ep, PAIRS, 10, S, CUTS)

        def census():
            return count_layer_transitions(r, layer, pid, event_ptr=cols.event_ptr, n_layers=10)

        for _ in range(3):
            s, sz, t = study(), sizes()[1], census()
        kept = s.kept(CUTS[0], CUTS[2])
        assert int(kept.sum()) == sz.n_segments, (int(kept.sum()), sz.n_segments)
        ms_study, ms_sizes, ms_census = (median_ms(f, reps) for f in (study, sizes, census))
        k_study, k_sizes = kernel_ms(study, "k_cs_pairs"), kernel_ms(sizes, "k_gb_count")
        far = int(s.counts[:, :, -1, -1].sum())
        n_pairs = int(s.counts.sum())
        say("%s, %d sector(s): %d hits, %d pairs (%d true; %.1f %% in the last-by-last cell), %d kept at the default "
            "cuts" % (what, S, cols.r.shape[0], n_pairs, int(s.counts[:, 1].sum()), 100.0 * far / max(n_pairs, 1),
                      sz.n_segments))
        say("  study %.3f ms (k_cs_pairs %.3f ms); gnn_graph_build_sizes %.3f ms (k_gb_count %.3f ms); census %.3f ms, "
            "%d transitions" % (ms_study, k_study, ms_sizes, k_sizes, ms_census, int(t.sum())))
    ref = os.path.join(REPO, "tests", "golden", "cut_study", "reference_time.json")
    if os.path.exists(ref):
        with open(ref) as f:
            rec = json.load(f)
        say("reference notebook cells on a host CPU, the one c3-shaped event with one sector (recorded by "
            "gen_cut_study_golden.py --time): all-pairs loop and binning %.3f s, census %.3f s"
            % (rec["study_seconds"], rec["census_seconds"]))
    say("not measured: counters of the LDS atomics (bank conflicts), other edge counts, real TrackML events")
    if not args.quick:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
