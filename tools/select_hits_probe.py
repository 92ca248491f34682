"""Device hit selection (select_hits.select_hits on csrc/select_hits.hip) on detector-scale synthetic TrackML events:
the time of one event (the event tests/golden/select_hits/reference_time.json was taken at) and of 16 such events in
one call, `build_graphs`' own time on the selected hits, and raw tables to scores for one event (selection, graph
build, first forward).  Times are HIP events around the whole Python call after warm-up, so both library calls, the
read-back of the sizes and the host work between them are counted; the median of the repetitions is given, with the
smallest.  Also the distance in float32 ulps between the device's default phi (atan2f in the fill kernel) and
np.arctan2, on every fixture and on the detector-scale event: tests/test_gpu_select_hits.py takes its bound from
the largest.

--selection-only runs the one event's selection 8 times (3 warm-up + 5 timed) and nothing else: the run to put under
`rocprofv3 --kernel-trace --stats` (tools/rocpd_kernel_stats.py <db> 8 gives profiles/select_hits_kernels.txt).

usage: python tools/select_hits_probe.py [--quick] [--selection-only] [--out FILE]
(default FILE: profiles/select_hits_probe.txt)
"""
import argparse
import glob
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gnn_fpga_amd import select_hits, synth  # noqa: E402
from gnn_fpga_amd.model import SegmentClassifier  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden", "select_hits")
DETECTOR_EVENT = dict(n_tracks=10000, n_noise=20000, seed=11)       # tools/gen_select_hits_golden.py --time
TABLES = ("hits", "truth", "particles")


def event_ms(fn, reps):
    """(median, smallest) milliseconds of fn() between two HIP events."""
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


def on_dev(ev):
    return [{k: (v if k == "event_ptr" else torch.from_numpy(v).cuda()) for k, v in ev[t].items()} for t in TABLES]


def ulps(a, b):
    """Distance of two float32 arrays in units in the last place (their ordered integer keys)."""
    def key(v):
        i = np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="few repetitions and no file (for a profiler run)")
    ap.add_argument("--selection-only", action="store_true", help="only the one event's selection (for a profiler run)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "select_hits_probe.txt"))
    args = ap.parse_args()
    reps = 5 if args.quick or args.selection_only else 40
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("select_hits probe on %s" % torch.cuda.get_device_name(0))
    ev = synth.trackml_events(1, **DETECTOR_EVENT)
    dev = on_dev(ev)
    phi = torch.atan2(dev[0]["y"], dev[0]["x"])
    sel_fn = lambda: select_hits(*dev, pt_min=1.0, phi=phi)            # noqa: E731
    for _ in range(3):
        sel = sel_fn()
    med, least = event_ms(sel_fn, reps)
    say("one detector-scale event (synth.trackml_events(1, 10000, 20000, seed=11), pt_min 1.0): %d hits, %d truth rows, "
        "%d particles -> %d selected; device selection %.3f ms (smallest %.3f)"
        % (ev["hits"]["x"].shape[0], ev["truth"]["hit_id"].shape[0], ev["particles"]["px"].shape[0], len(sel), med,
           least))
    if args.selection_only:
        return
    med_nm, _ = event_ms(lambda: select_hits(*dev, pt_min=1.0, phi=phi, no_missing_hits=True), reps)
    say("  the same with no_missing_hits: %.3f ms" % med_nm)
    graphs_fn = lambda: sel.build_graphs(n_phi_sectors=8)               # noqa: E731
    for _ in range(3):
        b = graphs_fn()
    gmed, gleast = event_ms(graphs_fn, reps)
    say("  build_graphs on the selected hits (8 sectors, default cuts): %d segments in %d graphs; %.3f ms (smallest "
        "%.3f)" % (b.n_segments, b.n_graphs, gmed, gleast))
    model = SegmentClassifier(input_dim=3, hidden_dim=8, n_iters=4).cuda().eval()

    def chain():
        with torch.no_grad():
            model(sel_fn().build_graphs(n_phi_sectors=8))
    for _ in range(3):
        chain()
    cmed, cleast = event_ms(chain, reps)
    say("  raw tables to scores (selection + graph build + first forward, use_plan=%r): %.3f ms (smallest %.3f)"
        % (model.use_plan, cmed, cleast))
    ref = os.path.join(GOLD, "reference_time.json")
    if os.path.exists(ref):
        rec = json.load(open(ref))
        say("  reference select_hits on a host CPU, the same event (recorded by gen_select_hits_golden.py --time): "
            "%.3f s, %d selected" % (rec["seconds"], rec["selected"]))
    ev16 = synth.trackml_events(16, **DETECTOR_EVENT)
    dev16 = on_dev(ev16)
    fn16 = lambda: select_hits(*dev16, pt_min=1.0)                      # noqa: E731
    for _ in range(2):
        s16 = fn16()
    med16, least16 = event_ms(fn16, max(5, reps // 4))
    say("16 such events in one call (default phi): %d hits -> %d selected; device selection %.3f ms (smallest %.3f)"
        % (ev16["hits"]["x"].shape[0], len(s16), med16, least16))
    worst = 0
    for path in sorted(glob.glob(os.path.join(GOLD, "*.npz"))):
        with np.load(path) as f:
            fx = {"hits": {k[5:]: f[k] for k in f.files if k.startswith("hits_")},
                  "truth": {k[6:]: f[k] for k in f.files if k.startswith("truth_")},
                  "particles": {k[10:]: f[k] for k in f.files if k.startswith("particles_")}}
            got = select_hits(*on_dev(fx), pt_min=float(f["pt_min"]), no_missing_hits=bool(f["no_missing_hits"]))
            d = ulps(got.phi.cpu().numpy(), f["ref_phi"])
            worst = max(worst, int(d.max(initial=0)))
    d = ulps(select_hits(*dev, pt_min=1.0).phi.cpu().numpy(), np.arctan2(ev["hits"]["y"], ev["hits"]["x"])[sel.row.cpu().numpy()])
    say("default phi (atan2f in the fill kernel) against np.arctan2 in float32 ulps: the largest over the fixtures %d, "
        "over the detector-scale event %d (%d of %d hits differ)" % (worst, int(d.max()), int((d > 0).sum()), d.shape[0]))
    if not args.quick:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
