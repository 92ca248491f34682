"""The two routes of the fixed-point forward against each other on the GPU: "events", one launch with a workgroup per
graph (csrc/fixed_events.hip), and "per_module", one kernel per reference module (csrc/fixed_point.hip: 15 launches at
three iterations) - through `quantize_model(...)(batch)`, as a user calls them, with `use_events` switched.

Per point and format: the two routes' outputs are compared bit for bit first; then ROUNDS rounds, the routes alternating
inside every round, of REPS calls each between two HIP events after WARM warm-up calls.  A figure is the median over the
rounds of a round's median call time; "spread" is the largest minus the smallest round median of that route - what a
difference between the routes has to be judged against.  Then a 12-format `scan_precision` over 8 batches of 64 muon
graphs, end to end: a host clock around the scan and a final synchronise, the routes alternating, SCANS times each.
The kernel's registers, LDS and occupancy come from build/fixed_events.remarks of the very build that ran.

usage: python tools/fixed_events_probe.py [--out FILE]
"""
import argparse
import os
import re
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from gnn_fpga_amd import FixedPointFormat, HitGraphBatch, _lib, quantize_model, scan_precision, synth  # noqa: E402
from gnn_fpga_amd.model import SegmentClassifier  # noqa: E402

WARM, REPS, ROUNDS, SCANS = 10, 30, 5, 3
FORMATS = (FixedPointFormat(16, 6, "trn", "wrap", 10), FixedPointFormat(24, 8, "trn", "wrap", 12))


def points():
    muon = [synth.muon_graph(s) for s in range(1024)]
    for D in (8, 16):
        for n in (1, 64, 512, 1024):
            yield "%d muon graphs" % n, muon[:n], 11, D, 3
    yield "32 toy graphs", [synth.toy2d_graph(s) for s in range(32)], 2, 32, 10
    yield "256 x layered(150, 1000)", [synth.layered_graph(150, 1000, 3, seed=s) for s in range(256)], 3, 8, 3


def model_of(F, D, T):
    torch.manual_seed(0)
    return SegmentClassifier(input_dim=F, hidden_dim=D, n_iters=T).cuda().eval()


def round_median(fn):
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def alternate(fns):
    """{route: (median of the round medians, their spread)} in ms."""
    for fn in fns.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            rounds[k].append(round_median(fn))
    return {k: (float(np.median(v)), max(v) - min(v)) for k, v in rounds.items()}


def resources(F, D):
    path = os.path.join(REPO, "build", "fixed_events.remarks")
    if not os.path.exists(path):
        return "no build remarks"
    for blk in open(path).read().split("Function Name: ")[1:]:
        if re.match(r"\S*?k_fx_eventILi%dELi%dE" % (F, D), blk):
            get = lambda name: re.search(re.escape(name) + r": (\d+)", blk).group(1)    # noqa: E731
            return "%s VGPRs, %s SGPRs, scratch %s, %s waves/SIMD by registers" % (
                get("VGPRs"), get("TotalSGPRs"), get("ScratchSize [bytes/lane]"), get("Occupancy [waves/SIMD]"))
    return "not in the remarks"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on a GPU; there is nothing to measure without one"
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    out("fixed_events_probe: %s; %d warm-up calls, %d rounds x %d calls per route, routes alternating (HIP events, ms)"
        % (torch.cuda.get_device_name(0), WARM, ROUNDS, REPS))
    out("%-26s %-8s %-12s %9s %20s %20s %7s" % ("point", "shape", "format", "LDS/WG", "events median spread",
                                               "per_module med spread", "ratio"))
    for name, graphs, F, D, T in points():
        batch = HitGraphBatch.from_graphs(graphs).to("cuda")
        lay = batch.event_layout()
        model = model_of(F, D, T)
        for f in FORMATS:
            qe, qp = quantize_model(model, f), quantize_model(model, f)
            qp.use_events = False
            oe, op = qe(batch), qp(batch)
            assert (qe.last_route, qp.last_route) == ("events", "per_module"), (name, qe.last_route, qp.last_route)
            assert torch.equal(oe.raw, op.raw) and torch.equal(oe.counts, op.counts) and torch.equal(oe.scores, op.scores)
            t = alternate({"events": lambda: qe(batch), "per_module": lambda: qp(batch)})
            lds = _lib.fxev_lds_bytes(F, D, f.table_bits, lay.max_hits, lay.max_segments)
            out("%-26s (%2d,%2d) (%2d,%d,tb%2d) %6.1f KB %11.4f %8.4f %11.4f %8.4f %6.2fx"
                % (name, F, D, f.total_bits, f.int_bits, f.table_bits, lds / 1024.0, t["events"][0], t["events"][1],
                   t["per_module"][0], t["per_module"][1], t["per_module"][0] / t["events"][0]))
    for F, D in ((11, 8), (11, 16), (2, 32), (3, 8)):
        out("k_fx_event<%d, %d>: %s" % (F, D, resources(F, D)))

    # the workload fixed point exists for: a scan over formats on trigger-size batches, end to end
    model = model_of(11, 8, 3)
    items = []
    for i in range(8):
        b = HitGraphBatch.from_graphs([synth.muon_graph(64 * i + s) for s in range(64)]).to("cuda")
        items.append((b, b.y))
    formats = [FixedPointFormat(W, I, "trn", "wrap", 10) for W in (8, 12, 16, 24) for I in (2, 4, 6)]
    secs = {True: [], False: []}
    rows = {}
    for rep in range(SCANS + 1):            # (the first pair warms up)
        for use in (True, False):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows[use] = scan_precision(model, items, formats, use_events=use)
            torch.cuda.synchronize()
            if rep:
                secs[use].append(time.perf_counter() - t0)
    for re_, rp in zip(rows[True], rows[False]):
        assert np.array_equal(re_["overflows"], rp["overflows"]) and re_["auc"] == rp["auc"] and rp["events_overflowed"] is None
    out("scan_precision, 12 formats x 8 batches of 64 muon graphs at (11, 8, T 3), host clock, %d scans per route:" % SCANS)
    for use, label in ((True, "events"), (False, "per_module")):
        out("  %-10s median %8.2f ms, min %8.2f, max %8.2f" % (label, 1e3 * np.median(secs[use]), 1e3 * min(secs[use]),
                                                             1e3 * max(secs[use])))
    out("  events that overflow per format (of 512): %s" % [r["events_overflowed"] for r in rows[True]])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
