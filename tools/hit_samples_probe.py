"""Samples per second of build_hit_samples (csrc/hit_samples.hip, both calls and the one read-back) at the
notebook's shape and at detector scale, timed with HIP events after warm-up, beside the numpy specification's
host time on the same inputs.  Writes the table to stdout (profiles/hit_samples_probe.txt keeps one run).

usage: python tools/hit_samples_probe.py [--reps N]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnn_fpga_amd import build_hit_samples, synth  # noqa: E402

SHAPES = (("notebook: 3 events x (40 tracks + 300 noise)", 40, 300, 3),
          ("detector: 4 events x (1000 tracks + 10000 noise)", 1000, 10000, 4),
          ("detector: 16 events x (1000 tracks + 10000 noise)", 1000, 10000, 16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    print("%-52s %8s %8s %10s %12s %12s" % ("input", "hits", "samples", "device ms", "samples/s", "numpy ms"))
    for name, nt, nn_, ne in SHAPES:
        ev = synth.barrel_event(nt, nn_, n_events=ne, seed=7)
        cols = [ev.r, ev.phi, ev.z, ev.layer, ev.particle_id]
        dcols = [torch.from_numpy(c).to(dev) for c in cols]
        for _ in range(3):
            s = build_hit_samples(*dcols, event_ptr=ev.event_ptr)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            s = build_hit_samples(*dcols, event_ptr=ev.event_ptr)
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b) / args.reps
        t0 = time.perf_counter()
        h = build_hit_samples(*cols, event_ptr=ev.event_ptr)
        host_ms = 1e3 * (time.perf_counter() - t0)
        assert len(h) == len(s)
        print("%-52s %8d %8d %10.3f %12.3g %12.1f" % (name, ev.r.shape[0], len(s), ms, len(s) / ms * 1e3, host_ms))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
