"""Fixtures for the toy graph builders (tests/golden/toy_graphs/*.npz), made by RUNNING the reference's data cells.

Segment cases (seg_*.npz): cells 3, 4, 7-17 and 24 of gnn/GCN_Seg_Toy2D.ipynb are read from the notebook and executed
as they are, cell 12's Python triple loop included, with det_r, n_events and n_tracks set after cell 7 and numpy's seed
fixed (and argsort pinned to the stable sort the notebooks' numpy did on arrays this small: see _Np).  The edge case
feeds hand-made entry and exit points to the notebook's own gen_tracks through a thin stand-in
for `np` whose random.uniform hands them out.

Hit cases (hits_*.npz): calc_adjacency, norm_adjacency and kwnorm_adjacency of gnn/GCN_Toy2D.ipynb's cell 4 and the
whole of cell 17 are executed on hits taken from the SEGMENT notebook's generate_data, widened to fp64.  The hit
notebook's own generate_data indexes an array with a list of arrays (`tracks[[idx0, idx, idx2]]`), which today's numpy
refuses, so it cannot run; its cell 4 also says np.int, which the stand-in for `np` maps to the builtin (np.float
likewise).  The edge case's hits are hand-made fp64 lines with exact and nearly exact intercepts.

Nothing of either notebook is written into the repository: the fixtures hold inputs and results only.

Per segment case: hit_x float32, hit_y, det_r, sigma, X, y, and the adjacency in coordinate form over its STRUCTURAL
entries (A_batch, A_rows, A_cols where cell 12 wrote a 1; A_vals = seg_A there, float32, zeros included; A_shape).
Per hit case: hit_x float64, hit_y, det_r, seed_size, X, y0, per norm in (none, row, kw) the finite non-zero entries
(<norm>_batch, _rows, _cols, _vals, float32 as the notebook's functions return them), and iso_batch / iso_rows: the
rows that norm_adjacency fills with NaN (1 / 0), which the builders and synth leave zero.

The tool fails unless the edge cases hold: a tie within a layer; hit-pair decisions whose x0 or xn lies within 4 ulps
of 0 and of 1, on both sides of each (for 0, where x0 = x - slope r cancels, the ulp is that of x); an isolated hit;
segment entries that are normal, sub-normal and exactly zero.  Files are written with fixed zip timestamps: a rerun
reproduces them byte for byte.  `--time` also times the notebooks' cells per event at their own shapes into
reference_time.json (which, being a measurement, is not reproducible).

usage: python tools/gen_toy_graphs_golden.py [--reference DIR] [--time]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "toy_graphs")

from gen_gcn_golden import _NoPlot, _cells, write_npz  # noqa: E402

DET_R = (0, 1, 2, 3, 5, 7, 9, 11, 13, 15)
NB1 = float(np.nextafter(np.float32(1), np.float32(0)))        # the largest float32 below 1
TINY = 1e-30
FLT_MIN = float(np.finfo(np.float32).tiny)

# (name, det_r, n_tracks, n_events)
CASES = [("l10_t5", DET_R, 5, 4), ("l10_t4", DET_R, 4, 3), ("l3_t2", (0, 1, 3), 2, 4), ("l2_t1", (0, 2), 1, 3)]

# the segment edge case: (xin, xout) per track, five tracks per event
SEG_EDGE = [
    # in at 0 / just below 1 / tiny; a flat track at 0.5 that 0.75 -> 0 crosses exactly on the layer at r = 5
    [(0.0, NB1), (NB1, 0.0), (TINY, 0.5), (0.5, 0.5), (0.75, 0.0)],
    # two identical tracks (a tie on every layer); out at tiny and just below 1
    [(0.3, 0.7), (0.3, 0.7), (TINY, NB1), (NB1, TINY), (0.6, 0.6)],
    # steep and flat tracks side by side: slope differences from 0 to beyond the kernel's underflow
    [(0.0, 0.0), (0.05, 0.95), (0.95, 0.05), (0.5, 0.52), (0.4, 0.2)],
    [(0.11, 0.13), (0.12, 0.125), (0.9, 0.1), (0.1, 0.9), (NB1, NB1)],
]


class _Np:
    """Stands in for `np` in the notebooks' cells: numpy, with np.int / np.float as the builtins, argsort pinned to a
    stable sort and, when `uniform` holds arrays, a random.uniform that hands them out in turn.

    The notebooks' numpy sorted arrays of 4 or 5 elements by insertion (equal positions keep the lower track first);
    today's numpy hands float arrays to a vectorised sort on the CPUs that have one, and the order of equal positions
    then depends on the machine the tool runs on.  kind="stable" is what the notebooks got, on every machine."""

    class _Random:
        def __init__(self, queue):
            self.queue = queue

        def uniform(self, *a, **k):
            if self.queue:
                v = self.queue.pop(0)
                assert k.get("size") == v.shape[0]
                return v
            return np.random.uniform(*a, **k)

        def __getattr__(self, name):
            return getattr(np.random, name)

    int, float = int, float

    def __init__(self, uniform=None):
        self.random = _Np._Random(list(uniform) if uniform is not None else [])

    @staticmethod
    def argsort(a, axis=-1):
        return np.argsort(a, axis=axis, kind="stable")

    def __getattr__(self, name):
        return getattr(np, name)


def run_segment_cells(ref_dir, det_r, n_tracks, n_events, seed, ends=None):
    """The segment notebook's data cells: (namespace, seconds spent in cells 9-17 and 24)."""
    src = _cells(ref_dir, "GCN_Seg_Toy2D.ipynb")
    queue = None
    if ends is not None:
        ends = np.asarray(ends, dtype=np.float64)                            # [E, T, 2], as uniform() returns them
        queue = [ends[:, t, k] for t in range(ends.shape[1]) for k in range(2)]
    ns = {"np": _Np(queue), "plt": _NoPlot(), "print": lambda *a, **k: None}
    np.random.seed(seed)
    for c in (3, 4, 7):
        exec(compile(src[c], "GCN_Seg_Toy2D.ipynb cell %d" % c, "exec"), ns)
    ns["det_r"] = np.array(det_r, dtype=np.float32)
    ns["n_det_layers"], ns["n_events"], ns["n_tracks"] = len(det_r), n_events, n_tracks
    exec(compile(src[8], "GCN_Seg_Toy2D.ipynb cell 8", "exec"), ns)
    t0 = time.perf_counter()
    for c in (9, 10, 11, 12, 13, 14, 15, 16, 17, 24):
        exec(compile(src[c], "GCN_Seg_Toy2D.ipynb cell %d" % c, "exec"), ns)
    return ns, time.perf_counter() - t0


def segment_case(ns, det_r):
    A = ns["seg_A"].astype(np.float32)
    bi, ri, ci = np.nonzero(ns["seg_adj"])
    assert ns["hit_x"].dtype == np.float32 and ns["seg_slope"].dtype == np.float32
    assert not np.any(A[ns["seg_adj"] == 0])
    return {"hit_x": ns["hit_x"], "hit_y": ns["hit_y"].astype(np.int64), "det_r": np.array(det_r, dtype=np.float64),
            "sigma": np.float64(ns["sigma"]), "X": ns["seg_X"].astype(np.float32), "y": ns["seg_y"].astype(np.float32),
            "A_batch": bi.astype(np.int32), "A_rows": ri.astype(np.int32), "A_cols": ci.astype(np.int32),
            "A_vals": A[bi, ri, ci], "A_shape": np.array(A.shape, np.int64)}


def run_hit_cells(ref_dir, hit_x, hit_y, det_r, seed_size=3):
    """Cell 4's adjacency functions and cell 17 of the hit notebook on given hits: (fixture arrays, seconds in cell 17)."""
    src = _cells(ref_dir, "GCN_Toy2D.ipynb")
    ns = {"np": _Np()}
    exec(compile(src[4], "GCN_Toy2D.ipynb cell 4", "exec"), ns)
    det = np.array(det_r, dtype=np.float64)
    E, L = hit_x.shape[0], det.shape[0]
    T = hit_x.shape[1] // L
    shape = (E, L, T)
    ns["x"] = np.asarray(hit_x, dtype=np.float64)
    ns["y"] = np.asarray(hit_y)
    ns["r"] = np.broadcast_to(det[None, :, None], shape).reshape(E, -1)
    ns["l"] = np.broadcast_to(np.arange(L)[None, :, None], shape).reshape(E, -1)
    ns["seed_size"] = seed_size
    with np.errstate(divide="ignore", invalid="ignore"):
        t0 = time.perf_counter()
        exec(compile(src[17], "GCN_Toy2D.ipynb cell 17", "exec"), ns)
        dt = time.perf_counter() - t0
        kw = ns["kwnorm_adjacency"](ns["adj"])
    row = ns["A"]
    assert row.dtype == np.float32 and kw.dtype == np.float32
    out = {"hit_x": ns["x"], "hit_y": ns["y"].astype(np.int64), "det_r": det, "seed_size": np.int64(seed_size),
           "X": ns["X"].astype(np.float32), "y0": ns["y0"].astype(np.float32), "A_shape": np.array(row.shape, np.int64)}
    bad = ~np.isfinite(row).all(axis=2)
    out["iso_batch"], out["iso_rows"] = (v.astype(np.int32) for v in np.nonzero(bad))
    row = np.where(bad[:, :, None], np.float32(0), row)
    assert np.array_equal(bad, ns["adj"].sum(axis=1) == 0)
    for name, a in (("none", ns["adj"].astype(np.float32)), ("row", row), ("kw", kw)):
        bi, ri, ci = np.nonzero(a)
        out[name + "_batch"], out[name + "_rows"], out[name + "_cols"] = (v.astype(np.int32) for v in (bi, ri, ci))
        out[name + "_vals"] = a[bi, ri, ci]
    return out, dt


def sort_hits(tracks):
    """The segment notebook's sort (generate_data, cell 3) of [E, L, T] positions: (hit_x, hit_y) [E, L T]."""
    y = np.argsort(tracks, axis=-1, kind="stable")
    x = np.sort(tracks, axis=-1)
    return x.reshape(x.shape[0], -1), y.reshape(x.shape[0], -1)


def hit_edge_tracks():
    """Hand-made fp64 lines x(r) = xin + (xout - xin) r / 15, four per event: intercepts at exactly 0 and 1, one ulp
    inside them and tiny, so that the line through two hits of a track enters or leaves within rounding of a border."""
    rng = np.random.default_rng(20260)
    det = np.array(DET_R, dtype=np.float64)
    below1 = np.nextafter(1.0, 0.0)
    special = [0.0, 1.0, below1, 1e-300, 2.0 ** -60]
    events = []
    for e in range(8):
        xin = rng.uniform(0.05, 0.95, size=4)
        xout = rng.uniform(0.05, 0.95, size=4)
        for t in range(3):                                                   # three tracks touch a border
            which, v = rng.integers(0, 2), special[rng.integers(0, len(special))]
            if which:
                xout[t] = v
            else:
                xin[t] = v
        events.append(xin[:, None] + ((xout - xin) / 15.0)[:, None] * det[None, :])
    ev = np.stack(events)                                                    # [E, T, L]
    ev[0, 3] = 0.5                                                           # a flat track ...
    ev[0, 2] = 0.75 - 0.05 * det                                             # ... crossed exactly at r = 5
    assert ev[0, 2, 4] == 0.5
    return ev.transpose(0, 2, 1)


def border_decisions(hit_x, det_r):
    """How many adjacent-layer hit pairs have x0 / xn within 4 ulps of 0 / 1, by side: {(quantity, border, side): n}."""
    det = np.array(det_r, dtype=np.float64)
    T = hit_x.shape[1] // det.shape[0]
    r = np.repeat(det, T)
    lay = np.repeat(np.arange(det.shape[0]), T)
    x = hit_x
    near = np.abs(lay[None, :] - lay[:, None]) == 1
    dr = np.where(near, r[None, :] - r[:, None], 1.0)
    slope = (x[:, None, :] - x[:, :, None]) / dr
    xj, rj = x[:, None, :], r[None, None, :]
    out = {}
    for name, v, scale in (("x0", xj - slope * rj, np.maximum(np.abs(xj), np.abs(slope * rj))),
                           ("xn", xj + slope * (det[-1] - rj), np.maximum(np.abs(xj), np.abs(slope * (det[-1] - rj))))):
        for border in (0.0, 1.0):
            ulp = np.spacing(np.maximum(scale, border))
            close = near[None] & (np.abs(v - border) <= 4 * ulp)
            out[(name, border, "below")] = int((close & (v < border)).sum())
            out[(name, border, "at")] = int((close & (v == border)).sum())
            out[(name, border, "above")] = int((close & (v > border)).sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("GNN_REFERENCE", "../reference"))
    ap.add_argument("--time", action="store_true")
    a = ap.parse_args()
    if not os.path.isdir(os.path.join(a.reference, "gnn")):
        sys.exit("reference checkout not found at %s" % a.reference)
    os.makedirs(OUT, exist_ok=True)
    files = {}
    for i, (name, det_r, T, E) in enumerate(CASES):
        ns, _ = run_segment_cells(a.reference, det_r, T, E, seed=100 + i)
        files["seg_" + name] = segment_case(ns, det_r)
        files["hits_" + name], _ = run_hit_cells(a.reference, ns["hit_x"].astype(np.float64), ns["hit_y"], det_r)
    ns, _ = run_segment_cells(a.reference, DET_R, 5, len(SEG_EDGE), seed=0, ends=SEG_EDGE)
    seg_edge = files["seg_edge"] = segment_case(ns, DET_R)
    hx, hy = sort_hits(hit_edge_tracks())
    hit_edge = files["hits_edge"] = run_hit_cells(a.reference, hx, hy, DET_R)[0]

    # what the edge cases must hold
    x = seg_edge["hit_x"].reshape(len(SEG_EDGE), len(DET_R), 5)
    if not (np.diff(x, axis=-1) == 0).any() or not (np.diff(hx.reshape(8, len(DET_R), 4), axis=-1) == 0).any():
        sys.exit("the edge cases have no tie within a layer")
    v = seg_edge["A_vals"]
    classes = {"normal": int((v >= FLT_MIN).sum()), "sub-normal": int(((v > 0) & (v < FLT_MIN)).sum()),
               "zero": int((v == 0).sum())}
    if not all(classes.values()):
        sys.exit("the segment edge case misses a class of entries: %s" % classes)
    dec = border_decisions(hx, DET_R)
    for q in ("x0", "xn"):
        for border in (0.0, 1.0):
            inside = dec[(q, border, "above" if border == 0.0 else "below")]
            outside = dec[(q, border, "at")] + dec[(q, border, "below" if border == 0.0 else "above")]
            if not inside or not outside:
                sys.exit("the hit edge case has no %s within 4 ulps of %g on both sides: %s" % (q, border, dec))
    if not hit_edge["iso_rows"].shape[0]:
        sys.exit("the hit edge case has no isolated hit")
    for name in sorted(files):
        path = os.path.join(OUT, name + ".npz")
        write_npz(path, files[name])
        print("%s: %d bytes" % (path, os.path.getsize(path)))
    print("segment edge entries: %s; isolated hits in the hit edge case: %d" % (classes, hit_edge["iso_rows"].shape[0]))
    print("hit edge decisions within 4 ulps: %s" % {"%s %g %s" % k: n for k, n in dec.items() if n})
    if a.time:
        # the notebooks' own cells per event, at their own shapes (cell 12's loop is linear in the events)
        E = 16
        ns, dt_seg = run_segment_cells(a.reference, DET_R, 5, E, seed=1)
        ns4, _ = run_segment_cells(a.reference, DET_R, 4, 256, seed=2)
        _, dt_hit = run_hit_cells(a.reference, ns4["hit_x"].astype(np.float64), ns4["hit_y"], DET_R)
        rec = {"segments_l10_t5": {"events": E, "cells": "9-17, 24", "seconds_per_event": dt_seg / E},
               "hits_l10_t4": {"events": 256, "cells": "17", "seconds_per_event": dt_hit / 256}}
        with open(os.path.join(OUT, "reference_time.json"), "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
            f.write("\n")
        print(rec)


if __name__ == "__main__":
    main()
