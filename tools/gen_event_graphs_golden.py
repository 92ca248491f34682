"""Fixtures for the full-event graph builder (tests/golden/event_graphs/*.npz), made by RUNNING the reference's own
graph preparation: cells 5, 7, 8, 16, 17 and 18 (and 24 for the batch case) of gnn/MPNN_Seg_ACTS_fullEvents.ipynb,
read from the checkout given with --reference and executed in one namespace.  Nothing of the reference is copied
into this repository.

Adaptations, each stated:
* cell 5: under pandas 2.3 `groupby([...], as_index=False).r.idxmin()` is a DataFrame and `hits.loc[<DataFrame>]`
  raises "Cannot index with multidimensional key"; the `r` column of that result is taken (`.r.idxmin().r`);
* IPython magics (`%%time`) are dropped;
* cell 13 reads hit files through a process pool: `select_hits` is called on the whole frame instead (its groupby
  carries evtid, so the result is the concatenation cell 13 makes);
* cell 17's three occupancy bounds are replaced in its text by the case's (a case without a filter takes -1 and two
  bounds no event reaches), and the "thresholds" case gives construct_graph its two cuts as defaults, because cell
  18 calls it without them.

Inputs are seeded synthetic ACTS-like columns (gnn-fpga_amd/synth.py acts_events) plus hand-placed rows where a case
needs them.  Each file stores the builder's inputs (the raw columns and event_ptr), the cuts and bounds, and the
reference's result: X (cell 8's float64 X cast to float32, the cast merge_samples makes), the segment endpoints read
off Ri / Ro (`np.where(R.T)[1]`, local to the event), y, hit_ptr / seg_ptr and the event ids; the notebook case
also stores merge_samples' padded batch of the first four graphs, Ri / Ro in index form (-1: an empty column).  The
generator asserts the dtypes the specification relies on.  Files are written with fixed zip timestamps, so a rerun
reproduces them bit for bit.

--time runs cell 8 on one 5 000-hit event and writes reference_time.json beside the fixtures.

usage: python tools/gen_event_graphs_golden.py [--reference DIR] [--time]
"""
import argparse
import contextlib
import io
import json
import os
import re
import sys
import time
import zipfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from gnn_fpga_amd import synth  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "event_graphs")
CELLS = {5: "def select_hits", 7: "def calc_dphi", 8: "def construct_graph", 16: "evtids = ", 17: "n_nodes_min = ",
         18: "construct_graph(evt_hits", 24: "def merge_samples"}
NO_FILTER = (-1, 10 ** 9, 10 ** 9)
F32 = np.float32


def load_cells(ref_dir):
    with open(os.path.join(ref_dir, "gnn", "MPNN_Seg_ACTS_fullEvents.ipynb")) as f:
        nb = json.load(f)
    src = {}
    for i, mark in CELLS.items():
        text = "".join(nb["cells"][i]["source"])
        assert mark in text, "cell %d changed: %r is not in it" % (i, mark)
        src[i] = "\n".join(ln for ln in text.split("\n") if not ln.lstrip().startswith("%"))
    old = ".r.idxmin()\n"
    assert src[5].count(old) == 1, "cell 5 changed: the pandas adaptation no longer applies"
    src[5] = src[5].replace(old, ".r.idxmin().r\n")
    return src


def frame_of(cols):
    import pandas as pd
    evtid = np.repeat(np.arange(cols.event_ptr.shape[0] - 1, dtype=np.int64), np.diff(cols.event_ptr))
    return pd.DataFrame({"evtid": evtid, "barcode": cols.barcode.astype(np.int64), "volid": cols.volid.astype(np.int64),
                         "layid": cols.layid.astype(np.int64), "r": cols.r.astype(F32), "phi": cols.phi.astype(F32),
                         "z": cols.z.astype(F32)})


def run_reference(src, frame, cuts, bounds):
    """Cells 5, 7, 8, 16-18 on `frame`: the namespace after cell 18."""
    import pandas as pd
    ns = {"np": np, "pd": pd}
    for i in (5, 7, 8):
        exec(src[i], ns)
    hits = ns["select_hits"](frame)
    assert hits.phi.dtype == hits.z.dtype == hits.r.dtype == np.float32 and hits.layer.dtype == np.int8
    ns["hits"] = hits
    if cuts is not None:
        ns["construct_graph"].__defaults__ = cuts
    with contextlib.redirect_stdout(io.StringIO()):       # (cell 16 prints the number of events)
        exec(src[16], ns)
    c17 = src[17]
    for name, v in zip(("n_nodes_min", "n_nodes_max", "n_edges_max"), NO_FILTER if bounds is None else bounds):
        c17, k = re.subn(r"^%s = \d+$" % name, "%s = %d" % (name, v), c17, flags=re.M)
        assert k == 1, "cell 17 changed: %s" % name
    exec(c17, ns)
    exec(src[18], ns)
    return ns


def reference_arrays(ns, bounds):
    """The stored form of cell 18's lists, and the kept events' ids (cell 18 keeps none: its test is repeated)."""
    Xs, Ris, Ros, ys = ns["all_X"], ns["all_Ri"], ns["all_Ro"], ns["all_y"]
    hits, evtids = ns["hits"], ns["evtids"]
    lo, hi, emax = NO_FILTER if bounds is None else bounds
    sizes = hits.groupby("evtid").size()
    events = []
    k = 0
    for e in evtids:                                      # which events cell 18 kept: by their sizes, in its order
        n = int(sizes[e])
        if k < len(Xs) and Xs[k].shape[0] == n and n > lo and n < hi and ys[k].shape[0] < emax:
            events.append(int(e))
            k += 1
    assert k == len(Xs), "could not attribute cell 18's graphs to events"
    for X, y in zip(Xs, ys):
        assert X.dtype == np.float64 and y.dtype == bool, (X.dtype, y.dtype)
    src = [np.where(Ro.T)[1].astype(np.int32) for Ro in Ros]
    dst = [np.where(Ri.T)[1].astype(np.int32) for Ri in Ris]
    for a, b, y in zip(src, dst, ys):
        assert a.shape == b.shape == y.shape          # every column of Ri and Ro holds exactly one 1
    cat = (lambda v, dt, shape=(0,): np.concatenate(v).astype(dt) if v else np.zeros(shape, dt))
    return {"X": cat(Xs, np.float32, (0, 3)), "src": cat(src, np.int32), "dst": cat(dst, np.int32),
            "y": cat(ys, np.uint8), "hit_ptr": np.cumsum([0] + [X.shape[0] for X in Xs]).astype(np.int64),
            "seg_ptr": np.cumsum([0] + [y.shape[0] for y in ys]).astype(np.int64),
            "event_index": np.asarray(events, np.int64)}


def batch_arrays(src, ns, n):
    """merge_samples (cell 24) over the first n graphs, Ri / Ro in index form."""
    exec(src[24], ns)
    bX, bRi, bRo, by = ns["merge_samples"](ns["all_X"][:n], ns["all_Ri"][:n], ns["all_Ro"][:n], ns["all_y"][:n])
    assert bX.dtype == np.float32 and by.dtype == np.uint8

    def ends(R):
        out = np.full((R.shape[0], R.shape[2]), -1, np.int32)
        for g in range(R.shape[0]):
            col, hit = np.where(R[g].T)
            assert np.array_equal(col, np.arange(col.shape[0]))       # the real columns come first, one hit each
            out[g, col] = hit
        return out
    return {"batch_X": bX, "batch_src": ends(bRo), "batch_dst": ends(bRi), "batch_y": by}


def with_rows(cols, event, rows):
    """`cols` with hand-placed rows (r, phi, z, volid, layid, barcode) appended to `event`."""
    at = int(cols.event_ptr[event + 1])
    new = {k: np.array([row[i] for row in rows]) for i, k in enumerate(("r", "phi", "z", "volid", "layid", "barcode"))}
    ep = cols.event_ptr.copy()
    ep[event + 1:] += len(rows)
    return synth.ActsColumns(*[np.insert(getattr(cols, k), at, new[k].astype(getattr(cols, k).dtype))
                               for k in ("r", "phi", "z", "volid", "layid", "barcode")], ep)


def cases():
    """(name, columns, (dphi_max, dz_max) or None, (n_nodes_min, n_nodes_max, n_edges_max) or None)"""
    A = synth.acts_events
    yield "duplicates", A(2, 14, 30, seed=1, dup=0.4, dup_equal=0.6, missing=0.0), None, None
    yield "missing_layers", A(2, 16, 20, seed=2, missing=0.6, dup=0.0), None, None
    # an odd and a zero layid: (8, 9) -> 3, (8, 7) -> 2, (17, 1) -> 7, (13, 3) -> 4, (8, 0) -> -1: a layer -1 hit starts
    # segments to layer 0
    c = A(2, 10, 20, seed=3)
    odd = [(170.0, 0.3, 10.0, 8, 9, 901), (118.0, 0.31, 8.0, 8, 7, 901), (820.0, -1.0, 5.0, 17, 1, 902),
           (262.0, -1.01, 3.0, 13, 3, 902), (20.0, 0.29, 2.0, 8, 0, 901), (21.0, -2.0, -4.0, 8, 0, 903)]
    yield "odd_zero_layid", with_rows(with_rows(c, 0, odd), 1, odd[:5]), None, None
    # non-barrel rows, and event 1 left empty by the selection
    c = A(3, 10, 15, seed=4, non_barrel=0.3)
    m = (np.arange(c.r.shape[0]) >= c.event_ptr[1]) & (np.arange(c.r.shape[0]) < c.event_ptr[2])
    yield "non_barrel_empty_event", c._replace(volid=np.where(m, 9, c.volid).astype(np.int32)), None, None
    # hits at phi near +-pi: the wrap
    w = [(BR + 0.01 * k, s * (np.pi - 0.001 * (k + 1)), 3.0 * k, v, l, 800 + k)
         for k, (BR, (v, l)) in enumerate(zip(synth.BARREL_RADII, synth.ACTS_BARREL_LAYERS)) for s in (1.0, -1.0)]
    w += [(32.0, F32(np.pi), 0.0, 8, 2, 990), (72.0, -F32(np.pi), 1.0, 8, 4, 991)]
    yield "phi_wrap", with_rows(A(2, 12, 20, seed=5), 0, w), None, None
    # thresholds: differences of exactly f32(0.7) are left out (the comparison is in float32), one ulp less is kept
    t7 = F32(0.7)
    below = np.nextafter(t7, F32(0))
    th = [(32.0, t7, 0.0, 8, 2, 701),            # A, layer 0
          (72.0, 0.0, 0.0, 8, 4, 702),           # B: dphi = f32(0.7) exactly
          (72.0, t7 - below, 0.5, 8, 4, 703),    # C: dphi = f32(0.7) - one ulp of it (exact in float32)
          (72.0, 0.5, t7, 8, 4, 704),            # D: dz = f32(0.7) exactly
          (72.0, 0.5, below, 8, 4, 705)]         # E: dz one ulp below
    yield "thresholds", with_rows(A(1, 8, 40, seed=6), 0, th), (0.7, 0.7), None
    # the filter: events fail n_nodes_max (one with exactly 340 hits), n_nodes_min and, alone, n_edges_max (one with
    # exactly 1390 segments): all three tests are strict
    yield "filter", A(8, (2, 40), (5, 120), seed=17), None, (80, 340, 1390)
    yield "notebook", A(8, (4, 30), (10, 60), seed=8), None, (50, 500, 1000)


def write_npz(path, arrays):
    """np.savez_compressed with a fixed zip timestamp (reproducible bytes)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def check_case(name, cols, ref, ns, cuts, bounds):
    """What each case is named for, asserted on the reference's own result."""
    hits = ns["hits"]
    E = cols.event_ptr.shape[0] - 1
    if name == "duplicates":
        k = np.stack([np.repeat(np.arange(E), np.diff(cols.event_ptr)), cols.barcode, cols.volid, cols.layid, cols.r.view(np.int32)])
        assert np.unique(k, axis=1).shape[1] < k.shape[1], "no duplicate with exactly equal r"
    if name == "odd_zero_layid":
        assert hits.layer.min() == -1 and np.any(ref["y"] == 1)
    if name == "non_barrel_empty_event":
        assert ref["event_index"].tolist() == [0, 2]
    if name == "phi_wrap":
        assert np.abs(cols.phi).max() > 3.14
    if name == "thresholds":
        h = hits[hits.evtid == 0].reset_index(drop=True)
        pos = {int(b): i for i, b in enumerate(h.barcode.values)}
        seg = set(zip(ref["src"].tolist(), ref["dst"].tolist()))
        assert (pos[701], pos[702]) not in seg and (pos[701], pos[704]) not in seg, "an exact f32(0.7) was kept"
        assert (pos[701], pos[703]) in seg and (pos[701], pos[705]) in seg, "one ulp below f32(0.7) was left out"
    if bounds is not None:
        sizes = hits.groupby("evtid").size().values
        lo, hi, emax = bounds
        assert len(ref["event_index"]) > 0
        if name == "filter":
            assert np.any(sizes <= lo) and np.any(sizes >= hi), "no event fails each node bound"
            assert np.any(sizes == hi), "no event sits exactly on a bound"
            passing = int(np.sum((sizes > lo) & (sizes < hi)))
            assert passing > len(ref["event_index"]), "no event fails the edge bound alone"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.path.join(os.path.dirname(REPO), "reference"),
                    help="the reference checkout (its gnn/MPNN_Seg_ACTS_fullEvents.ipynb is read)")
    ap.add_argument("--time", action="store_true", help="also time cell 8 on one 5 000-hit event")
    args = ap.parse_args()
    src = load_cells(args.reference)
    os.makedirs(OUT, exist_ok=True)
    total = 0
    for name, cols, cuts, bounds in cases():
        ns = run_reference(src, frame_of(cols), cuts, bounds)
        ref = reference_arrays(ns, bounds)
        check_case(name, cols, ref, ns, cuts, bounds)
        arrays = {k: getattr(cols, k) for k in cols._fields}
        arrays.update({"ref_" + k: v for k, v in ref.items()})
        arrays["dphi_max"] = np.float64(np.pi / 4 if cuts is None else cuts[0])
        arrays["dz_max"] = np.float64(300.0 if cuts is None else cuts[1])
        arrays["bounds"] = np.asarray(bounds if bounds is not None else [], np.int64)
        arrays["dtypes"] = np.array(json.dumps({"phi": str(ns["hits"].phi.dtype), "z": str(ns["hits"].z.dtype),
                                                "layer": str(ns["hits"].layer.dtype),
                                                "features": str(ns["all_X"][0].dtype)}, sort_keys=True))
        if name == "notebook":
            assert len(ns["all_X"]) >= 4
            arrays.update(batch_arrays(src, ns, 4))
        path = os.path.join(OUT, name + ".npz")
        write_npz(path, arrays)
        total += os.path.getsize(path)
        print("%-24s %5d rows %5d hits %3d graphs %6d segments %7d bytes" % (
            name, cols.r.shape[0], ref["X"].shape[0], len(ref["event_index"]), ref["src"].shape[0],
            os.path.getsize(path)))
    print("total %d bytes" % total)
    if args.time:
        import pandas as pd
        cols = synth.acts_events(1, 380, 1350, seed=11)
        ns = {"np": np, "pd": pd}
        for i in (5, 7, 8):
            exec(src[i], ns)
        hits = ns["select_hits"](frame_of(cols))
        t0 = time.perf_counter()
        X, Ri, Ro, y = ns["construct_graph"](hits, ["r", "phi", "z"], np.array([1000., np.pi, 1000.]))
        dt = time.perf_counter() - t0
        rec = {"what": "reference cell 8 (construct_graph, default cuts) on the host CPU, one synthetic event: "
                       "synth.acts_events(1, 380, 1350, seed=11) after cell 5's selection",
               "rows": int(cols.r.shape[0]), "hits": int(X.shape[0]), "segments": int(y.shape[0]),
               "seconds": round(dt, 2)}
        with open(os.path.join(OUT, "reference_time.json"), "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        print(rec)


if __name__ == "__main__":
    main()
