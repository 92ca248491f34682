"""Fixtures for the hit-sample builder (tests/golden/hit_samples/*.npz), made by RUNNING the reference's own sample
preparation: cells 5, 9, 10, 11, 12, 14 and 15 of gnn/MPNN_HitClassifier.ipynb, read from the checkout given with
--reference and executed in one namespace.  Nothing of the reference is copied into this repository.

Adaptations, each stated:
* cell 5: under pandas 2.3 `groupby([...], as_index=False).r.idxmin()` is a DataFrame and `hits.loc[<DataFrame>]`
  raises "Cannot index with multidimensional key"; the `r` column of that result is taken (`.r.idxmin().r`);
* IPython magics (`%%time`) are dropped;
* the non-default cases override cell 12's constants (n_det_layers, n_layer_hits, n_seed_layers) in its text and
  give select_signal_hits (cell 10 calls it with its own defaults, 5 and 10) the same two values as defaults.

Inputs are seeded synthetic ACTS-like frames (evtid, barcode, volid, layid and float32 z, r, phi as
acts.process_hits_data makes them, barrel volumes 8, 13, 17 only).  Each file stores the builder's inputs (the
frame's columns after select_hits' layer renumbering, before deduplication: r, phi, z, layer, particle_id,
event_ptr), the constants, and the reference's full_X, full_Ri, full_Ro, full_y and sig_keys.  The generator
checks the dtype of every intermediate the specification relies on, and that no sample has an exact tie among
the K + 1 smallest distances of a layer (the reference's sort is not stable there); it reports the smallest gap in
ulps.  Files are written with fixed zip timestamps, so a rerun reproduces them bit for bit.

--time measures the reference's host time per sample (cells 10-15) on one stated synthetic event and writes
reference_time.json beside the fixtures.

usage: python tools/gen_hit_samples_golden.py [--reference DIR] [--time]
"""
import argparse
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
OUT = os.path.join(REPO, "tests", "golden", "hit_samples")

CELLS = (5, 9, 10, 11, 12, 14, 15)
VIDS = (8, 13, 17)
LAYIDS = ((8, 2), (8, 4), (8, 6), (8, 8), (13, 2), (13, 4), (13, 6), (13, 8), (17, 2), (17, 4))
RADII = (32.0, 72.0, 116.0, 172.0, 260.0, 360.0, 500.0, 660.0, 820.0, 1020.0)


def load_cells(ref_dir):
    with open(os.path.join(ref_dir, "gnn", "MPNN_HitClassifier.ipynb")) as f:
        nb = json.load(f)
    src = {}
    for i in CELLS:
        text = "".join(nb["cells"][i]["source"])
        src[i] = "\n".join(ln for ln in text.split("\n") if not ln.lstrip().startswith("%"))
    old = ".r.idxmin()\n"
    assert src[5].count(old) == 1, "cell 5 changed: the pandas adaptation no longer applies"
    src[5] = src[5].replace(old, ".r.idxmin().r\n")
    return src


def run_reference(src, frame, L, K, NS):
    """Cells 5 and 9-15 on `frame`: (hits after select_hits, namespace)."""
    import pandas as pd
    ns = {"np": np, "pd": pd}
    exec(src[5], ns)
    exec(src[9], ns)
    hits = ns["select_hits"](frame)
    ns["hits"] = hits
    ns["select_signal_hits"].__defaults__ = (K, L)
    exec(src[10], ns)
    exec(src[11], ns)
    c12 = src[12]
    for name, v in (("n_det_layers", L), ("n_layer_hits", K), ("n_seed_layers", NS)):
        c12, k = re.subn(r"^%s = \d+$" % name, "%s = %d" % (name, v), c12, flags=re.M)
        assert k == 1, "cell 12 changed: %s" % name
    exec(c12, ns)
    exec(src[14], ns)
    exec(src[15], ns)
    return hits, ns


def check_dtypes(ns, src):
    """The dtype chain the specification states (gnn-fpga_amd/hit_samples.py), on the namespace's last sample."""
    hits, eid, pid = ns["hits"], ns["eid"], ns["pid"]
    evt = ns["evt_groups"].get_group(eid)
    trk = evt[evt.barcode == pid]
    lay = evt[evt.layer == 0]
    th = trk.iloc[0]
    assert isinstance(th.r, np.float64), "the track hit is no longer float64: %r" % type(th.r)
    te = ns["calc_eta"](th.r, th.z)
    le = ns["calc_eta"](lay.r, lay.z)
    assert np.asarray(te).dtype == np.float64 and le.dtype == np.float32
    deta = le - te
    assert deta.dtype == np.float32
    want = (le.values - np.float32(te)).astype(np.float32)
    assert np.array_equal(deta.values.view(np.uint32), want.view(np.uint32)), "lay_eta - trk_eta is not float32 - f32"
    dphi = ns["calc_dphi"](th.phi, lay.phi)
    assert dphi.dtype == np.float32
    d = ns["calc_eta_phi_distance"](te, le, th.phi, lay.phi)
    assert d.dtype == np.float32
    for c in ("r", "phi", "z"):
        assert hits[c].dtype == np.float32
    f = hits[["r", "phi", "z"]].iloc[:3] / ns["feature_scale"]
    assert all(f[c].dtype == np.float64 for c in f), "the feature division is no longer float64"
    return {"trk_eta": str(np.asarray(te).dtype), "lay_eta": str(le.dtype), "deta": str(deta.dtype),
            "dphi": str(dphi.dtype), "d": str(d.dtype), "features": str(f["r"].dtype)}


def tie_gap(ns, L, K):
    """Smallest gap in float32 ulps between consecutive sorted distances among the K + 1 smallest, over every
    (sample, layer); 0 is an exact tie."""
    worst = np.inf
    calc_eta, dist = ns["calc_eta"], ns["calc_eta_phi_distance"]
    for eid, pid in ns["sig_keys"]:
        evt = ns["evt_groups"].get_group(eid)
        trk = evt[evt.barcode == pid]
        for j in range(L):
            lay = evt[evt.layer == j]
            th = trk.iloc[j]
            d = np.sort(dist(calc_eta(th.r, th.z), calc_eta(lay.r, lay.z), th.phi, lay.phi).values)[:K + 1]
            gaps = (d[1:].view(np.int32).astype(np.int64) - d[:-1].view(np.int32).astype(np.int64))
            worst = min(worst, int(gaps.min()))
    return worst


def acts_frame(rng, n_events, n_tracks, n_noise, missing=0.0, dup=0.0, dup_equal=0.0, shared_noise=None,
               phi_edge=0, sparse_layer=None, absent_layer=None):
    """A seeded ACTS-like frame: per event `n_tracks` helix-like tracks over the 10 barrel layers and `n_noise`
    noise hits per layer; a fraction of tracks misses a layer, a fraction of track hits is duplicated (a second
    hit, some with exactly equal r)."""
    import pandas as pd
    rows = []
    for ev in range(n_events):
        recs = []
        for t in range(n_tracks):
            bc = int(rng.integers(1, 2 ** 40))
            phi0 = rng.uniform(-np.pi, np.pi)
            if t < phi_edge:
                phi0 = np.pi - rng.uniform(0, 0.02) if t % 2 == 0 else -np.pi + rng.uniform(0, 0.02)
            k = rng.uniform(-4e-4, 4e-4)
            z0, cot = rng.normal(0, 40), rng.uniform(-1, 1)
            skip = int(rng.integers(0, 10)) if rng.random() < missing else -1
            for l, (vid, lid) in enumerate(LAYIDS):
                if l == skip or (absent_layer is not None and ev == 0 and l == absent_layer):
                    continue
                if sparse_layer is not None and ev == 1 and l == sparse_layer and t >= 4:
                    continue                                # 4 hits on that layer: the event fails the count
                r = RADII[l] + rng.normal(0, 0.1)
                ph = phi0 + k * r
                z = z0 + r * cot + rng.normal(0, 0.5)
                recs.append((ev, bc, vid, lid, r, ph, z))
                if rng.random() < dup:
                    r2 = r if rng.random() < dup_equal else r + rng.normal(0, 0.3)
                    recs.append((ev, bc, vid, lid, r2, ph + rng.normal(0, 1e-3), z + rng.normal(0, 0.5)))
        for l, (vid, lid) in enumerate(LAYIDS):
            if absent_layer is not None and ev == 0 and l == absent_layer:
                continue
            m = n_noise if not (sparse_layer is not None and ev == 1 and l == sparse_layer) else 0
            for q in range(m):
                bc = shared_noise if shared_noise is not None else -int(rng.integers(1, 2 ** 40))
                recs.append((ev, bc, vid, lid, RADII[l] + rng.normal(0, 0.1), rng.uniform(-np.pi, np.pi),
                             rng.uniform(-1000, 1000)))
        recs = [recs[i] for i in rng.permutation(len(recs))]
        rows.extend(recs)
    ev, bc, vid, lid, r, ph, z = (np.array(c) for c in zip(*rows))
    ph = np.mod(ph + np.pi, 2 * np.pi) - np.pi
    x, y = (r * np.cos(ph)).astype(np.float32), (r * np.sin(ph)).astype(np.float32)
    xs, ys = pd.Series(x), pd.Series(y)
    return pd.DataFrame({"evtid": ev.astype(np.int64), "barcode": bc.astype(np.int64), "volid": vid.astype(np.int64),
                         "layid": lid.astype(np.int64)}).assign(
        z=z.astype(np.float32), r=np.sqrt(xs ** 2 + ys ** 2), phi=np.arctan2(ys, xs))


def builder_inputs(frame):
    """select_hits' barrel renumbering (the caller's column arithmetic), before deduplication."""
    vol = np.searchsorted(np.array(VIDS), frame.volid.values)
    assert np.array_equal(np.array(VIDS)[vol], frame.volid.values)
    layer = (frame.layid.values // 2 - 1 + 4 * vol).astype(np.int32)
    ev = frame.evtid.values
    assert np.all(np.diff(ev) >= 0), "events must be contiguous and ascending"
    E = int(ev.max()) + 1 if ev.size else 1
    event_ptr = np.searchsorted(ev, np.arange(E + 1)).astype(np.int64)
    return {"r": frame.r.values.astype(np.float32), "phi": frame.phi.values.astype(np.float32),
            "z": frame.z.values.astype(np.float32), "layer": layer, "particle_id": frame.barcode.values.astype(np.int64),
            "event_ptr": event_ptr}


def cases():
    rng = np.random.default_rng
    yield "duplicates", acts_frame(rng(1), 2, 12, 8, dup=0.3, dup_equal=0.5), 10, 5, 3
    yield "missing_layers", acts_frame(rng(2), 2, 14, 7, missing=0.4), 10, 5, 3
    yield "event_fails_count", acts_frame(rng(3), 3, 10, 6, sparse_layer=4), 10, 5, 3
    yield "absent_layer", acts_frame(rng(4), 2, 10, 7, absent_layer=9), 10, 5, 3
    yield "shared_noise", acts_frame(rng(5), 2, 8, 6, shared_noise=0), 10, 5, 3
    yield "phi_edges", acts_frame(rng(6), 2, 14, 8, phi_edge=10), 10, 5, 3
    yield "k8_seed2", acts_frame(rng(7), 2, 12, 9, missing=0.2, dup=0.1), 10, 8, 2
    yield "k3_seed0", acts_frame(rng(8), 2, 10, 5, missing=0.2, dup=0.1), 10, 3, 0
    yield "notebook", acts_frame(rng(9), 3, 40, 30, missing=0.1, dup=0.05), 10, 5, 3


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.path.join(os.path.dirname(REPO), "reference"),
                    help="the reference checkout (its gnn/MPNN_HitClassifier.ipynb is read)")
    ap.add_argument("--time", action="store_true", help="also time cells 10-15 on one synthetic event")
    args = ap.parse_args()
    src = load_cells(args.reference)
    os.makedirs(OUT, exist_ok=True)
    total = 0
    for name, frame, L, K, NS in cases():
        hits, ns = run_reference(src, frame, L, K, NS)
        S = int(ns["n_samples"])
        assert S > 0 or name == "event_fails_count"
        if S:
            dt = check_dtypes(ns, src)
            gap = tie_gap(ns, L, K)
            assert gap > 0, "%s: an exact tie at a selection boundary (reseed the case)" % name
        else:
            dt, gap = {}, None
        arrays = dict(builder_inputs(frame))
        arrays.update({"n_det_layers": np.int64(L), "n_layer_hits": np.int64(K), "n_seed_layers": np.int64(NS),
                       "full_X": ns["full_X"], "full_Ri": ns["full_Ri"], "full_Ro": ns["full_Ro"],
                       "full_y": ns["full_y"], "sig_keys": np.asarray(ns["sig_keys"], np.int64).reshape(-1, 2),
                       "min_gap_ulps": np.int64(gap if gap is not None else -1),
                       "dtypes": np.array(json.dumps(dt, sort_keys=True))})
        path = os.path.join(OUT, name + ".npz")
        write_npz(path, arrays)
        total += os.path.getsize(path)
        print("%-18s %5d hits %4d kept %4d samples  min gap %s ulps  %7d bytes" % (
            name, frame.shape[0], hits.shape[0], S, gap, os.path.getsize(path)))
    print("total %d bytes" % total)
    if args.time:
        frame = acts_frame(np.random.default_rng(11), 1, 200, 100)
        t0 = time.perf_counter()
        hits, ns = run_reference(src, frame, 10, 5, 3)
        dt = time.perf_counter() - t0
        S = int(ns["n_samples"])
        rec = {"what": "reference cells 5 and 9-15 (select_hits dedup, select_signal_hits, the cell-15 loop) on the "
                       "host CPU, one synthetic event: acts_frame(default_rng(11), 1 event, 200 tracks, 100 noise "
                       "hits per layer), about 300 hits per layer",
               "hits": int(frame.shape[0]), "samples": S, "seconds": round(dt, 3),
               "ms_per_sample": round(1e3 * dt / max(S, 1), 2)}
        with open(os.path.join(OUT, "reference_time.json"), "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        print(rec)


if __name__ == "__main__":
    main()
