"""Fixtures for the hit selection (tests/golden/select_hits/*.npz), made by RUNNING the reference's own selection:
gnn/prepareGraphs.py `select_hits` (:53-85), called per event as `process_event` (:136-170) calls it, and for the
chain case `split_phi_sectors` (:87-106) and gnn/graph.py `construct_graph` after it.  Nothing of the reference is
copied: its modules are imported from the checkout given with --reference (prepareGraphs.py with a stand-in `trackml`
module, which it imports for its CSV reader only).

One adaptation, the one tools/gen_event_graphs_golden.py states for the notebook's copy of the function: under pandas
2.3 `groupby([...], as_index=False).r.idxmin()` is a DataFrame and `hits.loc[<DataFrame>]` raises; `select_hits` is
executed from its own source text with `.r.idxmin()` replaced by `.r.idxmin().r`.  The generator asserts that the
replaced text occurs exactly once.

Inputs are seeded synthetic raw tables (gnn-fpga_amd/synth.py trackml_events) with hand-made changes where a case
needs them; every event carries rows on each of the ten barrel layers (the reference raises otherwise).  Each file
holds the three tables (hits_*, truth_*, particles_*, their event_ptr), phi (np.arctan2(y, x) per hit row, float32:
what the reference computes, handed to the selection as given), pt_min, no_missing_hits and the reference's result:
ref_row (the input row of each selected hit, found by its hit_id), ref_hit_id, ref_layer, ref_particle_id, ref_r,
ref_phi, ref_z and ref_event_ptr; the chain case also holds the reference's graphs in the layout of
tests/golden/graph_build (g<g>_X, g<g>_Ri_rows, ...).  Files are written with fixed zip timestamps, so a rerun
reproduces them bit for bit.

--time runs the reference's select_hits on one detector-scale synthetic event and writes reference_time.json.

usage: python tools/gen_select_hits_golden.py [--reference DIR] [--time]
"""
import argparse
import inspect
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from gnn_fpga_amd import synth  # noqa: E402
from gen_graph_golden import adjacent_pairs, load_reference, write_npz  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "select_hits")
TABLES = (("hits", ("hit_id", "x", "y", "z", "volume_id", "layer_id")), ("truth", ("hit_id", "particle_id")),
          ("particles", ("particle_id", "px", "py")))
DETECTOR_EVENT = dict(n_events=1, n_tracks=10000, n_noise=20000, seed=11)     # about 130 000 hits, 11 000 particles
F32 = np.float32
BIG = 2 ** 62


def reference_select_hits(ref_prep):
    """The reference's select_hits, from its own source text with the one stated adaptation."""
    import pandas as pd
    text = inspect.getsource(ref_prep.select_hits)
    old = ".r.idxmin()\n"
    assert text.count(old) == 1, "select_hits changed: the pandas adaptation no longer applies"
    ns = {"np": np, "pd": pd}
    exec(text.replace(old, ".r.idxmin().r\n"), ns)
    return ns["select_hits"]


def frames(ev, e):
    """Event e's three tables as the DataFrames trackml.dataset.load_event gives."""
    import pandas as pd
    out = []
    for name, cols in TABLES:
        ep = ev[name]["event_ptr"]
        out.append(pd.DataFrame({k: ev[name][k][ep[e]:ep[e + 1]] for k in cols}))
    return out


def run_reference(sel, ev, pt_min, no_missing):
    """select_hits per event, as process_event calls it: (the stored arrays, the frames)."""
    ep = ev["hits"]["event_ptr"]
    parts = {k: [] for k in ("row", "hit_id", "layer", "particle_id", "r", "phi", "z")}
    out_ptr, kept = [0], []
    for e in range(ep.shape[0] - 1):
        hits, truth, particles = frames(ev, e)
        for c in ("x", "y", "z"):
            assert hits[c].dtype == np.float32
        assert particles.px.dtype == particles.py.dtype == np.float32
        got = sel(hits, truth, particles, pt_min=pt_min, no_missing_hits=no_missing)
        if len(got):
            assert got.r.dtype == got.phi.dtype == got.z.dtype == np.float32, (got.r.dtype, got.phi.dtype)
        ids = ev["hits"]["hit_id"][ep[e]:ep[e + 1]]
        o = np.argsort(ids, kind="stable")
        assert np.all(np.diff(ids[o]) > 0)
        hid = got.hit_id.values.astype(np.int64)
        row = o[np.searchsorted(ids[o], hid)] + ep[e]
        assert np.array_equal(ev["hits"]["hit_id"][row], hid)
        parts["row"].append(row)
        parts["hit_id"].append(hid)
        parts["layer"].append(got.layer.values.astype(np.int32))
        parts["particle_id"].append(got.particle_id.values.astype(np.int64))
        for c in ("r", "phi", "z"):
            parts[c].append(got[c].values.astype(F32))
        out_ptr.append(out_ptr[-1] + len(got))
        kept.append(got)
    dt = {"row": np.int64, "hit_id": np.int64, "layer": np.int32, "particle_id": np.int64, "r": F32, "phi": F32, "z": F32}
    ref = {"ref_" + k: np.concatenate(v).astype(dt[k]) for k, v in parts.items()}
    ref["ref_event_ptr"] = np.asarray(out_ptr, np.int64)
    return ref, kept


def one_event(ev):
    assert ev["hits"]["event_ptr"].shape[0] == 2
    return ev


def append_hits(ev, rows):
    """A one-event `ev` with hand-placed hits (x, y, z, volume_id, layer_id, particle_id) appended, numbered on."""
    ev = one_event(ev)
    h, t = ev["hits"], ev["truth"]
    nid = int(h["hit_id"].max()) + 1 + np.arange(len(rows))
    new = {"hit_id": nid, "x": [r[0] for r in rows], "y": [r[1] for r in rows], "z": [r[2] for r in rows],
           "volume_id": [r[3] for r in rows], "layer_id": [r[4] for r in rows]}
    for k, v in new.items():
        h[k] = np.concatenate([h[k], np.asarray(v).astype(h[k].dtype)])
    t["hit_id"] = np.concatenate([np.asarray(nid, np.int64), t["hit_id"]])        # (truth in another order)
    t["particle_id"] = np.concatenate([np.asarray([r[5] for r in rows], np.int64), t["particle_id"]])
    h["event_ptr"] = np.array([0, h["hit_id"].shape[0]], np.int64)
    t["event_ptr"] = np.array([0, t["hit_id"].shape[0]], np.int64)
    return ev


def track_hits(ev, k):
    """(particle id, rows) of the k-th particle row's hits on barrel layers, one-event `ev`."""
    pid = int(ev["particles"]["particle_id"][k])
    hid = ev["truth"]["hit_id"][ev["truth"]["particle_id"] == pid]
    rows = np.flatnonzero(np.isin(ev["hits"]["hit_id"], hid))
    vl = set(synth.ACTS_BARREL_LAYERS)
    return pid, np.array([r for r in rows if (int(ev["hits"]["volume_id"][r]), int(ev["hits"]["layer_id"][r])) in vl])


def with_hits(ev, lo=0):
    """Particle rows of a one-event `ev` that have barrel hits, from row `lo` on."""
    return [k for k in range(lo, ev["particles"]["particle_id"].shape[0]) if track_hits(ev, k)[1].size > 0]


def cases():
    """(name, tables, pt_min, no_missing_hits)"""
    T = synth.trackml_events
    yield "default", T(1, 60, 80, seed=1), 0.5, False
    yield "no_missing", T(1, 60, 80, seed=2, missing=0.4), 0.5, True
    # groups of 3 and more hits with exactly equal r: copies of a hit's (x, y) under new hit_ids, and hits at
    # mirrored (x, y) (the same r from other coordinates); the lowest input row must win
    ev = T(1, 30, 40, seed=3, dup=0.3, dup_equal=1.0, pt_range=(0.6, 3.0))
    extra = []
    for k in with_hits(ev)[:6]:
        pid, rows = track_hits(ev, k)
        for r in rows[:3]:
            h = ev["hits"]
            x, y, z, v, l = h["x"][r], h["y"][r], h["z"][r], h["volume_id"][r], h["layer_id"][r]
            extra += [(x, y, z + 1.0, v, l, pid), (y, x, z + 2.0, v, l, pid), (-x, y, z + 3.0, v, l, pid)]
    yield "ties", append_hits(ev, extra), 0.5, False
    # a particle with pt exactly pt_min is dropped (the cut is strict)
    ev = T(1, 40, 60, seed=4)
    k = with_hits(ev)[0]
    ev["particles"]["px"][k], ev["particles"]["py"][k] = F32(0.3), F32(0.4)
    edge = np.sqrt(ev["particles"]["px"][k] ** 2 + ev["particles"]["py"][k] ** 2)
    assert edge.dtype == np.float32
    yield "pt_edge", ev, float(edge), False
    ev = T(1, 40, 60, seed=5)
    k = with_hits(ev)[0]
    ev["particles"]["px"][k], ev["particles"]["py"][k] = F32(0.0), F32(0.0)
    yield "pt_edge_zero", ev, 0.0, False
    # ids: particle ids above 2^53 one apart (one passes the cut, its neighbour fails; two more both pass),
    # non-contiguous hit_ids, truth rows for absent hits, hits without truth rows, particles without hits
    ev = T(1, 40, 60, seed=6, extra_particles=0.3)
    ks = with_hits(ev)[:4]
    for k, new, pt in zip(ks, (BIG + 1, BIG + 2, BIG + 5, BIG + 6), (2.0, 0.1, 1.5, 1.5)):
        old = ev["particles"]["particle_id"][k]
        ev["particles"]["particle_id"][k] = new
        ev["truth"]["particle_id"][ev["truth"]["particle_id"] == old] = new
        ev["particles"]["px"][k], ev["particles"]["py"][k] = F32(pt), F32(0.0)
    for tb in ("hits", "truth"):
        ev[tb]["hit_id"] = ev[tb]["hit_id"].astype(np.int64) * 7 + 3
    t = ev["truth"]
    keep = np.ones(t["hit_id"].shape[0], bool)
    keep[::9] = False                                                  # hits without truth rows
    absent = np.arange(5, 5 + 7 * 20, 7, dtype=np.int64)               # no hit has an id = 5 mod 7
    t["hit_id"] = np.concatenate([t["hit_id"][keep], absent])
    t["particle_id"] = np.concatenate([t["particle_id"][keep], np.resize(ev["particles"]["particle_id"], 20)])
    t["event_ptr"] = np.array([0, t["hit_id"].shape[0]], np.int64)
    yield "ids", ev, 0.5, False
    yield "other_volumes", T(1, 40, 60, seed=7, other=0.4), 0.5, False
    # three events in one call: hit_ids restart at 1, particle ids are shared, event 1 is left empty by the pt cut
    ev = T(3, 40, 60, seed=8, shared_ids=True)
    pe = ev["particles"]["event_ptr"]
    for c in ("px", "py"):
        ev["particles"][c][pe[1]:pe[2]] *= F32(0.01)
    yield "multi_event", ev, 0.5, False
    yield "chain", T(2, 50, 60, seed=9), 0.5, False


def check_case(name, ev, ref, pt_min):
    """What each case is named for, asserted on the reference's own result."""
    h, t, p = ev["hits"], ev["truth"], ev["particles"]
    for e in range(h["event_ptr"].shape[0] - 1):
        s = slice(h["event_ptr"][e], h["event_ptr"][e + 1])
        have = set(zip(h["volume_id"][s].tolist(), h["layer_id"][s].tolist()))
        assert have >= set(synth.ACTS_BARREL_LAYERS), "an event without rows on a barrel layer"
    pt = np.sqrt(p["px"] ** 2 + p["py"] ** 2)
    if name == "default":
        assert 0 < len(ref["ref_row"]) and np.any(pt <= F32(pt_min)) and np.any(t["particle_id"] == 0)
    if name == "no_missing":
        pid, cnt = np.unique(ref["ref_particle_id"], return_counts=True)
        assert len(pid) > 5 and np.all(cnt == 10)
    if name == "ties":
        rows = ref["ref_row"]
        r = np.sqrt(h["x"] ** 2 + h["y"] ** 2)
        tp = dict(zip(t["hit_id"].tolist(), t["particle_id"].tolist()))
        big = 0
        for row, pid, lay in zip(rows, ref["ref_particle_id"], ref["ref_layer"]):
            v, l = synth.ACTS_BARREL_LAYERS[lay]
            grp = [q for q in np.flatnonzero((h["volume_id"] == v) & (h["layer_id"] == l))
                   if tp.get(int(h["hit_id"][q])) == pid]
            least = [q for q in grp if r[q] == min(r[g] for g in grp)]
            assert row == min(least), "the lowest row of the smallest r did not win"
            big += len(least) >= 3
        assert big >= 10, "too few groups of 3 and more hits with equal r"
    if name == "pt_edge":
        k = np.flatnonzero(pt == F32(pt_min))
        assert k.size == 1 and p["particle_id"][k[0]] not in ref["ref_particle_id"]
        assert np.isin(h["hit_id"], t["hit_id"][t["particle_id"] == p["particle_id"][k[0]]]).any()
    if name == "pt_edge_zero":
        k = np.flatnonzero(pt == 0)
        assert pt_min == 0.0 and k.size == 1 and p["particle_id"][k[0]] not in ref["ref_particle_id"]
    if name == "ids":
        got = set(ref["ref_particle_id"].tolist())
        assert {BIG + 1, BIG + 5, BIG + 6} <= got and BIG + 2 not in got
        assert not np.isin(t["hit_id"], h["hit_id"]).all() and not np.isin(h["hit_id"], t["hit_id"]).all()
        assert not np.isin(p["particle_id"], t["particle_id"]).all() and np.all(np.diff(np.sort(h["hit_id"])) >= 7)
    if name == "other_volumes":
        have = set(zip(h["volume_id"].tolist(), h["layer_id"].tolist()))
        assert {(8, 3), (7, 2), (9, 4)} <= have
    if name == "multi_event":
        ep = ref["ref_event_ptr"]
        assert ep[1] == ep[2] and ep[1] > 0 and ep[3] > ep[2], "event 1 is not the empty one"
        hp = h["event_ptr"]
        assert all(h["hit_id"][hp[e]:hp[e + 1]].min() == 1 for e in range(3))
        pe = p["event_ptr"]
        assert set(p["particle_id"][pe[0]:pe[1]].tolist()) & set(p["particle_id"][pe[2]:pe[3]].tolist())


def chain_graphs(ref_graph, ref_prep, kept, cuts):
    """process_event after the selection (gnn/prepareGraphs.py:146-169) for every event's selected hits."""
    S, psm, pso, z0m = cuts
    out = []
    for e, hits in enumerate(kept):
        sectors = ref_prep.split_phi_sectors(hits.assign(evtid=e), n_phi_sectors=S)
        feature_scale = np.array([1000., np.pi / S, 1000.])
        for sh in sectors:
            assert sh.phi.dtype == np.float32
            g, _ = ref_graph.construct_graph(sh, layer_pairs=adjacent_pairs(), phi_slope_max=psm, phi_slope_mid_max=psm,
                                             phi_slope_outer_max=pso, z0_max=z0m, feature_names=["r", "phi", "z"],
                                             feature_scale=feature_scale)
            out.append(g)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.path.join(os.path.dirname(REPO), "reference"),
                    help="the reference checkout, its gnn/ directory is imported")
    ap.add_argument("--time", action="store_true", help="also time select_hits on one detector-scale event")
    args = ap.parse_args()
    ref_graph, ref_prep = load_reference(args.reference)
    sel = reference_select_hits(ref_prep)
    os.makedirs(OUT, exist_ok=True)
    total = 0
    for name, ev, pt_min, no_missing in cases():
        ref, kept = run_reference(sel, ev, pt_min, no_missing)
        check_case(name, ev, ref, pt_min)
        phi = np.arctan2(ev["hits"]["y"], ev["hits"]["x"])
        assert phi.dtype == np.float32
        assert np.array_equal(phi[ref["ref_row"]].view(np.uint32), ref["ref_phi"].view(np.uint32))
        arrays = {"%s_%s" % (tb, k): ev[tb][k] for tb, cols in TABLES for k in cols + ("event_ptr",)}
        arrays.update(ref)
        arrays.update({"phi": phi, "pt_min": np.float64(pt_min), "no_missing_hits": np.int64(no_missing)})
        if name == "chain":
            cuts = (8, 0.001, 0.001, 200.0)
            graphs = chain_graphs(ref_graph, ref_prep, kept, cuts)
            arrays.update({"n_phi_sectors": np.int64(cuts[0]), "cuts": np.array(cuts[1:], np.float64),
                           "n_graphs": np.int64(len(graphs))})
            assert sum(g.y.shape[0] for g in graphs) > 100
            for g, sg in enumerate(graphs):
                for k in ("X", "Ri_rows", "Ri_cols", "Ro_rows", "Ro_cols", "y"):
                    v = getattr(sg, k)
                    arrays["g%d_%s" % (g, k)] = v.astype(np.int32) if k.endswith(("rows", "cols")) else v
        path = os.path.join(OUT, name + ".npz")
        write_npz(path, arrays)
        total += os.path.getsize(path)
        print("%-14s %2d events %5d rows %5d selected %7d bytes" % (
            name, ev["hits"]["event_ptr"].shape[0] - 1, ev["hits"]["x"].shape[0], ref["ref_row"].shape[0],
            os.path.getsize(path)))
    print("total %d bytes" % total)
    if args.time:
        ev = synth.trackml_events(**DETECTOR_EVENT)
        hits, truth, particles = frames(ev, 0)
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            got = sel(hits, truth, particles, pt_min=1.0)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        rec = {"what": "reference select_hits (gnn/prepareGraphs.py:53-85, pt_min 1.0) on the host CPU, one synthetic "
                       "event: synth.trackml_events(1, 10000, 20000, seed=11); the best of three runs",
               "hits": int(len(hits)), "particles": int(len(particles)), "selected": int(len(got)),
               "seconds": round(best, 3)}
        with open(os.path.join(OUT, "reference_time.json"), "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        print(rec)


if __name__ == "__main__":
    main()
