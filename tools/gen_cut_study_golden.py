"""Fixtures for the cut study and the layer census (tests/golden/cut_study/*.npz), made by RUNNING the reference's own
notebook cells, read from the checkout given with --reference and executed here.  Nothing of the reference is copied
into this repository.

All-pair counts: cells 3 (calc_dphi) and 18 (the all-pairs loop) of gnn/GraphConstructionDev_mu200.ipynb.  Each
event's frame first goes through gnn/prepareGraphs.py `split_phi_sectors` (:87-106) with one sector, as
`process_event` does before it builds a graph: that re-centres phi in float32 and drops a hit exactly on +-pi, which
is what the graph builder's pairs are made of.  Cell 18 is then run once per (event, layer pair) - a pair with a
layer that has no hit is skipped as gnn/graph.py:82-89 does, where the cell itself would raise KeyError - and the
tool bins the cell's `phi_slope.abs()`, `z0.abs()` and `y` with np.searchsorted(edges, v, side="right").
Adaptation: the `%%time` magic is dropped.

Layer census: cells 16-17 and 37-40 of gnn/GraphConstructionDev.ipynb on the same frames with volid = 0 and
layid = layer.  Cell 39 is an IPython help query (`...?`) and is dropped.  The table is cell 40's `gid_counts`; cell
17's unique `gid_pairs` must be its non-zero entries.  The reference's sort_values('r') leaves the order of equal r
open, so the tool asserts that no (event, particle) has two equal r wherever it writes a census.

Each file holds the inputs (r, phi, z, layer, particle_id, event_ptr, layer_pairs), the float32 edges, `counts`
int64 [P, 2, NS + 1, NZ + 1] and, where made, `census` int64 [L, L].  Files are written with fixed zip timestamps,
so a rerun reproduces them bit for bit.  --time also measures the reference's host seconds for one c3-shaped event
(cell 18 after the one-sector split, and census cells 17 and 38-40) and writes reference_time.json beside them.

usage: python tools/gen_cut_study_golden.py [--reference DIR] [--time]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
OUT = os.path.join(REPO, "tests", "golden", "cut_study")

from gnn_fpga_amd import synth  # noqa: E402
from gen_graph_golden import adjacent_pairs, cols_from, load_reference, write_npz  # noqa: E402

N_LAYERS = 10


def load_cells(ref_dir, notebook, cells):
    with open(os.path.join(ref_dir, "gnn", notebook)) as f:
        nb = json.load(f)
    src = {}
    for i in cells:
        text = "".join(nb["cells"][i]["source"])
        src[i] = "\n".join(ln for ln in text.split("\n")
                           if not ln.lstrip().startswith("%") and not ln.rstrip().endswith("?"))
    return src


def event_frames(cols):
    import pandas as pd
    ep = cols.event_ptr
    for e in range(ep.shape[0] - 1):
        s = slice(int(ep[e]), int(ep[e + 1]))
        yield e, pd.DataFrame({"r": cols.r[s], "phi": cols.phi[s], "z": cols.z[s], "layer": cols.layer[s],
                               "barcode": cols.particle_id[s]}).assign(evtid=e)


def reference_counts(ref_prep, mu200, cols, pairs, se, ze):
    """Cell 18 per (event, pair) on the one-sector frames -> counts [P, 2, NS + 1, NZ + 1]."""
    import pandas as pd
    NS, NZ = se.shape[0], ze.shape[0]
    counts = np.zeros((len(pairs), 2, NS + 1, NZ + 1), np.int64)
    ns = {"np": np, "pd": pd}
    exec(mu200[3], ns)
    for e, frame in event_frames(cols):
        (hits,) = ref_prep.split_phi_sectors(frame, n_phi_sectors=1)
        assert hits.phi.dtype == hits.r.dtype == hits.z.dtype == np.float32
        present = set(hits.layer.unique().tolist())
        for p, (l1, l2) in enumerate(np.asarray(pairs).tolist()):
            if l1 not in present or l2 not in present:      # gnn/graph.py:82-89
                continue
            ns.update(evtids=np.array([e]), n_events=1, evt_hit_groups=hits.groupby("evtid"),
                      layer_pairs=np.array([[l1, l2]]))
            exec(mu200[18], ns)
            seg = ns["segments"]
            assert seg.phi_slope.dtype == seg.z0.dtype == np.float32, "the cell's arithmetic is no longer float32"
            assert seg.shape[0] == int((hits.layer == l1).sum()) * int((hits.layer == l2).sum())
            bs = np.searchsorted(se, seg.phi_slope.abs().values, side="right")
            bz = np.searchsorted(ze, seg.z0.abs().values, side="right")
            cell = (seg.y.values.astype(np.int64) * (NS + 1) + bs) * (NZ + 1) + bz
            counts[p] += np.bincount(cell, minlength=2 * (NS + 1) * (NZ + 1)).reshape(2, NS + 1, NZ + 1)
    return counts


def census_frame(cols):
    import pandas as pd
    return pd.concat([f for _, f in event_frames(cols)], ignore_index=True).assign(
        volid=0, layid=lambda d: d.layer.astype(np.int64))


def reference_census(dev, cols, n_layers):
    """Cells 16-17 and 37-40 -> table [L, L]."""
    import pandas as pd
    hits = census_frame(cols)
    ties = hits.groupby(["evtid", "barcode"]).r.agg(lambda v: v.duplicated().any())
    assert not ties.any(), "a particle with two equal r: the reference's sort leaves their order open"
    ns = {"np": np, "pd": pd, "hits": hits}
    for i in (16, 17, 37, 38, 39, 40):
        exec(dev[i], ns)
    table = np.zeros((n_layers, n_layers), np.int64)
    gc = ns["gid_counts"]
    assert np.all(gc.volid_1.values == 0) and np.all(gc.volid_2.values == 0)
    table[gc.layid_1.values.astype(np.int64), gc.layid_2.values.astype(np.int64)] = gc.n.values
    a, b = np.nonzero(table)
    assert np.array_equal(ns["gid_pairs"][:, [1, 3]], np.stack([a, b], axis=1)), "cell 17 and cell 40 disagree"
    return table


SLOPE_EDGES = [0.0, 1e-4, 3e-4, 6e-4, 1e-3, 2e-3, 5e-3, 1e-2]
Z0_EDGES = [25.0, 50.0, 100.0, 200.0, 400.0, 1000.0]


def cases():
    """name, columns, layer pairs, phi_slope edges, z0 edges, make a census"""
    inf = float("inf")
    # 1. a 10-layer event with the notebooks' adjacent layer pairs
    yield "notebook", synth.barrel_event(28, 40, seed=31), adjacent_pairs(), SLOPE_EDGES, Z0_EDGES, True
    # 2. dr = 0: hits sharing a radius across two layers, and a layer paired with itself
    ev = synth.barrel_event(24, 20, seed=32)
    r = ev.r.copy()
    r[(ev.layer == 2) | (ev.layer == 3)] = np.float32(172.0)
    yield "dr_zero", ev._replace(r=r), np.array([[2, 3], [3, 3], [0, 1], [1, 2]]), SLOPE_EDGES, Z0_EDGES, False
    # 3. hits at +-pi (dropped by the sector split), just inside them, and tracks that cross the wrap
    ev = synth.barrel_event(30, 20, seed=33)
    pi32 = np.float32(np.pi)
    special = np.array([pi32, -pi32, np.nextafter(pi32, np.float32(0)), np.nextafter(-pi32, np.float32(0))] * 4,
                       np.float32)
    phi = ev.phi.copy()
    near = np.flatnonzero(np.abs(ev.phi) > 2.9)
    phi[near[:special.shape[0]]] = special[:near.shape[0]]
    yield "phi_wrap", ev._replace(phi=phi), adjacent_pairs(), SLOPE_EDGES, Z0_EDGES, True
    # 4. a layer without hits: pairs (3, 4) and (4, 5) add nothing
    ev = synth.barrel_event(26, 30, seed=34)
    keep = ev.layer != 4
    yield "missing_layer", cols_from(ev.r[keep], ev.phi[keep], ev.z[keep], ev.layer[keep], ev.particle_id[keep]), \
        adjacent_pairs(), SLOPE_EDGES, Z0_EDGES, True
    # 5. two events (noise ids repeat across them), a repeated and a backward pair
    yield "two_events", synth.barrel_event(14, 12, n_events=2, seed=35), \
        np.array([[0, 1], [1, 2], [0, 1], [5, 6], [7, 5], [8, 9]]), SLOPE_EDGES, Z0_EDGES, True
    # 6. +inf as the last edge of both axes: the last bins hold only dr = 0 pairs
    ev = synth.barrel_event(20, 15, seed=36)
    r = ev.r.copy()
    r[(ev.layer == 0) | (ev.layer == 1)] = np.float32(32.0)
    yield "inf_edge", ev._replace(r=r), adjacent_pairs(), [1e-3, 1e-2, inf], [200.0, inf], False
    # 7. edges ON values of the data, each with its upper neighbour: one-ulp bins (tests/pair_value_cases.py chooses
    # the values where a reciprocal-multiply differs from the division)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import pair_value_cases
    se, ze = pair_value_cases.fixture_edges()
    yield "pair_values", pair_value_cases.probe_event("one").cols, adjacent_pairs(), se, ze, False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.path.join(os.path.dirname(REPO), "reference"),
                    help="the reference checkout (its gnn/ notebooks are read, gnn/prepareGraphs.py is imported)")
    ap.add_argument("--time", action="store_true", help="also time the cells on a c3-shaped event")
    args = ap.parse_args()
    _, ref_prep = load_reference(args.reference)
    mu200 = load_cells(args.reference, "GraphConstructionDev_mu200.ipynb", (3, 18))
    dev = load_cells(args.reference, "GraphConstructionDev.ipynb", (16, 17, 37, 38, 39, 40))
    os.makedirs(OUT, exist_ok=True)
    total = 0
    for name, cols, pairs, se, ze, with_census in cases():
        with np.errstate(over="ignore"):
            se, ze = np.asarray(se, np.float32), np.asarray(ze, np.float32)
        pairs = np.asarray(pairs, np.int32)
        counts = reference_counts(ref_prep, mu200, cols, pairs, se, ze)
        arrays = {"r": cols.r, "phi": cols.phi, "z": cols.z, "layer": cols.layer, "particle_id": cols.particle_id,
                  "event_ptr": cols.event_ptr, "layer_pairs": pairs, "phi_slope_edges": se, "z0_edges": ze,
                  "counts": counts}
        if with_census:
            arrays["census"] = reference_census(dev, cols, N_LAYERS)
        path = os.path.join(OUT, name + ".npz")
        write_npz(path, arrays)
        total += os.path.getsize(path)
        print("%-14s %4d hits %7d pairs (%5d true) last cell %7d census %s %6d bytes" % (
            name, cols.r.shape[0], counts.sum(), counts[:, 1].sum(), counts[:, :, -1, -1].sum(),
            int(arrays["census"].sum()) if with_census else "-", os.path.getsize(path)))
    print("total %d bytes" % total)
    if args.time:
        cols = synth.barrel_event(1000, 0, seed=11)
        se, ze = np.asarray(SLOPE_EDGES, np.float32), np.asarray(Z0_EDGES, np.float32)
        t0 = time.perf_counter()
        counts = reference_counts(ref_prep, mu200, cols, adjacent_pairs(), se, ze)
        t_study = time.perf_counter() - t0
        t0 = time.perf_counter()
        table = reference_census(dev, cols, N_LAYERS)
        t_census = time.perf_counter() - t0
        rec = {"what": "the reference's notebook cells on the host CPU, one c3-shaped event "
                       "(synth.barrel_event(1000, 0, seed=11), one sector, 9 adjacent layer pairs): "
                       "study = split_phi_sectors + GraphConstructionDev_mu200 cell 18 per pair + the binning; "
                       "census = GraphConstructionDev cells 16-17 and 37-40",
               "hits": int(cols.r.shape[0]), "pairs": int(counts.sum()), "transitions": int(table.sum()),
               "study_seconds": round(t_study, 3), "census_seconds": round(t_census, 3)}
        with open(os.path.join(OUT, "reference_time.json"), "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        print(rec)


if __name__ == "__main__":
    main()
