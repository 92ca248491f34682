"""Fixtures for the graph builder (tests/golden/graph_build/*.npz), made by RUNNING the reference's own graph
construction: gnn/prepareGraphs.py `split_phi_sectors` (:87-106) and gnn/graph.py `construct_graph` (:95-142),
called per event as `process_event` (:136-170) calls them.  Nothing of the reference is copied: its modules are
imported from the checkout given with --reference (prepareGraphs.py with a stand-in `trackml` module, which it
imports for its CSV reader only).

Each file holds the inputs (r, phi, z, layer, particle_id, event_ptr, layer_pairs, n_phi_sectors and the cuts)
and, per graph g in event-major, sector-minor order, the reference's SparseGraph arrays g<g>_X, g<g>_Ri_rows,
g<g>_Ri_cols, g<g>_Ro_rows, g<g>_Ro_cols, g<g>_y.  The files are written with fixed zip timestamps, so a rerun
reproduces them bit for bit.  --time also measures the reference's host time for one c3-shaped event (1000
tracks, 10 layers, 8 sectors) and writes it to reference_time.json beside them.

usage: python tools/gen_graph_golden.py [--reference DIR] [--time]
"""
import argparse
import io
import json
import os
import sys
import time
import types
import zipfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "tests", "golden", "graph_build")

from gnn_fpga_amd import synth  # noqa: E402


def load_reference(ref_dir):
    gnn_dir = os.path.join(ref_dir, "gnn")
    sys.path.insert(0, gnn_dir)
    stub = types.ModuleType("trackml")
    stub.dataset = types.ModuleType("trackml.dataset")
    sys.modules.setdefault("trackml", stub)
    sys.modules.setdefault("trackml.dataset", stub.dataset)
    import graph as ref_graph            # gnn/graph.py
    import prepareGraphs as ref_prep     # gnn/prepareGraphs.py
    return ref_graph, ref_prep


def reference_graphs(ref_graph, ref_prep, cols, layer_pairs, n_phi_sectors, psm, pso, z0m):
    """process_event's graph step for every event of `cols` (gnn/prepareGraphs.py:143-169)."""
    import pandas as pd
    out = []
    ep = cols.event_ptr
    for e in range(ep.shape[0] - 1):
        s = slice(int(ep[e]), int(ep[e + 1]))
        hits = pd.DataFrame({"r": cols.r[s], "phi": cols.phi[s], "z": cols.z[s], "layer": cols.layer[s],
                             "particle_id": cols.particle_id[s]}).assign(evtid=e)
        for c in ("r", "phi", "z"):
            assert hits[c].dtype == np.float32
        sectors = ref_prep.split_phi_sectors(hits, n_phi_sectors=n_phi_sectors)
        feature_scale = np.array([1000., np.pi / n_phi_sectors, 1000.])
        for sh in sectors:
            assert sh.phi.dtype == np.float32, "the sector-centred phi is no longer float32"
            g, segments = ref_graph.construct_graph(sh, layer_pairs=layer_pairs, phi_slope_max=psm,
                                                    phi_slope_mid_max=psm, phi_slope_outer_max=pso, z0_max=z0m,
                                                    feature_names=["r", "phi", "z"], feature_scale=feature_scale)
            out.append(g)
    return out


def check_intermediate_dtypes(ref_graph, cols):
    """The arithmetic the builder restates is float32 in the reference for float32 columns: dphi, phi_slope, z0."""
    import pandas as pd
    h = pd.DataFrame({"r": cols.r[:64], "phi": cols.phi[:64], "z": cols.z[:64]})
    dphi = ref_graph.calc_dphi(h.phi, h.phi[::-1].reset_index(drop=True))
    dr = h.r[::-1].reset_index(drop=True) - h.r
    dz = h.z[::-1].reset_index(drop=True) - h.z
    assert dphi.dtype == np.float32 and (dphi / dr).dtype == np.float32 and (h.z - h.r * dz / dr).dtype == np.float32
    # thresholds given as Python floats compare in float32: f32(0.7) < 0.7 is False there, True in float64
    assert not bool((pd.Series(np.array([0.7], np.float32)) < 0.7).iloc[0])


def adjacent_pairs(n_layers=10):
    l = np.arange(n_layers)
    return np.stack([l[:-1], l[1:]], axis=1)


def cols_from(r, phi, z, layer, pid, event_ptr=None):
    r, phi, z = (np.asarray(v, dtype=np.float32) for v in (r, phi, z))
    ep = np.array([0, r.shape[0]], np.int64) if event_ptr is None else np.asarray(event_ptr, np.int64)
    return synth.HitColumns(r, phi, z, np.asarray(layer, np.int32), np.asarray(pid, np.int64), ep)


def cases():
    inf = float("inf")
    # 1. a ~2 k-hit event with the default cuts (gnn/prepareGraphs.py:37-42)
    yield "default_2k", synth.barrel_event(180, 200, seed=1), adjacent_pairs(), 8, 0.001, 0.001, 200.0
    # 2. hits exactly on the float32-rounded sector edges and on +-pi (8 sectors), two events
    ev = synth.barrel_event(60, 40, n_events=2, seed=2)
    edges = np.linspace(-np.pi, np.pi, 9)
    special = np.concatenate([edges.astype(np.float32), np.nextafter(edges.astype(np.float32), np.float32(0)),
                              [np.float32(np.pi), -np.float32(np.pi), np.float32(0.0)]]).astype(np.float32)
    phi = ev.phi.copy()
    rng = np.random.default_rng(3)
    pos = rng.choice(phi.shape[0], size=special.shape[0], replace=False)
    phi[pos] = special
    yield "sector_edges", ev._replace(phi=phi), adjacent_pairs(), 8, 0.001, 0.001, 200.0
    # 3. an empty layer (layer 4 has no hits: pairs (3, 4) and (4, 5) are skipped)
    ev = synth.barrel_event(150, 60, seed=4)
    keep = ev.layer != 4
    yield "empty_layer", cols_from(ev.r[keep], ev.phi[keep], ev.z[keep], ev.layer[keep], ev.particle_id[keep]), \
        adjacent_pairs(), 1, 0.001, 0.001, 200.0
    # 4. a repeated and a non-adjacent layer pair, layers beyond the pairs' range present
    ev = synth.barrel_event(120, 50, seed=5)
    yield "pairs_repeat_skip", ev, np.array([[0, 1], [2, 4], [0, 1], [7, 5], [8, 9]]), 2, 0.002, 0.002, 200.0
    # 5. dr = 0 pairs: a layer paired with itself, and hits sharing a radius across two layers
    ev = synth.barrel_event(80, 30, seed=6)
    r = ev.r.copy()
    r[ev.layer == 3] = np.float32(172.0)
    r[ev.layer == 2] = np.float32(172.0)
    yield "dr_zero", ev._replace(r=r), np.array([[2, 3], [3, 3], [0, 1], [1, 2]]), 1, 0.01, 0.01, 500.0
    # 6. all pairs with infinite thresholds (the muon graphs' rule, gnn/Muon_graph.py:60-83)
    ev = synth.barrel_event(12, 6, seed=7)
    yield "all_pairs_inf", ev, adjacent_pairs(), 1, inf, inf, inf
    # 7. a separate outer cut (pairs starting at layer >= 5 take phi_slope_outer_max)
    ev = synth.barrel_event(150, 100, seed=8)
    yield "outer_cut", ev, adjacent_pairs(), 4, 0.0006, 0.002, 150.0
    # 8. all three cuts ON values of the data (tests/pair_value_cases.py chooses them where a reciprocal-multiply
    # differs from the division): the pair at each cut is not kept, and would be one ulp further up
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import pair_value_cases
    psm, pso, z0m = pair_value_cases.fixture_cuts()
    yield "pair_values", pair_value_cases.probe_event("one").cols, adjacent_pairs(), 1, psm, pso, z0m


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
                    help="the reference checkout, its gnn/ directory is imported (default: ../reference beside "
                         "this repository)")
    ap.add_argument("--time", action="store_true", help="also time construct_graph on a c3-shaped event")
    args = ap.parse_args()
    ref_graph, ref_prep = load_reference(args.reference)
    os.makedirs(OUT, exist_ok=True)
    total = 0
    for name, cols, pairs, S, psm, pso, z0m in cases():
        check_intermediate_dtypes(ref_graph, cols)
        graphs = reference_graphs(ref_graph, ref_prep, cols, pairs, S, psm, pso, z0m)
        arrays = {"r": cols.r, "phi": cols.phi, "z": cols.z, "layer": cols.layer, "particle_id": cols.particle_id,
                  "event_ptr": cols.event_ptr, "layer_pairs": np.asarray(pairs, np.int32),
                  "n_phi_sectors": np.int64(S), "cuts": np.array([psm, pso, z0m], np.float64),
                  "n_graphs": np.int64(len(graphs))}
        for g, sg in enumerate(graphs):
            for k in ("X", "Ri_rows", "Ri_cols", "Ro_rows", "Ro_cols", "y"):
                v = getattr(sg, k)
                arrays["g%d_%s" % (g, k)] = v.astype(np.int32) if k.endswith(("rows", "cols")) else v
        path = os.path.join(OUT, name + ".npz")
        write_npz(path, arrays)
        total += os.path.getsize(path)
        print("%-18s %2d graphs %6d hits %7d segments %7d bytes" % (
            name, len(graphs), sum(g.X.shape[0] for g in graphs), sum(g.y.shape[0] for g in graphs),
            os.path.getsize(path)))
    print("total %d bytes" % total)
    if args.time:
        cols = synth.barrel_event(1000, 0, seed=11)
        t0 = time.perf_counter()
        graphs = reference_graphs(ref_graph, ref_prep, cols, adjacent_pairs(), 8, 0.001, 0.001, 200.0)
        dt = time.perf_counter() - t0
        rec = {"what": "reference split_phi_sectors + construct_graph, one c3-shaped event on the host CPU "
                       "(synth.barrel_event(1000, 0, seed=11), 8 sectors, default cuts)",
               "hits": int(cols.r.shape[0]), "segments": int(sum(g.y.shape[0] for g in graphs)),
               "seconds": round(dt, 3)}
        with open(os.path.join(OUT, "reference_time.json"), "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        print(rec)


if __name__ == "__main__":
    main()
