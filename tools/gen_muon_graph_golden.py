"""Fixtures for the muon graph builder (tests/golden/muon_graph/*.npz), made by RUNNING the reference's own
gnn/prepareMuonGraphs.py `main()` unmodified, through sys.argv and a temporary input and output directory.  Nothing of
the reference is copied: its modules are imported from the checkout given with --reference.  It imports `uproot` to
read ROOT files only; a stand-in module serves `tree.pandas.df` as (entry, subentry)-indexed frames of
synth.emtf_events-style columns.  `plotgraphs` is replaced by a no-op, and `construct_graph` is wrapped to record the
entry of every graph it is called for (the file numbers count graphs, written or not).

Each file holds the inputs (mu_<column>, pu_<column>, mu_event_ptr, pu_event_ptr, vp_pt, vp_eta, vp_ptr,
entry_start, muon_only), graph_entry [every graph's entry, in file-number order] and, for every npz file the
reference wrote, in file order, file_graph [its file number] and f<k>_X, f<k>_Ri_rows, f<k>_Ri_cols, f<k>_Ro_rows,
f<k>_Ro_cols, f<k>_y, f<k>_pt, f<k>_eta.  Fixed zip timestamps: a rerun reproduces the bytes.  --time measures the
reference's host time per event on 64 entries and writes reference_time.json beside them.

usage: python tools/gen_muon_graph_golden.py [--reference DIR] [--time]
"""
import argparse
import contextlib
import glob
import io
import json
import os
import sys
import tempfile
import time
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))
OUT = os.path.join(REPO, "tests", "golden", "muon_graph")

from gnn_fpga_amd import synth  # noqa: E402
from gnn_fpga_amd.muon_graph import HIT_FEATURES  # noqa: E402
from gen_graph_golden import write_npz  # noqa: E402

FILES = {}          # path -> (hit columns, vp arrays, entry_start) served by the stand-in uproot


class _Tree:
    def __init__(self, src):
        self.src = src
        self.pandas = self

    def df(self, branches, entrystart=None, entrystop=None):
        import pandas as pd
        cols, vp, start = self.src
        if branches[0].startswith("vp_"):
            ptr, data = vp["vp_ptr"], {k: vp[k] for k in branches}
        else:
            ptr, data = cols["event_ptr"], {k: cols[k] for k in branches}
        n_e = ptr.shape[0] - 1
        lo = max(int(entrystart) - start, 0)
        hi = min(int(entrystop) - start, n_e)
        rows = np.arange(ptr[lo], ptr[hi])
        entry = start + np.repeat(np.arange(lo, hi), np.diff(ptr[lo:hi + 1]))
        sub = rows - ptr[lo:hi][np.repeat(np.arange(hi - lo), np.diff(ptr[lo:hi + 1]))]
        idx = pd.MultiIndex.from_arrays([entry, sub], names=["entry", "subentry"])
        return pd.DataFrame({k: v[rows] for k, v in data.items()}, index=idx)


def _open(path):
    return {"ntupler": {"tree": _Tree(FILES[os.path.abspath(path)])}}


def load_reference(ref_dir):
    stub = types.ModuleType("uproot")
    stub.open = _open
    sys.modules["uproot"] = stub
    sys.path.insert(0, os.path.join(ref_dir, "gnn"))
    import prepareMuonGraphs as ref      # gnn/prepareMuonGraphs.py
    return ref


def run_reference(ref, d, start=0, muon_only=False):
    """prepareMuonGraphs.main() on one (muon, PU) file pair: (graph entries, [(file number, arrays)])."""
    E = d["muon"]["event_ptr"].shape[0] - 1
    vp = {"vp_pt": d["vp_pt"], "vp_eta": d["vp_eta"], "vp_ptr": d["vp_ptr"]}
    entries = []
    orig = ref.construct_graph

    def recording(hits, *a, **k):
        entries.append(int(hits["entry"].iloc[0]))
        return orig(hits, *a, **k)

    with tempfile.TemporaryDirectory() as tmp:
        mdir, pdir, odir = (os.path.join(tmp, s) for s in ("mu", "pu", "out"))
        for dd in (mdir, pdir):
            os.makedirs(dd)
        open(os.path.join(mdir, "mu_SingleMuon_Endcap.root"), "w").close()
        open(os.path.join(pdir, "pu_SingleMuon_Endcap.root"), "w").close()
        FILES[os.path.abspath(os.path.join(mdir, "mu_SingleMuon_Endcap.root"))] = (d["muon"], vp, start)
        FILES[os.path.abspath(os.path.join(pdir, "pu_SingleNeutrino_PU200.root"))] = (d["pu"], vp, start)
        argv = ["prepareMuonGraphs.py", "--input-muon-dir", mdir, "--input-pu-dir", pdir, "--start", str(start),
                "--end", str(start + E), "--output-dir", odir] + (["--muononly", "1"] if muon_only else [])
        saved = sys.argv, ref.construct_graph, ref.plotgraphs
        sys.argv, ref.construct_graph, ref.plotgraphs = argv, recording, (lambda inputdir: None)
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                ref.main()
        finally:
            sys.argv, ref.construct_graph, ref.plotgraphs = saved
        files = []
        for path in sorted(glob.glob(os.path.join(odir, "*.npz"))):
            num = int(os.path.basename(path)[:-4].rsplit("_", 1)[1])
            with np.load(path) as f:
                files.append((num, {k: f[k] for k in f.files}))
    return entries, files


def from_rows(entries_mu, entries_pu):
    """Hand-made entries: lists of (type, station, ring, z, r, phi, tp1, tp2) rows per entry and source."""
    out = {}
    for name, ents in (("muon", entries_mu), ("pu", entries_pu)):
        rows = [r for e in ents for r in e]
        a = np.array(rows, dtype=np.float64).reshape(-1, 8)
        cols = {"vh_type": a[:, 0], "vh_station": a[:, 1], "vh_ring": a[:, 2], "vh_sim_z": a[:, 3],
                "vh_sim_r": a[:, 4], "vh_sim_phi": a[:, 5], "vh_sim_tp1": a[:, 6], "vh_sim_tp2": a[:, 7],
                "vh_sim_theta": np.degrees(np.arctan2(a[:, 4], np.abs(a[:, 3]) + 1.0)),
                "vh_bend": np.arange(a.shape[0]) % 17 - 8}
        out[name] = {k: v.astype(np.int32 if k in synth.EMTF_INT_COLUMNS else np.float32) for k, v in cols.items()}
        out[name]["event_ptr"] = np.concatenate([[0], np.cumsum([len(e) for e in ents])]).astype(np.int64)
    E = len(entries_mu)
    rng = np.random.default_rng(E)
    out["vp_pt"] = rng.uniform(2.0, 50.0, size=E).astype(np.float32)
    out["vp_eta"] = rng.uniform(1.2, 2.4, size=E).astype(np.float32)
    out["vp_ptr"] = np.arange(E + 1, dtype=np.int64)
    return out


def _copy_rows(ent, dr=7.0, dphi=0.01):
    return [(t, s, r, z, rr + dr, p + dphi, 0, 0) for t, s, r, z, rr, p, _, _ in ent]


def cases():
    # 1. seeded events with every rule in play
    yield "default", synth.emtf_events(12, seed=1), 0, False
    # 2. trap 1: z = +0 and -0 (layer 0 nodes no pair uses; np.sign(-0.0) is +0.0), LUT -99 chambers
    d = synth.emtf_events(6, seed=2, p_no_layer=0.15)
    for src in ("muon", "pu"):
        z = d[src]["vh_sim_z"]
        z[1::7] = np.float32(0.0)
        z[4::9] = np.float32(-0.0)
    yield "layer_z0", d, 0, False
    # 3. trap 2: PU entries longer and shorter than the muon entries, many rows without a layer
    yield "cross_filter", synth.emtf_events(10, seed=3, n_pu=14.0, p_no_layer=0.25), 0, False
    # 4. trap 3: entries 1 and 3 lose all muon rows to the truth filter: later ordinals are misaligned and the last
    # PU entries are dropped
    d = synth.emtf_events(8, seed=4)
    ep = d["muon"]["event_ptr"]
    for e in (1, 3):
        d["muon"]["vh_sim_tp1"][ep[e]:ep[e + 1]] = 2
    yield "ordinal", d, 0, False
    # 5. trap 4: up to 6 rows per chamber, duplicates on both z sides
    d = synth.emtf_events(6, seed=5, max_dup=6)
    d["muon"]["vh_sim_z"][2::5] *= -1
    d["pu"]["vh_sim_z"][3::4] *= -1
    yield "duplicates", d, 0, False
    # 6. trap 5: set order 3, 8, 9, 11 -> 8, 9, 3, 11 and -1, -3, -2, -10, -12, 4, 5 -> 4, 5, -12, -10, -2, -3, -1
    e0 = [(1, 1, 1, 602.0, 160.0, 0.1, 0, 0), (1, 2, 1, 830.0, 220.0, 0.11, 0, 0), (1, 3, 1, 935.0, 250.0, 0.12, 0, 0),
          (1, 4, 1, 1025.0, 270.0, 0.13, 0, 0), (1, 1, 4, 600.0, 120.0, 0.1, 0, 0)]
    e1 = [(4, 1, 1, -540.0, 90.0, -3.1, 0, 0), (1, 1, 1, -602.0, 100.0, -3.12, 0, 0),
          (3, 1, 1, -567.0, 95.0, 3.13, 0, 0), (2, 3, 1, -970.0, 160.0, 3.12, 0, 0),
          (2, 4, 1, -1060.0, 175.0, -3.13, 0, 0), (1, 1, 2, 700.0, 300.0, 1.0, 0, 0),
          (2, 1, 2, 705.0, 310.0, 1.01, 0, 0)]
    rest = synth.emtf_events(3, seed=6)
    d = from_rows([e0, e1], [_copy_rows(e0), _copy_rows(e1)])
    yield "set_order", _concat(d, rest), 0, False
    # 7. trap 6: dr = 0 across a pair (equal r on two layers) and dphi across +-pi
    d = synth.emtf_events(6, seed=7)
    for src in ("muon", "pu"):
        c = d[src]
        ep = c["event_ptr"]
        c["vh_sim_r"][ep[0]:ep[1]] = np.float32(250.0)
        p = c["vh_sim_phi"][ep[1]:ep[2]]
        p[0::2] = np.float32(3.14)
        p[1::2] = np.float32(-3.14)
        c["vh_sim_phi"][ep[2]:ep[3]] = np.float32(np.pi)
    yield "segments", d, 0, False
    # 8. trap 8: entry 2 has no vp row and entry 5 two (pt, eta of later graphs shift); entries start at 5
    d = synth.emtf_events(8, seed=8)
    d["vp_ptr"] = np.array([0, 1, 2, 2, 3, 4, 6, 7, 8], np.int64)
    yield "vp_shift", d, 5, False
    # 9. trap 9: an entry with one layer per z side (no pair: no file), an entry whose only pair keeps no segment
    # (dr = 0: a file with zero segments), then seeded entries
    a = [(1, 1, 1, 602.0, 200.0, 0.5, 0, 0), (1, 2, 1, -830.0, 260.0, 0.5, 0, 0)]
    b = [(1, 1, 1, 602.0, 200.0, 0.5, 0, 0), (1, 2, 1, 830.0, 200.0, 0.5, 0, 0)]
    d = from_rows([a, b], [_copy_rows(a, dr=0.0), _copy_rows(b, dr=0.0)])
    yield "no_file", _concat(d, synth.emtf_events(4, seed=9)), 0, False
    # 10. trap 10: --muononly
    yield "muononly", synth.emtf_events(10, seed=10), 0, True
    # 11, 12. the builder's bounds (tests/muon_bound_cases.py): graphs of 42 hits with 6 on a signed layer, 140
    # segments and all 25 layer values, PU rows first and muon rows first; 60 of the set-order entries
    import muon_bound_cases as mb
    by = {c.name: c for c in mb.batch()}
    full = [c.name for c in mb.batch() if c.group in ("full", "neighbours")]
    yield "bounds_full", _bound_entries([by[n] for n in full]), 0, False
    orders = [c for c in mb.batch() if c.group == "explicit" and not c.mu_first]
    seeded = [c for c in mb.batch() if c.group == "orders" and not c.mu_first]
    orders += seeded[::mb.ORDERS_PER_N] + seeded[mb.ORDERS_PER_N * 10 + 1::mb.ORDERS_PER_N]
    assert len(orders) == 60
    yield "bounds_set_order", _bound_entries(orders), 0, False


def _bound_entries(cases):
    mu, pu, vp_pt, vp_eta = __import__("muon_bound_cases").columns([c.rows for c in cases])
    return {"muon": mu, "pu": pu, "vp_pt": vp_pt, "vp_eta": vp_eta,
            "vp_ptr": np.arange(len(cases) + 1, dtype=np.int64)}


def _concat(a, b):
    """Entries of a, then entries of b."""
    out = {}
    for src in ("muon", "pu"):
        out[src] = {k: np.concatenate([a[src][k], b[src][k]]) for k in HIT_FEATURES}
        out[src]["event_ptr"] = np.concatenate([a[src]["event_ptr"], a[src]["event_ptr"][-1] + b[src]["event_ptr"][1:]])
    for k in ("vp_pt", "vp_eta"):
        out[k] = np.concatenate([a[k], b[k]])
    out["vp_ptr"] = np.concatenate([a["vp_ptr"], a["vp_ptr"][-1] + b["vp_ptr"][1:]])
    return out


def pack(d, start, muon_only, entries, files):
    arrays = {"entry_start": np.int64(start), "muon_only": np.bool_(muon_only), "vp_pt": d["vp_pt"],
              "vp_eta": d["vp_eta"], "vp_ptr": d["vp_ptr"], "graph_entry": np.array(entries, np.int64),
              "file_graph": np.array([n for n, _ in files], np.int64)}
    for src, p in (("muon", "mu"), ("pu", "pu")):
        for k in HIT_FEATURES + ("event_ptr",):
            arrays["%s_%s" % (p, k)] = d[src][k]
    for k, (_, f) in enumerate(files):
        for name in ("X", "Ri_rows", "Ri_cols", "Ro_rows", "Ro_cols", "y", "pt", "eta"):
            v = f[name]
            arrays["f%d_%s" % (k, name)] = v.astype(np.int32) if name.endswith(("rows", "cols")) else v
    return arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.path.join(os.path.dirname(REPO), "reference"),
                    help="the reference checkout, its gnn/ directory is imported (default: ../reference beside "
                         "this repository)")
    ap.add_argument("--time", action="store_true", help="also time main() per event on 64 seeded entries")
    args = ap.parse_args()
    import warnings
    warnings.simplefilter("ignore")
    ref = load_reference(args.reference)
    os.makedirs(OUT, exist_ok=True)
    total = 0
    for name, d, start, muon_only in cases():
        entries, files = run_reference(ref, d, start, muon_only)
        path = os.path.join(OUT, name + ".npz")
        write_npz(path, pack(d, start, muon_only, entries, files))
        total += os.path.getsize(path)
        print("%-13s %2d graphs %2d files %5d hits %6d segments %7d bytes" % (
            name, len(entries), len(files), sum(f["X"].shape[0] for _, f in files),
            sum(f["y"].shape[0] for _, f in files), os.path.getsize(path)))
    print("total %d bytes" % total)
    if args.time:
        d = synth.emtf_events(64, seed=11)
        t0 = time.perf_counter()
        entries, _ = run_reference(ref, d)
        dt = time.perf_counter() - t0
        rec = {"what": "reference prepareMuonGraphs.main() on 64 entries of synth.emtf_events(64, seed=11) on the "
                       "host CPU (stand-in uproot, plotting off), per graph",
               "graphs": len(entries), "seconds_total": round(dt, 3), "ms_per_event": round(1e3 * dt / len(entries), 2)}
        with open(os.path.join(OUT, "reference_time.json"), "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        print(rec)


if __name__ == "__main__":
    main()
