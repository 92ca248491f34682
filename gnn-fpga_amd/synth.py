"""Synthetic hit graphs with the shapes of the reference's data products.

No dataset, ROOT file or TrackML CSV is reachable from this build (no network,
`uproot`/`trackml` absent), so inputs are generated with the *schema and
statistics* the reference's data-prep scripts emit:

* `layered_graph`   - TrackML/ACTS barrel style: hits assigned to
  `n_layers` detector layers, every segment joins a hit in layer l to a hit in
  layer l+1 (adjacent-layer rule, reference gnn/prepareGraphs.py:153-155), segments
  emitted grouped by layer pair (as the pd.concat over layer pairs does,
  reference gnn/graph.py:80-93).
* `bipartite_graph` - toy-2D / muon style: complete bipartite segments between
  consecutive occupied layers (reference gnn/Muon_graph.py:60-83 keeps every pair;
  gnn/MPNN_Seg_Toy2D.ipynb: 4 tracks x 10 layers = 40 hits, 144 segments).

Index convention (reference gnn/graph.py:128-135): segment j starts at hit
`src[j]` (the row with Ro[n, j] = 1) and ends at hit `dst[j]` (Ri[n, j] = 1).

Everything is numpy on the host; `numpy.random.default_rng(seed)` only.
"""
from collections import namedtuple

import numpy as np

# X float32 [N, F]; src, dst int32 [E]; y float32 [E] (segment truth label)
HitGraph = namedtuple("HitGraph", ["X", "src", "dst", "y"])

MUON_FEATURES = ("vh_sim_z", "vh_sim_theta", "vh_sim_phi", "vh_sim_r", "vh_bend",
                 "vh_sim_tp1", "vh_sim_tp2", "vh_station", "vh_ring", "vh_type",
                 "vh_layer")  # reference gnn/prepareMuonGraphs.py:169-170 (F = 11)


def layered_graph(n_hits, n_segments, n_features=3, n_layers=10, seed=0,
                  sort_hits_by_layer=False):
    """TrackML-shaped random layered graph: SURVEY.md 8(d) `synth_graph(N,E,F,L,seed)`."""
    if n_hits < n_layers:
        raise ValueError("need at least one hit per layer")
    rng = np.random.default_rng(seed)
    layer = rng.integers(0, n_layers, size=n_hits)
    layer[rng.permutation(n_hits)[:n_layers]] = np.arange(n_layers)  # no empty layer
    if sort_hits_by_layer:
        layer = np.sort(layer)
    X = rng.uniform(-1.0, 1.0, size=(n_hits, n_features)).astype(np.float32)
    hits_of = [np.flatnonzero(layer == l) for l in range(n_layers)]
    n_pairs = n_layers - 1
    per_pair = np.full(n_pairs, n_segments // n_pairs, dtype=np.int64)
    per_pair[: n_segments % n_pairs] += 1
    src = np.empty(n_segments, dtype=np.int32)
    dst = np.empty(n_segments, dtype=np.int32)
    o = 0
    for l in range(n_pairs):
        k = int(per_pair[l])
        src[o:o + k] = rng.choice(hits_of[l], size=k)
        dst[o:o + k] = rng.choice(hits_of[l + 1], size=k)
        o += k
    y = (rng.random(n_segments) < 0.2).astype(np.float32)
    return HitGraph(X, src, dst, y)


def bipartite_graph(hits_per_layer, n_features=2, seed=0):
    """Complete bipartite segments between consecutive layers.

    `hits_per_layer` is a sequence of hit counts, one per occupied layer; hits are
    numbered layer by layer. Toy-2D: [4]*10 -> 40 hits, 144 segments.
    """
    rng = np.random.default_rng(seed)
    hits_per_layer = [int(h) for h in hits_per_layer]
    n_hits = sum(hits_per_layer)
    X = rng.uniform(-1.0, 1.0, size=(n_hits, n_features)).astype(np.float32)
    first = np.concatenate([[0], np.cumsum(hits_per_layer)])
    src, dst = [], []
    for l in range(len(hits_per_layer) - 1):
        a = np.arange(first[l], first[l + 1])
        b = np.arange(first[l + 1], first[l + 2])
        aa, bb = np.meshgrid(a, b, indexing="ij")
        src.append(aa.ravel())
        dst.append(bb.ravel())
    src = np.concatenate(src).astype(np.int32)
    dst = np.concatenate(dst).astype(np.int32)
    y = (rng.random(src.shape[0]) < 0.25).astype(np.float32)
    return HitGraph(X, src, dst, y)


def toy2d_graph(seed=0):
    """gnn/MPNN_Seg_Toy2D.ipynb shape: 40 hits, 144 segments, F = 2."""
    return bipartite_graph([4] * 10, n_features=2, seed=seed)


def muon_graph(seed=0):
    """prepareMuonGraphs.py output shape: tens of hits over a few signed layers, F = 11."""
    rng = np.random.default_rng(1000 + seed)
    n_layers = int(rng.integers(4, 9))
    hits = rng.integers(1, 6, size=n_layers)
    g = bipartite_graph(hits, n_features=len(MUON_FEATURES), seed=seed)
    return g


def to_dense(graph, n_hits_pad=None, n_segments_pad=None, dtype=np.float32):
    """Index form -> the dense one-hot incidence matrices the reference consumes.

    Same fill rule as reference gnn/graph.py:28-35 (`graph_from_sparse`):
    Ri[dst[j], j] = 1, Ro[src[j], j] = 1; padded rows/columns stay zero
    (reference gnn/trainSegmentClassifier.py:83-93).
    """
    n, e = graph.X.shape[0], graph.src.shape[0]
    N = n if n_hits_pad is None else n_hits_pad
    E = e if n_segments_pad is None else n_segments_pad
    X = np.zeros((N, graph.X.shape[1]), dtype=np.float32)
    X[:n] = graph.X
    Ri = np.zeros((N, E), dtype=dtype)
    Ro = np.zeros((N, E), dtype=dtype)
    j = np.arange(e)
    Ri[graph.dst, j] = 1
    Ro[graph.src, j] = 1
    return X, Ri, Ro


# Barrel radii (mm) of the ten layers the reference's TrackML selection keeps (gnn/prepareGraphs.py:56-58: volumes
# 8, 13, 17), rounded.
BARREL_RADII = (32.0, 72.0, 116.0, 172.0, 260.0, 360.0, 500.0, 660.0, 820.0, 1020.0)

# Hit columns as the reference's graph construction consumes them (gnn/prepareGraphs.py:71-86): r, phi, z float32,
# layer int32, particle_id int64; event_ptr int64 [n_events + 1]: event e owns rows [event_ptr[e], event_ptr[e+1]).
HitColumns = namedtuple("HitColumns", ["r", "phi", "z", "layer", "particle_id", "event_ptr"])


def barrel_event(n_tracks, n_noise, n_events=1, seed=0):
    """Detector hits of `n_events` barrel events for graph_build.build_graphs.

    Every track crosses the ten BARREL_RADII on a helix-like path: phi(r) = phi0 + k r with a small
    curvature k, z(r) = z0 + r cot(theta) with z smeared by 0.5 mm, r smeared by 0.1 mm.  `n_noise` noise
    hits per event sit on random layers at random (phi, z) with particle ids -1, -2, ... (every noise hit
    its own id).  Each event's rows are shuffled (frame order is not layer order).
    """
    rng = np.random.default_rng(seed)
    radii = np.asarray(BARREL_RADII)
    n_layers = radii.shape[0]
    cols = {k: [] for k in ("r", "phi", "z", "layer", "particle_id")}
    event_ptr = np.zeros(n_events + 1, dtype=np.int64)
    for e in range(n_events):
        phi0 = rng.uniform(-np.pi, np.pi, size=(n_tracks, 1))
        k = rng.uniform(-4e-4, 4e-4, size=(n_tracks, 1))
        z0 = rng.normal(0.0, 40.0, size=(n_tracks, 1))
        cot = rng.uniform(-1.0, 1.0, size=(n_tracks, 1))
        r = radii[None, :] + rng.normal(0.0, 0.1, size=(n_tracks, n_layers))
        phi = phi0 + k * r
        z = z0 + r * cot + rng.normal(0.0, 0.5, size=(n_tracks, n_layers))
        layer = np.broadcast_to(np.arange(n_layers), (n_tracks, n_layers))
        pid = np.broadcast_to(np.arange(1, n_tracks + 1)[:, None] + e * 1_000_000, (n_tracks, n_layers))
        nl = rng.integers(0, n_layers, size=n_noise)
        r_n = radii[nl] + rng.normal(0.0, 0.1, size=n_noise)
        phi_n = rng.uniform(-np.pi, np.pi, size=n_noise)
        z_n = rng.uniform(-1000.0, 1000.0, size=n_noise)
        R = np.concatenate([r.ravel(), r_n])
        P = np.concatenate([phi.ravel(), phi_n])
        P = np.mod(P + np.pi, 2 * np.pi) - np.pi                  # into [-pi, pi)
        Z = np.concatenate([z.ravel(), z_n])
        L = np.concatenate([layer.ravel(), nl])
        I = np.concatenate([pid.ravel(), -np.arange(1, n_noise + 1)])
        order = rng.permutation(R.shape[0])
        for name, v in (("r", R), ("phi", P), ("z", Z), ("layer", L), ("particle_id", I)):
            cols[name].append(v[order])
        event_ptr[e + 1] = event_ptr[e] + R.shape[0]
    return HitColumns(np.concatenate(cols["r"]).astype(np.float32), np.concatenate(cols["phi"]).astype(np.float32),
                      np.concatenate(cols["z"]).astype(np.float32), np.concatenate(cols["layer"]).astype(np.int32),
                      np.concatenate(cols["particle_id"]).astype(np.int64), event_ptr)


def scores_from_labels(y, seed=0):
    """Seeded float32 stand-ins for a trained classifier's scores, from the segment labels y: true segments score
    0.55 + 0.45 u, fake ones 0.6 u, u uniform in [0, 1) - at threshold 0.5 every true segment passes and one fake
    segment in six.  The recipe the track builder's tests and probe share."""
    y = np.asarray(y).reshape(-1)
    u = np.random.default_rng(seed).random(y.shape[0]).astype(np.float32)
    return np.where(y > 0, 0.55 + 0.45 * u, 0.6 * u).astype(np.float32)


# gnn/MPNN_HitClassifier.ipynb cells 12-15: 10 detector layers x 5 candidate hits per sample (layer-major), the
# segments of every adjacent-layer pair in np.where order, X = [r, phi, z, seed] / (1000, pi, 1000, 1)
HitSamples = namedtuple("HitSamples", ["X", "Ri", "Ro", "y", "src", "dst"])


def hit_classifier_samples(n, seed=0, n_det_layers=10, n_layer_hits=5, n_seed_layers=3):
    """Seeded stand-ins for the notebook's track samples (its ACTS preparation, cells 5-15, needs pandas and the
    dataset).  Per sample one straight-in-(r, z), curving-in-phi track crosses the 10 layers; each layer keeps
    its true hit and the 4 nearest noise hits in (eta, phi), sorted by that distance (the true hit first, as
    cell 15's sort puts it); phi is centred on the first true hit; the last feature is the label on the first
    3 layers (the seed), 0 elsewhere.  Returns HitSamples: X float32 [n, 50, 4], Ri / Ro uint8 [n, 50, 225]
    (Ro = inner hit, Ri = outer hit), y uint8 [n, 50] (hit labels), src / dst int32 [225] (the same segments for
    every sample: the candidate layout is fixed)."""
    rng = np.random.default_rng(seed)
    n_hits = n_det_layers * n_layer_hits
    n_edges = n_layer_hits ** 2 * (n_det_layers - 1)
    layers = np.repeat(np.arange(n_det_layers), n_layer_hits)
    adj = np.stack(np.where((layers[None, :] - layers[:, None]) == 1), axis=1)     # cell 15's adj_idx
    src, dst = adj[:, 0].astype(np.int32), adj[:, 1].astype(np.int32)
    assert src.shape[0] == n_edges
    radii = 32.0 + 72.0 * np.arange(n_det_layers)                                  # mm
    X = np.zeros((n, n_hits, 4), dtype=np.float32)
    y = np.zeros((n, n_hits), dtype=np.uint8)
    for i in range(n):
        eta, phi0, z0 = rng.uniform(-1.5, 1.5), rng.uniform(-np.pi, np.pi), rng.normal(0.0, 50.0)
        curv = rng.uniform(-1e-3, 1e-3)                                            # rad / mm
        phi_ref = phi0 + curv * radii[0]                                           # the first true hit
        for l, r in enumerate(radii):
            z_t = z0 + r * np.sinh(eta)
            phi_t = phi0 + curv * r
            d_eta = rng.normal(0.0, 0.05, size=n_layer_hits - 1)
            d_phi = rng.normal(0.0, 0.05, size=n_layer_hits - 1)
            order = np.argsort(np.hypot(d_eta, d_phi))
            z = np.concatenate([[z_t], r * np.sinh(eta + d_eta[order]) + z0])
            phi = np.concatenate([[phi_t], phi_t + d_phi[order]])
            s = slice(l * n_layer_hits, (l + 1) * n_layer_hits)
            dphi = np.mod(phi - phi_ref + np.pi, 2 * np.pi) - np.pi               # centred on the first true hit
            X[i, s, 0] = r / 1000.0
            X[i, s, 1] = dphi / np.pi
            X[i, s, 2] = z / 1000.0
            y[i, l * n_layer_hits] = 1
        seed_hits = layers < n_seed_layers
        X[i, seed_hits, 3] = y[i, seed_hits]
    edge_idx = np.arange(n_edges)
    Ri = np.zeros((n, n_hits, n_edges), dtype=np.uint8)
    Ro = np.zeros((n, n_hits, n_edges), dtype=np.uint8)
    Ri[:, dst, edge_idx] = 1
    Ro[:, src, edge_idx] = 1
    return HitSamples(X, Ri, Ro, y, src, dst)


# EMTF chambers (vh_type, vh_station, vh_ring) with a LUT layer in gnn/prepareMuonGraphs.py:71-92, and the |z| and
# r range (cm) a hit in them takes here: one endcap's CSC (type 1), RPC (2), GEM (3) and ME0 (4) chambers
EMTF_CHAMBERS = (
    (4, 1, 1, 540.0, 60.0, 150.0), (3, 1, 1, 567.0, 130.0, 260.0), (1, 1, 4, 600.0, 100.0, 150.0),
    (1, 1, 1, 602.0, 150.0, 270.0), (1, 1, 2, 700.0, 275.0, 460.0), (1, 1, 3, 690.0, 505.0, 700.0),
    (2, 1, 2, 705.0, 275.0, 460.0), (3, 2, 1, 795.0, 140.0, 320.0), (2, 2, 2, 800.0, 355.0, 700.0),
    (1, 2, 1, 830.0, 140.0, 350.0), (1, 2, 2, 832.0, 355.0, 700.0), (1, 3, 1, 935.0, 160.0, 350.0),
    (1, 3, 2, 937.0, 355.0, 700.0), (2, 3, 1, 970.0, 160.0, 350.0), (2, 3, 2, 972.0, 355.0, 520.0),
    (2, 3, 3, 974.0, 520.0, 700.0), (1, 4, 1, 1025.0, 180.0, 350.0), (1, 4, 2, 1027.0, 355.0, 700.0),
    (2, 4, 1, 1060.0, 180.0, 350.0), (2, 4, 2, 1062.0, 355.0, 520.0), (2, 4, 3, 1064.0, 520.0, 700.0))
# (type, station, ring) inside the LUT's [0, 5)^3 that it maps to -99: DT chambers, RE1/3, RE2/3
EMTF_NO_LAYER = ((0, 1, 1), (0, 2, 1), (0, 3, 2), (0, 4, 1), (2, 1, 3), (2, 2, 3))
EMTF_INT_COLUMNS = ("vh_bend", "vh_sim_tp1", "vh_sim_tp2", "vh_station", "vh_ring", "vh_type")


def _emtf_rows(rng, entry, chamber, side, r, phi, theta_deg, tp_rate, n_entries):
    """Rows of one source, shuffled within each entry: columns of gnn/prepareMuonGraphs.py:169-170 + event_ptr."""
    n = entry.shape[0]
    ch = np.asarray(EMTF_CHAMBERS + tuple(t + (800.0, 100.0, 700.0) for t in EMTF_NO_LAYER))
    z = side * (ch[chamber, 3] + rng.normal(0.0, 1.0, size=n))
    tp = rng.random(size=(2, n)) < tp_rate
    cols = {"vh_sim_z": z, "vh_sim_theta": theta_deg, "vh_sim_phi": np.mod(phi + np.pi, 2 * np.pi) - np.pi,
            "vh_sim_r": r, "vh_bend": rng.integers(-40, 41, size=n),
            "vh_sim_tp1": np.where(tp[0], rng.integers(1, 4, size=n), 0),
            "vh_sim_tp2": np.where(tp[1], rng.integers(-3, 0, size=n), 0),
            "vh_station": ch[chamber, 1], "vh_ring": ch[chamber, 2], "vh_type": ch[chamber, 0]}
    order = np.lexsort((rng.random(size=n), entry))
    out = {k: (v[order].astype(np.int32) if k in EMTF_INT_COLUMNS else v[order].astype(np.float32))
           for k, v in cols.items()}
    out["event_ptr"] = np.concatenate([[0], np.cumsum(np.bincount(entry, minlength=n_entries))]).astype(np.int64)
    return out


def emtf_events(n_entries, seed=0, n_pu=24.0, p_hit=0.9, max_dup=3, tp_rate=0.08, p_no_layer=0.05):
    """Seeded stand-ins for the EMTF ntuple branches gnn/prepareMuonGraphs.py reads (:169-173), for
    muon_graph.build_muon_graphs: a dict with `muon` and `pu` (the ten hit_features columns - float32 z, theta, phi,
    r; int32 bend, tp1, tp2, station, ring, type - and event_ptr [n_entries + 1]) and `vp_pt`, `vp_eta` (float32,
    one row per entry) with `vp_ptr`.

    Muon entry e: one muon on one z side (eta in [1.2, 2.4], uniform phi) crosses every chamber of EMTF_CHAMBERS
    whose r range holds z tan(theta), with probability p_hit each, and leaves 1 .. max_dup hits per chamber.  A
    fraction tp_rate of the rows has tp1 or tp2 != 0, and p_no_layer of the rows sit in a chamber the LUT maps to
    -99.  PU entry e: Poisson(n_pu) hits in random chambers on either side.  Rows are shuffled within an entry."""
    rng = np.random.default_rng(seed)
    ch = np.asarray(EMTF_CHAMBERS)
    eta = rng.uniform(1.2, 2.4, size=n_entries)
    theta = 2.0 * np.arctan(np.exp(-eta))
    phi0 = rng.uniform(-np.pi, np.pi, size=n_entries)
    side = np.where(rng.random(size=n_entries) < 0.5, -1.0, 1.0)
    r_c = ch[None, :, 3] * np.tan(theta)[:, None]                          # [E, 21]
    inside = (r_c >= ch[None, :, 4]) & (r_c <= ch[None, :, 5]) & (rng.random(size=r_c.shape) < p_hit)
    ndup = np.where(inside, rng.integers(1, max_dup + 1, size=r_c.shape), 0)
    entry = np.repeat(np.repeat(np.arange(n_entries), ch.shape[0]), ndup.ravel())
    chamber = np.repeat(np.tile(np.arange(ch.shape[0]), n_entries), ndup.ravel())
    bad = rng.random(size=entry.shape[0]) < p_no_layer
    chamber = np.where(bad, ch.shape[0] + rng.integers(0, len(EMTF_NO_LAYER), size=entry.shape[0]), chamber)
    n = entry.shape[0]
    r = r_c[entry, np.minimum(chamber, ch.shape[0] - 1)] + rng.normal(0.0, 0.5, size=n)
    muon = _emtf_rows(rng, entry, chamber, side[entry], r, phi0[entry] + rng.normal(0.0, 0.01, size=n),
                      np.degrees(theta[entry]) + rng.normal(0.0, 0.05, size=n), tp_rate, n_entries)
    npu = rng.poisson(n_pu, size=n_entries)
    pe = np.repeat(np.arange(n_entries), npu)
    m = pe.shape[0]
    pch = np.where(rng.random(size=m) < p_no_layer, ch.shape[0] + rng.integers(0, len(EMTF_NO_LAYER), size=m),
                   rng.integers(0, ch.shape[0], size=m))
    lo = np.where(pch < ch.shape[0], ch[np.minimum(pch, ch.shape[0] - 1), 4], 100.0)
    hi = np.where(pch < ch.shape[0], ch[np.minimum(pch, ch.shape[0] - 1), 5], 700.0)
    pr = rng.uniform(lo, hi)
    pside = np.where(rng.random(size=m) < 0.5, -1.0, 1.0)
    pu = _emtf_rows(rng, pe, pch, pside, pr, rng.uniform(-np.pi, np.pi, size=m),
                    np.degrees(np.arctan2(pr, 800.0)), 0.5, n_entries)
    pt = 1.0 / rng.uniform(0.01, 0.5, size=n_entries)
    return {"muon": muon, "pu": pu, "vp_pt": pt.astype(np.float32), "vp_eta": (side * eta).astype(np.float32),
            "vp_ptr": np.arange(n_entries + 1, dtype=np.int64)}


# Raw ACTS cluster columns as gnn/MPNN_Seg_ACTS_fullEvents.ipynb's select_hits (cell 5) takes them: r, phi, z float32,
# volid, layid int32, barcode int64; event_ptr int64 [n_events + 1].  The ten barrel layers as (volid, layid):
ActsColumns = namedtuple("ActsColumns", ["r", "phi", "z", "volid", "layid", "barcode", "event_ptr"])
ACTS_BARREL_LAYERS = ((8, 2), (8, 4), (8, 6), (8, 8), (13, 2), (13, 4), (13, 6), (13, 8), (17, 2), (17, 4))
ACTS_OTHER_VOLUMES = (7, 9, 12, 14, 16, 18)        # endcaps: dropped by the selection


def acts_events(n_events, n_tracks, n_noise, seed=0, missing=0.1, dup=0.05, dup_equal=0.5, non_barrel=0.02):
    """Seeded raw hit columns of `n_events` ACTS-like events for event_graphs.build_event_graphs.

    `n_tracks` and `n_noise` are counts per event, or (lo, hi) ranges drawn per event (hi exclusive).  Tracks cross
    the ten barrel layers as in `barrel_event`; a fraction `missing` of them misses one layer; a fraction `dup` of
    the track hits has a second hit on the same layer, `dup_equal` of those with exactly the same r (the
    deduplication's tie); noise hits sit on random barrel layers with their own negative barcodes, a few of them
    sharing barcode 0; a fraction `non_barrel` of extra rows lies in endcap volumes.  Rows are shuffled per event."""
    rng = np.random.default_rng(seed)
    radii = np.asarray(BARREL_RADII)
    lay_v = np.asarray([v for v, _ in ACTS_BARREL_LAYERS])
    lay_l = np.asarray([l for _, l in ACTS_BARREL_LAYERS])
    L = radii.shape[0]
    draw = lambda v: int(rng.integers(v[0], v[1])) if isinstance(v, (tuple, list)) else int(v)   # noqa: E731
    cols = {k: [] for k in ("r", "phi", "z", "volid", "layid", "barcode")}
    event_ptr = np.zeros(n_events + 1, dtype=np.int64)
    for e in range(n_events):
        nt, nn_ = draw(n_tracks), draw(n_noise)
        phi0 = rng.uniform(-np.pi, np.pi, size=(nt, 1))
        k = rng.uniform(-4e-4, 4e-4, size=(nt, 1))
        z0 = rng.normal(0.0, 40.0, size=(nt, 1))
        cot = rng.uniform(-1.0, 1.0, size=(nt, 1))
        r = radii[None, :] + rng.normal(0.0, 0.1, size=(nt, L))
        phi = phi0 + k * r
        z = z0 + r * cot + rng.normal(0.0, 0.5, size=(nt, L))
        lay = np.broadcast_to(np.arange(L), (nt, L))
        bc = np.broadcast_to(rng.integers(1, 2 ** 40, size=(nt, 1)), (nt, L))
        skip = np.where(rng.random(size=nt) < missing, rng.integers(0, L, size=nt), -1)
        have = (lay != skip[:, None]).ravel()
        R, P, Z, Ly, B = (a.ravel()[have] for a in (r, phi, z, lay, bc))
        d = np.flatnonzero(rng.random(size=R.shape[0]) < dup)
        same = rng.random(size=d.shape[0]) < dup_equal
        nl = rng.integers(0, L, size=nn_)
        nb = -rng.integers(1, 2 ** 40, size=nn_)
        nb[rng.random(size=nn_) < 0.05] = 0
        R = np.concatenate([R, np.where(same, R[d], R[d] + rng.normal(0.0, 0.3, size=d.shape[0])),
                            radii[nl] + rng.normal(0.0, 0.1, size=nn_)])
        P = np.concatenate([P, P[d] + rng.normal(0.0, 1e-3, size=d.shape[0]), rng.uniform(-np.pi, np.pi, size=nn_)])
        Z = np.concatenate([Z, Z[d] + rng.normal(0.0, 0.5, size=d.shape[0]), rng.uniform(-1000.0, 1000.0, size=nn_)])
        Ly = np.concatenate([Ly, Ly[d], nl])
        B = np.concatenate([B, B[d], nb])
        V, Li = lay_v[Ly], lay_l[Ly]
        m = int(rng.binomial(max(R.shape[0], 1), non_barrel))
        R = np.concatenate([R, rng.uniform(30.0, 1000.0, size=m)])
        P = np.concatenate([P, rng.uniform(-np.pi, np.pi, size=m)])
        Z = np.concatenate([Z, rng.uniform(-3000.0, 3000.0, size=m)])
        V = np.concatenate([V, rng.choice(ACTS_OTHER_VOLUMES, size=m)])
        Li = np.concatenate([Li, 2 * rng.integers(1, 7, size=m)])
        B = np.concatenate([B, rng.integers(1, 2 ** 40, size=m)])
        P = np.mod(P + np.pi, 2 * np.pi) - np.pi                  # into [-pi, pi)
        order = rng.permutation(R.shape[0])
        for name, v in (("r", R), ("phi", P), ("z", Z), ("volid", V), ("layid", Li), ("barcode", B)):
            cols[name].append(v[order])
        event_ptr[e + 1] = event_ptr[e] + R.shape[0]
    cat = lambda k, dt: (np.concatenate(cols[k]) if cols[k] else np.zeros(0)).astype(dt)     # noqa: E731
    return ActsColumns(cat("r", np.float32), cat("phi", np.float32), cat("z", np.float32), cat("volid", np.int32),
                       cat("layid", np.int32), cat("barcode", np.int64), event_ptr)


# Raw TrackML event tables as gnn/prepareGraphs.py's select_hits (:53-85) takes them from trackml.dataset.load_event:
# hits (hit_id int32, x, y, z float32, volume_id, layer_id int32), truth (hit_id, particle_id int64) and particles
# (particle_id int64, px, py float32), each a dict of columns plus event_ptr int64 [n_events + 1].
TRACKML_OTHER_LAYERS = ((8, 3), (7, 2), (9, 4), (12, 2), (14, 6), (16, 2), (18, 4))     # dropped by the selection


def trackml_events(n_events, n_tracks, n_noise, seed=0, missing=0.1, dup=0.05, dup_equal=0.5, other=0.05,
                   pt_range=(0.1, 3.0), shared_ids=False, extra_particles=0.1):
    """Seeded raw tables of `n_events` TrackML-like events for select_hits.select_hits: {"hits", "truth", "particles"}.

    Per event `n_tracks` particles (random 48-bit ids, the same in every event with `shared_ids`; pt uniform in
    `pt_range`) cross the ten barrel layers of ACTS_BARREL_LAYERS as in `barrel_event`; a fraction `missing` of them
    misses one layer; a fraction `dup` of the track hits has a second hit on the same layer, `dup_equal` of those at
    exactly the same (x, y), so the same r; `n_noise` noise hits (particle id 0 in truth, no particle row), two of
    them on each barrel layer first, so that no layer of an event is empty; a fraction `other` of extra rows lies on
    (volume, layer) pairs the selection drops, half of them noise, half with a truth particle; a fraction
    `extra_particles` of extra particle rows has no hit.  Hits are shuffled and numbered 1 .. n in the shuffled order
    (hit_ids restart in every event); truth and particles are shuffled separately."""
    rng = np.random.default_rng(seed)
    radii = np.asarray(BARREL_RADII)
    lay_v = np.asarray([v for v, _ in ACTS_BARREL_LAYERS])
    lay_l = np.asarray([l for _, l in ACTS_BARREL_LAYERS])
    oth = np.asarray(TRACKML_OTHER_LAYERS)
    L = radii.shape[0]
    H = {k: [] for k in ("hit_id", "x", "y", "z", "volume_id", "layer_id")}
    T = {k: [] for k in ("hit_id", "particle_id")}
    P = {k: [] for k in ("particle_id", "px", "py")}
    ptr = {k: np.zeros(n_events + 1, dtype=np.int64) for k in ("hits", "truth", "particles")}
    ids0 = None
    for e in range(n_events):
        nt = int(n_tracks)
        ids = rng.permutation(np.unique(rng.integers(1, 2 ** 48, size=2 * nt + 2)))[:nt]
        if shared_ids:
            ids0 = ids if ids0 is None else ids0
            ids = ids0
        phi0 = rng.uniform(-np.pi, np.pi, size=(nt, 1))
        k = rng.uniform(-4e-4, 4e-4, size=(nt, 1))
        z0 = rng.normal(0.0, 40.0, size=(nt, 1))
        cot = rng.uniform(-1.0, 1.0, size=(nt, 1))
        r = radii[None, :] + rng.normal(0.0, 0.1, size=(nt, L))
        phi = phi0 + k * r
        z = z0 + r * cot + rng.normal(0.0, 0.5, size=(nt, L))
        lay = np.broadcast_to(np.arange(L), (nt, L))
        pid = np.broadcast_to(ids[:, None], (nt, L))
        skip = np.where(rng.random(size=nt) < missing, rng.integers(0, L, size=nt), -1)
        have = (lay != skip[:, None]).ravel()
        R, F, Z, Ly, I = (a.ravel()[have] for a in (r, phi, z, lay, pid))
        d = np.flatnonzero(rng.random(size=R.shape[0]) < dup)
        same = rng.random(size=d.shape[0]) < dup_equal
        nn_ = int(n_noise)
        nl = np.concatenate([np.repeat(np.arange(L), 2), rng.integers(0, L, size=max(nn_ - 2 * L, 0))])[:max(nn_, 0)]
        R = np.concatenate([R, np.where(same, R[d], R[d] + rng.normal(0.0, 0.3, size=d.shape[0])),
                            radii[nl] + rng.normal(0.0, 0.1, size=nl.shape[0])])
        F = np.concatenate([F, np.where(same, F[d], F[d] + rng.normal(0.0, 1e-3, size=d.shape[0])),
                            rng.uniform(-np.pi, np.pi, size=nl.shape[0])])
        Z = np.concatenate([Z, Z[d] + rng.normal(0.0, 0.5, size=d.shape[0]),
                            rng.uniform(-1000.0, 1000.0, size=nl.shape[0])])
        Ly = np.concatenate([Ly, Ly[d], nl])
        I = np.concatenate([I, I[d], np.zeros(nl.shape[0], dtype=np.int64)])
        V, Li = lay_v[Ly], lay_l[Ly]
        m = int(rng.binomial(max(R.shape[0], 1), other))
        pick = rng.integers(0, oth.shape[0], size=m)
        R = np.concatenate([R, rng.uniform(30.0, 1000.0, size=m)])
        F = np.concatenate([F, rng.uniform(-np.pi, np.pi, size=m)])
        Z = np.concatenate([Z, rng.uniform(-3000.0, 3000.0, size=m)])
        V = np.concatenate([V, oth[pick, 0]])
        Li = np.concatenate([Li, oth[pick, 1]])
        I = np.concatenate([I, np.where(rng.random(size=m) < 0.5, 0, ids[rng.integers(0, nt, size=m)] if nt else 0)])
        n = R.shape[0]
        order = rng.permutation(n)
        X, Y = (R * np.cos(F))[order], (R * np.sin(F))[order]
        H["hit_id"].append(np.arange(1, n + 1))
        for name, v in (("x", X), ("y", Y), ("z", Z[order]), ("volume_id", V[order]), ("layer_id", Li[order])):
            H[name].append(v)
        to = rng.permutation(n)
        T["hit_id"].append(np.arange(1, n + 1)[to])
        T["particle_id"].append(I[order][to])
        nx = int(round(extra_particles * nt))
        extra = -rng.permutation(np.arange(1, nx + 1))                   # (ids no track has)
        pt = rng.uniform(pt_range[0], pt_range[1], size=nt + nx)
        ang = rng.uniform(-np.pi, np.pi, size=nt + nx)
        po = rng.permutation(nt + nx)
        P["particle_id"].append(np.concatenate([ids, extra])[po])
        P["px"].append((pt * np.cos(ang))[po])
        P["py"].append((pt * np.sin(ang))[po])
        ptr["hits"][e + 1] = ptr["hits"][e] + n
        ptr["truth"][e + 1] = ptr["truth"][e] + n
        ptr["particles"][e + 1] = ptr["particles"][e] + nt + nx
    cat = lambda d, k, dt: (np.concatenate(d[k]) if d[k] else np.zeros(0)).astype(dt)     # noqa: E731
    hits = {"hit_id": cat(H, "hit_id", np.int32), "x": cat(H, "x", np.float32), "y": cat(H, "y", np.float32),
            "z": cat(H, "z", np.float32), "volume_id": cat(H, "volume_id", np.int32),
            "layer_id": cat(H, "layer_id", np.int32), "event_ptr": ptr["hits"]}
    truth = {"hit_id": cat(T, "hit_id", np.int64), "particle_id": cat(T, "particle_id", np.int64),
             "event_ptr": ptr["truth"]}
    particles = {"particle_id": cat(P, "particle_id", np.int64), "px": cat(P, "px", np.float32),
                 "py": cat(P, "py", np.float32), "event_ptr": ptr["particles"]}
    return {"hits": hits, "truth": truth, "particles": particles}


# ---- the toy notebooks' graphs (gnn/GCN_Seg_Toy2D.ipynb, gnn/GCN_Toy2D.ipynb): straight 2D tracks through ten detector
# layers, for the graph-convolution classifiers of gcn.py ---------------------------------------------------------------
TOY_DET_R = (0.0, 1.0, 2.0, 3.0, 5.0, 7.0, 9.0, 11.0, 13.0, 15.0)


def _toy_tracks(rng, n_events, n_tracks, det_r):
    """[n_events, n_tracks, n_layers] float32 hit positions of straight tracks entering and leaving inside (0, 1)."""
    xin = rng.uniform(size=(n_events, n_tracks)).astype(np.float32)
    xout = rng.uniform(size=(n_events, n_tracks)).astype(np.float32)
    slope = (xout - xin) / np.float32(det_r[-1] - det_r[0])
    return slope[:, :, None] * det_r[None, None, :] + xin[:, :, None]


def toy_segment_graphs_from_hits(hit_x, hit_y, det_r=TOY_DET_R, sigma=0.01):
    """The segment graphs of GCN_Seg_Toy2D.ipynb (cells 10-17 and 24) from hits sorted within each layer: hit_x, hit_y
    [n_events, n_layers * n_tracks] (layer-major; positions and track labels).

    A segment joins a hit to a hit of the next layer; segment (l, a, b) = hit a of layer l to hit b of layer l + 1 has
    index (l T + a) T + b, the order cell 10's np.triu(...).nonzero() gives.  Two segments are adjacent when one ends
    where the other starts (cell 12's triple loop, here an index comparison), weighted by a Gaussian of their slope
    difference (cell 17, float32).  Returns X [E, S, 5] = (x0, x1, r0, r1, slope), A [E, S, S], y [E, S], float32;
    a row of A has at most 2 T non-zeros."""
    det_r = np.asarray(det_r, dtype=np.float32)
    L = det_r.shape[0]
    E = hit_x.shape[0]
    T = hit_x.shape[1] // L
    lay, a, b = np.meshgrid(np.arange(L - 1), np.arange(T), np.arange(T), indexing="ij")
    h0 = (lay * T + a).ravel()                       # first hit of each segment
    h1 = ((lay + 1) * T + b).ravel()                 # second hit
    hit_r = np.repeat(det_r, T)
    seg_x = np.stack([hit_x[:, h0], hit_x[:, h1]], axis=-1).astype(np.float32)
    seg_r = np.broadcast_to(np.stack([hit_r[h0], hit_r[h1]], axis=-1)[None], seg_x.shape).astype(np.float32)
    slope = (seg_x[:, :, 1] - seg_x[:, :, 0]) / (seg_r[:, :, 1] - seg_r[:, :, 0])
    y = (hit_y[:, h0] == hit_y[:, h1]).astype(np.float32)
    fwd = h1[:, None] == h0[None, :]                 # segment i ends where segment j starts
    adj = (fwd | fwd.T).astype(np.float32)
    dslope = slope[:, None, :] - slope[:, :, None]
    kern = np.exp(-(dslope ** 2) / np.float32(2 * sigma ** 2)).astype(np.float32)
    X = np.concatenate([seg_x, seg_r, slope[:, :, None]], axis=-1).astype(np.float32)
    return X, (adj[None] * kern).astype(np.float32), y.reshape(E, h0.shape[0])


def toy_segment_graphs(n_events, seed=0, n_tracks=5, det_r=TOY_DET_R, sigma=0.01):
    """Seeded inputs of GCN_Seg_Toy2D.ipynb (cells 3, 4, 10-17, 24) without its Python triple loop: n_tracks straight
    tracks per event, hits sorted within each layer, all 225 (at the defaults) layer-to-next-layer segments.
    Returns (X [E, 225, 5], A [E, 225, 225] the kernel-weighted segment adjacency, y [E, 225]), float32."""
    rng = np.random.default_rng(seed)
    r = np.asarray(det_r, dtype=np.float32)
    tracks = _toy_tracks(rng, n_events, n_tracks, r).transpose(0, 2, 1)        # [E, L, T]
    order = np.argsort(tracks, axis=-1)
    x = np.take_along_axis(tracks, order, axis=-1)
    return toy_segment_graphs_from_hits(x.reshape(n_events, -1), order.reshape(n_events, -1), det_r, sigma)


def toy_hit_graphs_from_hits(hit_x, hit_y, det_r=TOY_DET_R, seed_size=3, norm="row", target=0):
    """The hit graphs of GCN_Toy2D.ipynb (cells 8 and 17 with cell 4's calc_adjacency, norm_adjacency and
    kwnorm_adjacency) from hits sorted within each layer: hit_x float64 (float32 is widened exactly), hit_y
    [n_events, n_layers * n_tracks] (layer-major; positions and track labels).  Returns what `toy_hit_graphs`
    documents, with track `target` as the target track: (X, A, y0)."""
    if norm not in (None, "row", "kw"):
        raise ValueError("norm must be None, 'row' or 'kw'")
    det = np.asarray(det_r, dtype=np.float64)
    L = det.shape[0]
    x = np.asarray(hit_x).astype(np.float64)
    y = np.asarray(hit_y)
    n_tracks = x.shape[1] // L
    r = np.broadcast_to(np.repeat(det, n_tracks)[None], x.shape)
    lay = np.broadcast_to(np.repeat(np.arange(L), n_tracks)[None], x.shape)
    y0 = (y == target).astype(np.float32)
    X = np.stack([x, r / det.max(), np.where(lay < seed_size, y0, 0.0)], axis=-1).astype(np.float32)
    adj_l = np.abs(lay[:, None, :] - lay[:, :, None]) == 1
    dx = x[:, None, :] - x[:, :, None]
    dr = r[:, None, :] - r[:, :, None]
    dr = np.where(dr == 0, 1e-7, dr)
    slope = dx / dr
    x0 = x[:, None, :] - slope * r[:, None, :]
    xn = x[:, None, :] + slope * (det.max() - r[:, None, :])
    a = (adj_l & (x0 < 1) & (x0 > 0) & (xn < 1) & (xn > 0)).astype(np.float64)
    if norm == "row":
        s = a.sum(axis=1)
        a = np.where(s > 0, 1.0 / np.where(s > 0, s, 1.0), 0.0)[:, :, None] * a
    elif norm == "kw":
        ahat = np.eye(a.shape[1])[None] + a
        d = 1.0 / np.sqrt(ahat.sum(axis=1))
        a = d[:, :, None] * ahat * d[:, None, :]
    return X, a.astype(np.float32), y0


def toy_hit_graphs(n_events, seed=0, n_tracks=4, seed_size=3, norm="row", det_r=TOY_DET_R):
    """Seeded inputs of GCN_Toy2D.ipynb (cells 4, 8, 17): hit graphs of n_tracks straight tracks, hits sorted within
    each layer.  X [E, 40, 3] = (x, r / r_max, seed: the target-track flag on the first seed_size layers), y [E, 40] =
    hit is on track 0, and A [E, 40, 40]: hits of adjacent layers whose connecting line enters and leaves inside
    (0, 1), with `norm` = None (binary), "row" (norm_adjacency: row i divided by sum_k a[k, i]; NOT symmetric) or
    "kw" (kwnorm_adjacency: D (I + a) D with D = diag(1 / sqrt(sum_k (I + a)[k, i])); has a diagonal).

    A hit with no neighbour keeps a ZERO row under "row"; the notebook writes NaN there (1 / 0 times 0), which the
    compressed adjacency refuses."""
    if norm not in (None, "row", "kw"):
        raise ValueError("norm must be None, 'row' or 'kw'")
    rng = np.random.default_rng(seed)
    det = np.asarray(det_r, dtype=np.float64)
    tracks = _toy_tracks(rng, n_events, n_tracks, det.astype(np.float32)).astype(np.float64).transpose(0, 2, 1)
    order = np.argsort(tracks, axis=-1)
    x = np.take_along_axis(tracks, order, axis=-1).reshape(n_events, -1)
    return toy_hit_graphs_from_hits(x, order.reshape(n_events, -1), det_r, seed_size, norm)


def toy_tracks(n_events, n_tracks, seed=0, det_r=TOY_DET_R):
    """Seeded [n_events, n_tracks, n_layers] float32 positions of straight tracks (gen_tracks of both notebooks' cell
    3 / 4, with numpy's Generator): what toy_graphs.sort_toy_tracks starts from."""
    return _toy_tracks(np.random.default_rng(seed), n_events, n_tracks, np.asarray(det_r, dtype=np.float32))


# ---- the toy MPNN notebook's inputs (gnn/MPNN_Seg_Toy2D.ipynb cells 8, 11, 12), for toy_mpnn.py -------------------------
def toy_mpnn_segments(n_layers, n_tracks):
    """(src, dst) int64 [T^2 (L - 1)] of ONE event, hits layer-major: every hit of a layer to every hit of the next,
    in the order cell 11's np.where(d == 1) gives - segment (l T + a) T + b joins hit l T + a to hit (l + 1) T + b."""
    lay, a, b = np.meshgrid(np.arange(n_layers - 1), np.arange(n_tracks), np.arange(n_tracks), indexing="ij")
    return (lay * n_tracks + a).ravel().astype(np.int64), ((lay + 1) * n_tracks + b).ravel().astype(np.int64)


def toy_mpnn_graphs_from_hits(hit_x, hit_y, det_r=TOY_DET_R):
    """The numpy specification of toy_mpnn.build_toy_mpnn_graphs: hit_x, hit_y [E, L * T] (layer-major, sorted within
    each layer) -> X [E, L T, 2] = (x, r) float32 (cell 12), src, dst [S] of one event (cell 11; every event has the
    same), y [E, S] float32 = the segment's two hits carry the same label (cell 12's ey)."""
    det = np.asarray(det_r, dtype=np.float64)
    L = det.shape[0]
    hit_x = np.asarray(hit_x)
    T = hit_x.shape[1] // L
    src, dst = toy_mpnn_segments(L, T)
    r = np.broadcast_to(np.repeat(det, T)[None], hit_x.shape)
    X = np.stack([hit_x.astype(np.float64), r], axis=-1).astype(np.float32)
    hit_y = np.asarray(hit_y)
    return X, src, dst, (hit_y[:, src] == hit_y[:, dst]).astype(np.float32)
