"""Hand-built entries that put the muon graph builder (csrc/muon_graph.hip) at the bounds its kernels are written
for: 42 hits per graph, 6 hits on one signed layer, 25 distinct signed-layer values (CPython's set table at 8, 32 and
128 slots), more than two ballot rounds of candidates, raw rows at and around the 64-lane chunks of k_mg_entry, and
cut values on and beside f32(10e30).  Nothing is drawn from synth: every entry is a list of rows per source, written
so that the cross-frame filter, the truth filter and the deduplication leave exactly the hits the case names.

One batch holds every case (`batch()`), so a test builds it once per layout.  The cases before the 1-hit entry have
their PU rows first in the graph; that entry has PU rows only, so in every later entry the muon ordinal is behind the
PU ordinal and the muon rows come first (prepareMuonGraphs.py:193-232): the later block repeats the layer-list, full,
streaming and a part of the set-order cases that way.  The last entry loses its PU rows to the same rule.

Geometry: hit k of an entry has r = 100 + 3 k, so no two hits share r and every candidate of a layer pair is kept
(only the cut cases choose r, phi and z themselves).  Then the kept segments of a graph are its candidates T, and a
pair's first segment names the pair.

`lane0` restates what lane 0 of k_mg_pairs and the ballot rounds after it do, on plain lists, with switches for three
plausible defects; tests/test_muon_bounds_host.py shows which cases see each.
"""
import functools
import random

import numpy as np

from gnn_fpga_amd import muon_graph as mg
from gnn_fpga_amd.graph_build import wrap_dphi32

CUT = mg._CUT32                                            # f32(10e30), the specification's own scalar
CHAMBERS = {}                                              # layer -> its (type, station, ring), in LUT order
for _k, _v in mg.EMTF_LUT.items():
    CHAMBERS.setdefault(_v, []).append(_k)
NO_LAYER = (0, 0, 0)                                       # a chamber the LUT maps to -99
CAPACITY = {L: 2 * len(c) for L, c in CHAMBERS.items()}    # hits one layer can hold: chambers x 2 sources
WAVE = 64


# ---- rows ------------------------------------------------------------------------------------------------------------
def row(ch, z, r, phi, tp1=0, tp2=0):
    return (ch[0], ch[1], ch[2], z, r, phi, tp1, tp2)


def columns(entries):
    """(muon, pu, vp_pt, vp_eta) of a list of (muon rows, PU rows): host columns as build_muon_graphs takes them."""
    out = []
    for k in (0, 1):
        rows = [r for e in entries for r in e[k]]
        a = np.array(rows, dtype=np.float64).reshape(-1, 8)
        f32 = np.array([[r[3], r[4], r[5]] for r in rows], dtype=np.float32).reshape(-1, 3)   # (no float64 detour)
        c = {"vh_type": a[:, 0].astype(np.int32), "vh_station": a[:, 1].astype(np.int32),
             "vh_ring": a[:, 2].astype(np.int32), "vh_sim_z": f32[:, 0].copy(), "vh_sim_r": f32[:, 1].copy(),
             "vh_sim_phi": f32[:, 2].copy(), "vh_sim_tp1": a[:, 6].astype(np.int32),
             "vh_sim_tp2": a[:, 7].astype(np.int32),
             "vh_sim_theta": (np.abs(a[:, 5]) * 20.0 + 0.25).astype(np.float32),      # (of the row's own values:
             "vh_bend": (np.floor(np.abs(a[:, 4]) * 4.0) % 17 - 8).astype(np.int32),   # an entry alone builds the same)
             "event_ptr": np.concatenate([[0], np.cumsum([len(e[k]) for e in entries])]).astype(np.int64)}
        out.append(c)
    E = len(entries)
    vp_pt, vp_eta = (2.0 + 0.5 * np.arange(E)).astype(np.float32), (1.2 + 0.001 * np.arange(E)).astype(np.float32)
    return out[0], out[1], vp_pt, vp_eta


def _z(v, k):
    """A z whose sign gives the signed layer v (v = 0: +0.0 and -0.0 in turn; np.sign of either is +0.0)."""
    if v == 0:
        return -0.0 if k & 1 else 0.0
    return (500.0 + 40.0 * abs(v)) * (1.0 if v > 0 else -1.0)


def realise(first, second, mu_first):
    """(muon rows, PU rows) of an entry whose graph holds hits of the signed layers `first` (the source that comes
    first in the graph) then `second`, in that order.  Each source uses a chamber once (the deduplication); a 0 takes
    a chamber no other hit of its source needs.  The shorter source is filled up to the longer one's row count with
    rows that do not survive: PU rows of a chamber it already has (on the other z side), muon rows with tp1 or tp2
    set.  ValueError where a source has not the chambers."""
    if not first or not second:
        raise ValueError("both sources need a hit (the cross-frame filter pairs their rows)")
    rows, k = [], 0
    for vals in (first, second):
        used, chosen = set(), []
        for v in vals:
            if v != 0:
                free = [c for c in CHAMBERS[abs(v)] if c not in used]
                if not free:
                    raise ValueError("no chamber left for layer %d" % v)
                used.add(free[0])
                chosen.append(free[0])
            else:
                chosen.append(None)
        need = {L: sum(1 for v in vals if abs(v) == L) for L in CHAMBERS}
        for i, v in enumerate(vals):
            if v == 0:
                free = [c for L in sorted(CHAMBERS, key=lambda L: need[L] - len(CHAMBERS[L])) for c in CHAMBERS[L]
                        if c not in used]
                if not free:
                    raise ValueError("no chamber left for a z = 0 hit")
                used.add(free[0])
                chosen[i] = free[0]
        src = []
        for v, c in zip(vals, chosen):
            src.append(row(c, _z(v, k), 100.0 + 3.0 * k, 0.05 + 0.002 * k))
            k += 1
        rows.append(src)
    mu, pu = (rows[0], rows[1]) if mu_first else (rows[1], rows[0])
    n = max(len(mu), len(pu))
    for j in range(len(mu), n):                    # truth-filtered rows, of any chamber with a layer
        mu.append(row(CHAMBERS[12][j % 3], 1040.0, 400.0 + j, 1.0, tp1=1 - j % 2, tp2=j % 2))
    for j in range(len(pu), n):                    # duplicates of the PU source's first chamber, other z side
        pu.append(row(pu[0][:3], -pu[0][3] if pu[0][3] != 0 else 7.0, 500.0 + j, 2.0))
    return mu, pu


class Case:
    """One entry: its rows, the signed layers of its graph's hits in frame order (None where the case does not say),
    and which source comes first."""

    def __init__(self, name, group, mu_rows, pu_rows, layers=None, mu_first=False, expect=None):
        self.name, self.group, self.rows, self.layers, self.mu_first = name, group, (mu_rows, pu_rows), layers, mu_first
        self.expect = expect                       # set order stated as a literal (explicit orders only)


def _ordered(name, group, first, second, mu_first, expect=None):
    mu, pu = realise(list(first), list(second), mu_first)
    return Case(name, group, mu, pu, [float(v) for v in list(first) + list(second)], mu_first, expect)


# ---- set order -------------------------------------------------------------------------------------------------------
ORDERS_PER_N = 40


@functools.lru_cache(maxsize=None)
def seeded_orders():
    """For n = 1 .. 25 distinct signed layers, ORDERS_PER_N seeded (first, second) hit sequences whose first
    occurrences are a random order of n values of -12 .. 12, 0 allowed; half of them with hits after or between that
    repeat a value.  Orders the chambers cannot give (both signs of a one-chamber layer in one source) are drawn
    again."""
    out = []
    for n in range(1, 26):
        rng = random.Random(1000 + n)
        got = 0
        while got < ORDERS_PER_N:
            vals = rng.sample(range(-12, 13), n)
            a = rng.randint(1, max(1, n - 1))
            first, second = vals[:a], vals[a:]
            if rng.random() < 0.5 or not second:
                dup = [v for v in vals if rng.random() < 0.4] or [vals[-1]]
                rng.shuffle(dup)
                cut = rng.randint(0, len(second))
                second = second[:cut] + dup[:3] + second[cut:]
            try:
                realise(first, second, False)
            except ValueError:
                continue
            out.append((n, tuple(first), tuple(second)))
            got += 1
    return tuple(out)


# 16 distinct values one source can hold beside those of the one-chamber layers 1 and 2
_16 = (3, 4, 8, 9, 10, 11, 12, -3, -4, -8, -9, -11, -12, 5, 6, 7)
# (name, first, second, list(set(hit layers)) as the interpreter gives it); LITERALS below
EXPLICIT_HITS = (
    # hash(-1) == -2: the two collide in every table, and the later one is placed by perturbed probing
    ("m1_m2", (-1, -2), (-2,)),
    ("m2_m1", (-2, -1), (-1,)),
    ("m1_m2_in_32", (-1, -2, 3, 4, 5, -10, -9), (-8, -7)),
    ("m2_m1_in_32", (-2, -1, 3, 4, 5, -10, -9), (-8, -7)),
    ("m1_m2_in_128", _16 + (-1, -2), (1, 2, -10, 0)),
    ("m2_m1_in_128", _16 + (-2, -1), (1, 2, -10, 0)),
    # congruent mod 8, back to back: 4, 12, -4, -12 all start at slot 4 of the 8-slot table, 1, 9, -7 at slot 1
    ("mod8_slot4", (4, 12, -4, -12), (-12,)),
    ("mod8_slot1", (1, 9, -7), (9, -7)),
    ("mod8_both", (4, 12, 1, 9), (-4, -7, -12)),
    # congruent mod 32 and mod 128: only hash(-1) == hash(-2) is; the displaced one lands on slot 22 (118) = -10's
    # slot, so -10 and then -9, -8 are placed by LINEAR probing, the only way a table of 32 or 128 gets there
    ("mod32_chain", (-2, -1, 5, 6, 7, -10, -9, -8), (-7, -6)),
    ("mod32_chain_rev", (-1, -2, 5, 6, 7, -8, -9, -10), (-6, -7)),
    ("mod128_chain", _16 + (1, 2), (-2, -1, -10, -5, -6)),
    # the 5th and the 19th distinct value as the last hit: the table grows and nothing comes after
    ("grow5_last", (1, 2, 3, 4), (5,)),
    ("grow5_last_neg", (-1, -2, -3, 12), (-3, 12, -12)),
    ("grow19_last", _16 + (1, 2), (3, 4, -7)),
    ("grow19_last_zero", _16 + (1, 2), (8, 9, 0)),
    # the 5th and the 19th distinct value as the first hit after a run of hits that repeat a value
    ("grow5_after_run", (1, 2, 3, 4), (4, 3, 2, 1, 12, 11)),
    ("grow5_after_run_neg", (-2, -1, 10, 12), (-2, -1, 10, 12, 10, 12, -12, 11)),
    ("grow19_after_run", _16 + (1, 2), (12, 11, 10, 9, 8, 4, 3, -10, -7)),
    ("grow19_after_run_dup", _16 + (1, 2), (1, 2, 3, 4, 8, 9, 10, 11, 12, 10, 12, -10, -5)),
)
_P = [float(v) for v in range(1, 13)]
LITERALS = {
    "m1_m2": [-1.0, -2.0],
    "m2_m1": [-2.0, -1.0],
    "m1_m2_in_32": [3.0, 4.0, 5.0, -9.0, -2.0, -10.0, -8.0, -7.0, -1.0],
    "m2_m1_in_32": [3.0, 4.0, 5.0, -9.0, -1.0, -10.0, -8.0, -7.0, -2.0],
    "m1_m2_in_128": [0.0] + _P + [-12.0, -11.0, -1.0, -9.0, -8.0, -10.0, -4.0, -3.0, -2.0],
    "m2_m1_in_128": [0.0] + _P + [-12.0, -11.0, -2.0, -9.0, -8.0, -10.0, -4.0, -3.0, -1.0],
    "mod8_slot4": [-4.0, -12.0, 4.0, 12.0],
    "mod8_slot1": [1.0, -7.0, 9.0],
    "mod8_both": [1.0, 4.0, 9.0, 12.0, -12.0, -7.0, -4.0],
    "mod32_chain": [5.0, 6.0, 7.0, -9.0, -1.0, -10.0, -8.0, -7.0, -6.0, -2.0],
    "mod32_chain_rev": [5.0, 6.0, 7.0, -2.0, -9.0, -8.0, -10.0, -6.0, -7.0, -1.0],
    "mod128_chain": _P + [-12.0, -11.0, -1.0, -9.0, -8.0, -10.0, -6.0, -5.0, -4.0, -3.0, -2.0],
    "grow5_last": [1.0, 2.0, 3.0, 4.0, 5.0],
    "grow5_last_neg": [12.0, -12.0, -2.0, -3.0, -1.0],
    "grow19_last": _P + [-12.0, -11.0, -9.0, -8.0, -7.0, -4.0, -3.0],
    "grow19_last_zero": [0.0] + _P + [-12.0, -11.0, -9.0, -8.0, -4.0, -3.0],
    "grow5_after_run": [1.0, 2.0, 3.0, 4.0, 11.0, 12.0],
    "grow5_after_run_neg": [10.0, 11.0, 12.0, -12.0, -1.0, -2.0],
    "grow19_after_run": _P + [-12.0, -11.0, -10.0, -9.0, -8.0, -7.0, -4.0, -3.0],
    "grow19_after_run_dup": _P + [-12.0, -11.0, -10.0, -9.0, -8.0, -5.0, -4.0, -3.0],
}
EXPLICIT = tuple((n, f, s, LITERALS[n]) for n, f, s in EXPLICIT_HITS)


def expected_order(case):
    """The interpreter's own list(set(...)) of the graph's signed layers (float64, in frame order)."""
    return list(set(case.layers))


def pairs_of_segments(layer, src, dst):
    """The layer pairs in the order their segment blocks come: (layer of src, layer of dst) of every block's first
    segment.  Every pair of these cases keeps all its candidates."""
    out = []
    for s, d in zip(src, dst):
        p = (float(layer[s]), float(layer[d]))
        if not out or out[-1] != p:
            out.append(p)
    return out


# ---- full graphs -----------------------------------------------------------------------------------------------------
ALL_CHAMBERS = tuple(c for L in sorted(CHAMBERS) for c in CHAMBERS[L])       # 21, ascending layer


def full_entry(signs, mu_first=False, zero=()):
    """Both sources hold all 21 chambers once: 42 hits.  signs[k] (+1 / -1) is the z side of hit k in frame order
    (first source's chambers in ascending layer, then the second's); hits in `zero` have z = +-0."""
    vals = [0 if k in zero else s * mg.EMTF_LUT[ALL_CHAMBERS[k % 21]] for k, s in enumerate(signs)]
    return vals[:21], vals[21:]


def candidates(layers):
    """T of a graph with these signed layers: the sum over the layer pairs of (l1 hits) x (l2 hits)."""
    n = {}
    for v in layers:
        n[v] = n.get(v, 0) + 1
    return sum(n[a] * n[b] for a, b in mg.layer_pairs(mg.set_order(layers)))


def _signs_six_six(side):
    """6 hits on side * 10 and 6 on side * 12, the rest on the other side."""
    one = [side if mg.EMTF_LUT[c] in (10, 12) else -side for c in ALL_CHAMBERS]
    return one + one


def _signs_most_distinct():
    """All 24 non-zero values: a layer's hits of the first source on +, of the second on -; one hit of layer 10 (6
    hits, two to spare) has z = 0 for the 25th."""
    return [1] * 21 + [-1] * 21


# The sign assignment with the most candidates, found by search_most_segments() (an exhaustive search over the side of
# every layer as a whole, then single-hit flips until none gains): every hit on one side.  T = 140.
SIGNS_MOST_SEGMENTS = (1,) * 42


def search_most_segments():
    """Every assignment of whole layers to a side (2^12), scored by `candidates` (set_order and layer_pairs of the
    specification); then single-hit flips from the best until none gains.  Returns (T, signs)."""
    layer_of = [mg.EMTF_LUT[ALL_CHAMBERS[k % 21]] for k in range(42)]
    best = (-1, None)
    for bits in range(1 << 12):
        signs = [1 if bits >> (L - 1) & 1 else -1 for L in layer_of]
        t = candidates([float(s * L) for s, L in zip(signs, layer_of)])
        if t > best[0]:
            best = (t, signs)
    t, signs = best
    gained = True
    while gained:
        gained = False
        for k in range(42):
            trial = list(signs)
            trial[k] = -trial[k]
            tt = candidates([float(s * L) for s, L in zip(trial, layer_of)])
            if tt > t:
                t, signs, gained = tt, trial, True
    return t, tuple(signs)


# ---- layer lists -----------------------------------------------------------------------------------------------------
def layer_list_cases(mu_first, tag):
    """Exactly 5 and exactly 6 hits on +10 (and on -12), the partner layer of the pair with 1, 5 and 6."""
    out = []
    for n1 in (5, 6):
        for n2 in (1, 5, 6):
            for l1, l2 in ((10, 12), (-10, -12)):
                # the hits alternate between the layers inside each source, so list order is not hit order
                a, b = [l1] * min(n1, 3), [l2] * min(n2, 3)
                first = [v for p in zip(a, b + [None] * 3) for v in p if v is not None] + b[len(a):]
                a, b = [l1] * (n1 - 3), [l2] * (n2 - min(n2, 3))
                second = b + a
                if not second:
                    continue
                out.append(_ordered("list_%d_%d_%s%s" % (n1, n2, "p" if l1 > 0 else "m", tag), "lists", first, second,
                                    mu_first))
    return out


# ---- streaming and deduplication -------------------------------------------------------------------------------------
def _raw(rng, n, chambers, p_none=0.1, p_tp=0.3):
    """n raw rows per source of random chambers (a few without a layer), sides and truth flags."""
    mu, pu = [], []
    for s in range(n):
        for rows, tp in ((mu, p_tp), (pu, 0.5)):
            c = NO_LAYER if rng.random() < p_none else chambers[rng.randrange(len(chambers))]
            L = mg.EMTF_LUT.get(c, 1)
            rows.append(row(c, (500.0 + 40.0 * L) * rng.choice((-1.0, 1.0)), 100.0 + 0.75 * s + 0.25 * (rows is pu),
                            0.05 + 0.001 * s, tp1=int(rng.random() < tp), tp2=int(rng.random() < tp / 2)))
    return mu, pu


def _plain(c, s, side=1.0, tp1=0, pu=False):
    L = mg.EMTF_LUT[c]
    return row(c, side * (500.0 + 40.0 * L), 100.0 + 0.75 * s + (0.25 if pu else 0.0), 0.05 + 0.001 * s, tp1=tp1)


def stream_cases(tag):
    out = []
    some = [c for c in ALL_CHAMBERS if mg.EMTF_LUT[c] in (3, 4, 8, 9, 10, 12)]           # 13: never "all seen"
    for n in (63, 64, 65, 127, 128, 129, 300):
        rng = random.Random(n)
        out.append(Case("rows_%d%s" % (n, tag), "stream", *_raw(rng, n, some)))
    out.append(Case("rows_300_all_chambers" + tag, "stream", *_raw(random.Random(7), 300, ALL_CHAMBERS)))
    # a chamber's first row in chunk 0, 1, 2 and rows of the same chamber (other side, other r) in the next two chunks
    c3 = CHAMBERS[10] + CHAMBERS[12] + CHAMBERS[8]
    mu, pu = [], []
    for s in range(5 * WAVE):
        k, lane = divmod(s, WAVE)
        if lane == 10 + k and k < 3:
            c, side = c3[k], 1.0                                  # first row of chamber k, in chunk k
        elif lane == 20 + k and 1 <= k < 4:
            c, side = c3[k - 1], -1.0                             # its duplicate in chunk k + 1
        elif lane == 30 + k and 2 <= k < 5:
            c, side = c3[k - 2], -1.0                             # and in chunk k + 2
        else:
            c, side = NO_LAYER, 1.0
        mu.append(_plain(c, s, side) if c != NO_LAYER else row(c, 5.0, 50.0, 0.0))
        pu.append(_plain(c3[3 + k], s, 1.0, pu=True))             # PU: one chamber per chunk, 63 duplicates of it
    out.append(Case("dup_next_chunks" + tag, "stream", mu, pu))
    # every row of chunk 1 repeats a chamber of chunk 0; chunk 2 brings new ones
    mu, pu = [], []
    for s in range(3 * WAVE):
        k, lane = divmod(s, WAVE)
        c = ALL_CHAMBERS[lane % 9] if k < 2 else ALL_CHAMBERS[9 + lane % 8]
        side = -1.0 if k == 1 else 1.0
        mu.append(_plain(c, s, side))
        pu.append(_plain(ALL_CHAMBERS[(lane + 3) % 9] if k < 2 else ALL_CHAMBERS[12 + lane % 9], s, side, pu=True))
    out.append(Case("dup_whole_chunk" + tag, "stream", mu, pu))
    # the truth filter empties chunk 0 (and rows 64 .. 69) of the muon source
    mu, pu = [], []
    for s in range(2 * WAVE + 5):
        mu.append(_plain(ALL_CHAMBERS[s % 21], s, 1.0 if s % 3 else -1.0, tp1=int(s < WAVE + 6)))
        pu.append(_plain(ALL_CHAMBERS[(s * 5) % 21], s, 1.0 if s % 2 else -1.0, pu=True))
    out.append(Case("truth_empties_chunk" + tag, "stream", mu, pu))
    # the PU entry is longer than the muon entry: its rows from the muon count on are cut, here at 64 and at 128;
    # the chambers they hold appear nowhere before
    for n_mu, n_pu in ((64, 129), (128, 300), (65, 64)):
        mu = [_plain(ALL_CHAMBERS[s % 6], s) for s in range(n_mu)]
        pu = [_plain(ALL_CHAMBERS[s % 6 + 2] if s < min(n_mu, n_pu) else ALL_CHAMBERS[10 + s % 11], s, -1.0, pu=True)
              for s in range(n_pu)]
        if n_mu > n_pu:                                           # and a muon row past the PU count
            mu[-1] = _plain(ALL_CHAMBERS[20], n_mu - 1)
        out.append(Case("cut_%d_%d%s" % (n_mu, n_pu, tag), "stream", mu, pu))
    for c in out:
        c.mu_first = bool(tag)
    return out


# ---- cut values ------------------------------------------------------------------------------------------------------
def spec_values(h1, h2):
    """(phi_slope, z0) of the pair (l1 hit, l2 hit), each (r, phi, z) float32, as the specification computes them."""
    r1, p1, z1 = (np.array([v], np.float32) for v in h1)
    r2, p2, z2 = (np.array([v], np.float32) for v in h2)
    dphi = wrap_dphi32(p2 - p1)
    with np.errstate(all="ignore"):
        dr = r2 - r1
        return (dphi / dr)[0], (z1 - r1 * (z2 - z1) / dr)[0]


def _slope_pair(target):
    """(l1 hit, l2 hit) whose phi_slope is exactly `target`: r1 = 0, so dr = r2 and z0 = z1."""
    for d in np.float32(1e-31) * (np.float32(1) + np.arange(64, dtype=np.float32) / np.float32(64)):
        p = np.float32(target * d)
        for _ in range(8):
            for q in (p, np.nextafter(p, np.float32(0)), np.nextafter(p, np.float32(9))):
                h1, h2 = (np.float32(0), np.float32(0), np.float32(1)), (d, q, np.float32(2))
                if spec_values(h1, h2)[0] == target:
                    return h1, h2
            p = np.nextafter(p, np.float32(9))
    raise AssertionError("no float32 pair gives the slope %r" % target)


def cut_pairs():
    """name -> (l1 hit, l2 hit, kept): (r, phi, z) of the layer-3 and the layer-4 hit of a two-hit graph."""
    lo, hi = np.nextafter(CUT, np.float32(0)), np.nextafter(CUT, np.float32(np.inf))
    f = np.float32
    out = {}
    for name, t, kept in (("slope_below", lo, True), ("slope_at", CUT, False), ("slope_above", hi, False)):
        out[name] = _slope_pair(t) + (kept,)
        h1, h2 = _slope_pair(t)
        out[name + "_neg"] = (h1, (h2[0], -h2[1], h2[2]), kept)
    # z0 = z1 - (r1 * (z2 - z1)) / dr with r1 = dr = 1 and z1 = 1: z2 - z1 rounds to z2, z0 = 1 - z2 rounds to -z2
    for name, t, kept in (("z0_below", lo, True), ("z0_at", CUT, False), ("z0_above", hi, False)):
        out[name] = ((f(1), f(0.5), f(1)), (f(2), f(0.5), t), kept)
        out[name + "_neg"] = ((f(1), f(0.5), f(-1)), (f(2), f(0.5), -t), kept)    # layers -3, -4: the pair (-3, -4)
    out["dr0_dphi0_nan"] = ((f(250), f(0.5), f(600)), (f(250), f(0.5), f(700)), False)
    out["dr0_dphi_inf"] = ((f(250), f(0.5), f(600)), (f(250), f(0.75), f(700)), False)
    out["r1_dz_overflows"] = ((f(1e20), f(0.5), f(1e19)), (f(2e20), f(0.5), f(3e38)), False)
    out["plain_kept"] = ((f(250), f(0.5), f(600)), (f(260), f(0.51), f(700)), True)
    return out


def cut_cases():
    out = []
    for name, (h1, h2, kept) in cut_pairs().items():
        a = row(CHAMBERS[3][0], float(h1[2]), float(h1[0]), float(h1[1]))
        b = row(CHAMBERS[4][0], float(h2[2]), float(h2[0]), float(h2[1]))
        side = 1.0 if h1[2] > 0 else -1.0
        out.append(Case("cut_" + name, "cuts", [b], [a], [3.0 * side, 4.0 * side], expect=kept))
    return out


# ---- the batch -------------------------------------------------------------------------------------------------------
def full_cases(mu_first, tag):
    out = []
    for name, signs, zero in (("full_plus", _signs_six_six(1), ()), ("full_minus", _signs_six_six(-1), ()),
                              ("full_most_segments", SIGNS_MOST_SEGMENTS, ()),
                              ("full_most_distinct", _signs_most_distinct(), (13,))):
        out.append(_ordered(name + tag, "full", *full_entry(signs, zero=zero), mu_first))
    return out


EMPTY = Case("empty", "neighbours", [], [])
ONE_HIT = Case("one_hit", "neighbours", [row(CHAMBERS[7][0], 780.0, 300.0, 0.3, tp1=1)],
               [row(CHAMBERS[5][0], 700.0, 280.0, 0.3)], [5.0])
CLOSING = Case("closing", "neighbours",
               [row(CHAMBERS[3][0], 620.0, 150.0, 0.1), row(CHAMBERS[8][0], 820.0, 250.0, 0.1)],
               [row(CHAMBERS[3][0], 620.0, 160.0, 0.1), row(CHAMBERS[8][0], 820.0, 260.0, 0.1)])


@functools.lru_cache(maxsize=None)
def batch():
    """Every case, in the order of the one batched call: the PU-first block, (empty, full, 1-hit), the muon-first
    block, the closing entry."""
    cases = []
    for i, (n, first, second) in enumerate(seeded_orders()):
        cases.append(_ordered("order_n%d_%d" % (n, i % ORDERS_PER_N), "orders", first, second, False))
    for name, first, second, lit in EXPLICIT:
        cases.append(_ordered("explicit_" + name, "explicit", first, second, False, lit))
    cases += full_cases(False, "") + layer_list_cases(False, "") + stream_cases("") + cut_cases()
    cases += [EMPTY, _ordered("full_between", "neighbours", *full_entry(_signs_six_six(1)), False), ONE_HIT]
    for i, (n, first, second) in enumerate(seeded_orders()):
        if i % ORDERS_PER_N < 5:
            cases.append(_ordered("order_n%d_%d_mu" % (n, i % ORDERS_PER_N), "orders", first, second, True))
    for name, first, second, lit in EXPLICIT:
        cases.append(_ordered("explicit_" + name + "_mu", "explicit", first, second, True, lit))
    cases += full_cases(True, "_mu") + layer_list_cases(True, "_mu") + stream_cases("_mu")
    cases.append(CLOSING)
    return tuple(cases)


def batch_columns():
    return columns([c.rows for c in batch()])


def index_of(name):
    return [c.name for c in batch()].index(name)


def graph_of(res, e):
    """(X, src, dst, y, hit_source) of entry e in a host MuonGraphs of either layout, src / dst local to the graph;
    None where the entry has no graph."""
    b = res.batch
    if res.layout == "padded":
        if not res.present[e]:
            return None
        g, nh, ns = e, int(res.n_hits[e]), int(res.n_segments[e])
    else:
        hit = np.flatnonzero(np.asarray(res.entry) - res.entry_start == e)
        if hit.size == 0:
            return None
        g = int(hit[0])
        nh, ns = int(b.hit_ptr[g + 1] - b.hit_ptr[g]), int(b.seg_ptr[g + 1] - b.seg_ptr[g])
    h0, s0 = int(b.hit_ptr[g]), int(b.seg_ptr[g])
    X = np.asarray(b.X)[h0:h0 + nh]
    return (X, np.asarray(b.src)[s0:s0 + ns] - h0, np.asarray(b.dst)[s0:s0 + ns] - h0, np.asarray(b.y)[s0:s0 + ns],
            np.asarray(res.hit_source)[h0:h0 + nh].astype(np.int64))


def check_cases(res):
    """What the cases claim, read off a host MuonGraphs of the whole batch (the specification's or the device's):
    the frame order, the pair order against the interpreter's set, l1-major segments, the cut decisions, the maxima.
    Returns the census {hits, layer_hits, distinct, candidates, rounds, rows}."""
    top = dict(hits=0, layer_hits=0, distinct=0, candidates=0, rounds=0, rows=0)
    for e, c in enumerate(batch()):
        top["rows"] = max(top["rows"], len(c.rows[0]), len(c.rows[1]))
        got = graph_of(res, e)
        if c.name in ("empty",):
            assert got is None
            continue
        assert got is not None, c.name
        X, src, dst, y, source = got
        layer = X[:, 10]
        if c.name != "closing" and c.name != "one_hit" and c.group != "cuts":
            assert bool(source[0] == 1) == c.mu_first, c.name
        vals = [float(v) for v in layer]
        n = {}
        for v in vals:
            n[v] = n.get(v, 0) + 1
        top["hits"] = max(top["hits"], len(vals))
        top["layer_hits"] = max([top["layer_hits"]] + [k for v, k in n.items() if v != 0])
        top["distinct"] = max(top["distinct"], len(n))
        if c.group == "stream":
            continue                                      # (their geometry does not keep every candidate)
        if c.layers is not None and c.group != "cuts":
            assert vals == c.layers, c.name
        if c.group == "cuts":
            assert sorted(vals) == sorted(c.layers) and len(src) == int(c.expect), c.name
            if c.expect:
                assert (vals[src[0]], vals[dst[0]]) == tuple(c.layers), c.name
            continue
        # the pair order is the interpreter's; inside a pair the segments are l1-major, both in frame order
        order = list(set(vals))
        if c.expect is not None:
            assert order == c.expect, c.name
        pairs = mg.layer_pairs(order)
        want_s, want_d = [], []
        for l1, l2 in pairs:
            a, b = [k for k, v in enumerate(vals) if v == l1], [k for k, v in enumerate(vals) if v == l2]
            want_s += [i for i in a for _ in b]
            want_d += [j for _ in a for j in b]
        assert pairs_of_segments(layer, src, dst) == pairs, c.name
        assert src.tolist() == want_s and dst.tolist() == want_d, c.name
        assert y.tolist() == [float(source[i] == 1 and source[j] == 1) for i, j in zip(want_s, want_d)], c.name
        top["candidates"] = max(top["candidates"], len(want_s))
        top["rounds"] = max(top["rounds"], -(-len(want_s) // WAVE))
    return top


def slot(res, e, first_row):
    """Slot e of a padded host MuonGraphs as bytes that do not depend on where the slot is: X, y, the sources, src /
    dst local to the slot, hit_row local to the entry ((muon, PU) first rows), the counts and flags."""
    H, S = mg.MAX_GRAPH_HITS, mg.MAX_GRAPH_SEGMENTS
    b = res.batch
    src, dst = (np.asarray(t)[e * S:(e + 1) * S].astype(np.int64) for t in (b.src, b.dst))
    source = np.asarray(res.hit_source)[e * H:(e + 1) * H].astype(np.int64)
    hrow = np.asarray(res.hit_row)[e * H:(e + 1) * H].astype(np.int64)
    hrow = np.where(source == 1, hrow - first_row[0], np.where(source == 0, hrow - first_row[1], hrow))
    parts = [np.asarray(b.X)[e * H:(e + 1) * H], np.asarray(b.y)[e * S:(e + 1) * S], source, hrow,
             np.where(src >= 0, src - e * H, src), np.where(dst >= 0, dst - e * H, dst)]
    parts += [np.asarray(getattr(res, k))[e:e + 1].astype(np.int64) for k in ("present", "written", "n_hits",
                                                                               "n_segments")]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def check_neighbours(padded, build):
    """In the padded build of the batch, the slots of the empty entry before the full entry and of the 1-hit entry
    after it hold byte for byte what a build without the full entry puts there; `build(entries)` gives that build
    (padded, host arrays).  The 1-hit entry has PU rows only: alone the reference drops it (no muon entry to mix it
    with), so it is built with the closing entry behind it, as in the batch."""
    mu, pu = batch_columns()[:2]
    first = lambda e: (int(mu["event_ptr"][e]), int(pu["event_ptr"][e]))  # noqa: E731
    e = index_of("full_between")
    assert [c.name for c in batch()[e - 1:e + 2]] == ["empty", "full_between", "one_hit"]
    assert padded.n_hits[e - 1:e + 2].tolist() == [0, 42, 1]
    assert padded.present[e - 1:e + 2].tolist() == [False, True, True]
    assert slot(padded, e - 1, first(e - 1)) == slot(build([EMPTY.rows]), 0, (0, 0))
    assert slot(padded, e, first(e)) == slot(build([batch()[e].rows]), 0, (0, 0))
    assert slot(padded, e + 1, first(e + 1)) == slot(build([ONE_HIT.rows, CLOSING.rows]), 0, (0, 0))


def census(res):
    """(hits, kept segments, hits on one signed layer, distinct values) maxima over the graphs of a flat MuonGraphs."""
    b = res.batch
    lay = np.asarray(b.X)[:, 10]
    top = [0, 0, 0, 0]
    for g in range(b.n_graphs):
        v = lay[int(b.hit_ptr[g]):int(b.hit_ptr[g + 1])]
        u, k = np.unique(v, return_counts=True)
        top = [max(top[0], v.size), max(top[1], int(b.seg_ptr[g + 1] - b.seg_ptr[g])),
               max([top[2]] + [int(c) for w, c in zip(u, k) if w != 0]), max(top[3], u.size)]
    return tuple(top)


# ---- lane 0 of k_mg_pairs, restated ----------------------------------------------------------------------------------
EMPTY_SLOT = -128


def _probe(tab, mask, v, stats):
    h = -2 if v == -1 else v
    perturb = h % (1 << 64)
    i = h & mask
    while True:
        if tab[i] == EMPTY_SLOT:
            return i, False
        if tab[i] == v:
            return i, True
        if i + 9 <= mask:
            for j in range(1, 10):
                stats["linear"] = max(stats["linear"], j)
                if tab[i + j] == EMPTY_SLOT:
                    return i + j, False
                if tab[i + j] == v:
                    return i + j, True
        stats["perturbed"][mask] = stats["perturbed"].get(mask, 0) + 1
        perturb >>= 5
        i = (i * 5 + 1 + perturb) & mask


def lane0(sv, keep, tmp_entries=32, layer_hits=8, guard="<", carry_kept=True):
    """k_mg_pairs on one graph, restated: sv the signed layers (ints) of its hits in frame order, keep(a, b) the pair
    test.  Returns (src, dst, stats) with src / dst as the kernel writes them (-1: a slot it never wrote).

    tmp_entries   entries the `tmp` copy holds when the table is rebuilt (the kernel: 32); further ones are lost
    layer_hits    kLayerHits, the slots of one layer's hit list (the kernel: 8; 6 are ever needed)
    guard         "<" as the kernel has it (lcnt < kLayerHits), or "<="
    carry_kept    False: a ballot round places its segments by the round's own prefix count alone"""
    stats = {"linear": 0, "perturbed": {}, "grown": []}
    tab, lcnt, lst = [EMPTY_SLOT] * 128, [0] * 25, [0] * (25 * layer_hits + 1)
    mask, fill = 7, 0
    for k, v in enumerate(sv):
        ok = lcnt[v + 12] <= layer_hits if guard == "<=" else lcnt[v + 12] < layer_hits
        if v != 0 and ok:
            lst[(v + 12) * layer_hits + lcnt[v + 12]] = k
            lcnt[v + 12] += 1
        slot, found = _probe(tab, mask, v, stats)
        if found:
            continue
        tab[slot] = v
        fill += 1
        if fill * 5 >= mask * 3:
            size = 8
            while size <= fill * 4:
                size <<= 1
            tmp = [w for w in tab[:mask + 1] if w != EMPTY_SLOT][:tmp_entries]
            tab[:size] = [EMPTY_SLOT] * size
            mask = size - 1
            stats["grown"].append((size, len(tmp)))
            for w in tmp:
                tab[_probe(tab, mask, w, stats)[0]] = w
    order = [v for v in tab[:mask + 1] if v != EMPTY_SLOT]
    p, m = [v for v in order if v > 0], [v for v in order if v < 0]
    pairs = [(p[i], p[i + 1]) for i in range(len(p) - 1)] + [(m[i + 1], m[i]) for i in range(len(m) - 1)]
    cand = []
    for l1, l2 in pairs:
        n2 = lcnt[l2 + 12]
        for q in range(lcnt[l1 + 12] * n2):
            cand.append((lst[(l1 + 12) * layer_hits + q // n2], lst[(l2 + 12) * layer_hits + q % n2]))
    total = sum(1 for a, b in cand if keep(a, b))
    src, dst, kept = [-1] * total, [-1] * total, 0
    for t0 in range(0, len(cand), WAVE):
        flags = [keep(a, b) for a, b in cand[t0:t0 + WAVE]]
        for lane, (a, b) in enumerate(cand[t0:t0 + WAVE]):
            if flags[lane]:
                o = (kept if carry_kept else 0) + sum(flags[:lane])
                src[o], dst[o] = a, b
        kept += sum(flags)
    stats["order"], stats["rounds"], stats["candidates"] = order, -(-len(cand) // WAVE), len(cand)
    return src, dst, stats


DEFECTS = {"tmp_of_16": dict(tmp_entries=16), "kept_not_carried": dict(carry_kept=False),
           "layer_list_of_5": dict(layer_hits=5),
           # as the issue words it; with the deduplication no layer ever gets a 7th hit, so no input can see it
           "guard_le_of_6": dict(layer_hits=6, guard="<=")}


def restated_graph(X, **defect):
    """lane0 on the hits of one graph (X [n, 11] as the specification gives it), the pair test the specification's."""
    r, phi, z = (X[:, k].astype(np.float32) for k in (3, 2, 0))
    with np.errstate(all="ignore"):
        dr = r[None, :] - r[:, None]
        slope = wrap_dphi32(phi[None, :] - phi[:, None]) / dr
        z0 = z[:, None] - r[:, None] * (z[None, :] - z[:, None]) / dr
        K = (np.abs(slope) < CUT) & (np.abs(z0) < CUT)
    assert slope.dtype == z0.dtype == np.float32
    return lane0([int(v) for v in X[:, 10]], lambda a, b: bool(K[a, b]), **defect)
