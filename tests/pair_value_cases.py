"""The graph builder's pair arithmetic, pinned on its values: what tests/test_pair_values_host.py (the numpy
specification) and tests/test_gpu_pair_values.py (csrc/graph_build.hip) share.

`restate` is an independent restatement of the reference's steps for one small input: the sector split and the float32
re-centring of gnn/prepareGraphs.py:88-103, the wrap of gnn/graph.py:37-42 and slope and z0 of gnn/graph.py:57-62, one
hit pair at a time with np.float32 scalars, in the reference's order of operations.  It calls neither
`graph_build.pair_values` nor `wrap_dphi32`.  From its table of (phi_slope, z0, same particle) come

* `expected_counts`: the cut study's count array for any edges (the bin of v is the number of edges <= v, NaN last);
* `expected_segments` / `expected_kept`: the builder's src, dst, y, seg_ptr and per-pair counts for any cuts.

The checks put the cuts ON the values.  `check_value_probe` walks all distinct |phi_slope| and |z0| in chunks of 31
values v and passes the sorted union of v and nextafter(v, +inf) as edges: the one-ulp bin [v, next(v)) holds exactly
the pairs whose value is v, so the calls together say that the multiset of float32 values per (layer pair, class) is
the restatement's, to the bit.  `check_cuts_on_values` builds graphs with the cut at a value v and at next(v), as exact
float32 values and as Python floats a quarter of an ulp inside (thresholds round to float32, to nearest, before the
comparison): the two builds differ by exactly the pairs whose value is v.  The values are chosen where multiplying by
float32(1) / dr differs from dividing by dr (`alt_reciprocal`), some of the slopes where carrying dphi unrounded into
the divide differs too (`alt_unrounded_dphi`), so neither shortcut can pass.  Every check raises AssertionError.

`hand_made` is a table of single pairs at the arithmetic's corners and `tile_event` an event whose layers sit on the
row (128) and tile (512) sizes of k_gb_pairs and k_cs_pairs.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

from gnn_fpga_amd import study_segment_cuts, synth
from gnn_fpga_amd.graph_build import build_graphs

F = np.float32
INF = float("inf")
PI32 = F(np.pi)                       # numpy compares and subtracts np.pi and 2 np.pi as float32 against float32 data
TWO_PI32 = F(2 * np.pi)
INNER_LAYERS = 5                      # gnn/graph.py:65: pairs whose first layer is below this take phi_slope_max
ADJACENT = np.stack([np.arange(9), np.arange(1, 10)], axis=1).astype(np.int32)
CHUNK = 31                            # values per axis and call: 62 edges, 63 x 63 = 3969 of the 4096 cells
N_CUT_VALUES = 16                     # per axis, for the cuts through the builder
TINY = F(1e-45)                       # the smallest subnormal

Event = namedtuple("Event", ["cols", "pairs", "n_phi_sectors"])
PairTable = namedtuple("PairTable", ["graph", "pair", "src", "dst", "slope", "z0", "same"])
Restated = namedtuple("Restated", ["hit_ptr", "hit_index", "r", "cphi", "z", "table"])


def up(v):
    """The next float32 above v."""
    return np.nextafter(np.asarray(v, F), F(np.inf))


# ---- the independent restatement ---------------------------------------------------------------------------------------
def restate(ev):
    """Every hit pair of every listed layer pair of every (event, sector) graph, in the builder's order (graphs
    event-major and sector-minor, layer pairs as listed, l1 hits in frame order, for each of them the l2 hits in frame
    order), computed one pair at a time in float32 scalars."""
    cols, pairs, S = ev
    width = 2 * np.pi / S                                              # gnn/prepareGraphs.py:88-89
    edges = np.linspace(-np.pi, np.pi, S + 1)
    hit_ptr, index, rr, cc, zz = [0], [], [], [], []
    rows_out = {k: [] for k in PairTable._fields}
    ep = cols.event_ptr
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        for e in range(len(ep) - 1):
            for s in range(S):
                lo, hi = edges[s], edges[s + 1]
                hits = [i for i in range(int(ep[e]), int(ep[e + 1])) if lo < float(cols.phi[i]) < hi]      # :100
                cphi = [(F(cols.phi[i]) - F(lo)) - F(width / 2) for i in hits]                            # :102
                base, g = hit_ptr[-1], len(hit_ptr) - 1
                for p, (l1, l2) in enumerate(np.asarray(pairs).tolist()):
                    first = [k for k, i in enumerate(hits) if cols.layer[i] == l1]
                    second = [k for k, i in enumerate(hits) if cols.layer[i] == l2]
                    for a in first:
                        r1, p1, z1 = F(cols.r[hits[a]]), cphi[a], F(cols.z[hits[a]])
                        for b in second:
                            r2, p2, z2 = F(cols.r[hits[b]]), cphi[b], F(cols.z[hits[b]])
                            dphi = p2 - p1                                                                # graph.py:39-41
                            if dphi > PI32:
                                dphi = dphi - TWO_PI32
                            if dphi < -PI32:
                                dphi = dphi + TWO_PI32
                            dz = z2 - z1                                                                  # :59-62
                            dr = r2 - r1
                            slope = dphi / dr
                            z0 = z1 - r1 * dz / dr
                            assert type(slope) is F and type(z0) is F
                            for k, v in zip(PairTable._fields, (g, p, base + a, base + b, slope, z0,
                                                                cols.particle_id[hits[a]] == cols.particle_id[hits[b]])):
                                rows_out[k].append(v)
                index += hits
                rr += [cols.r[i] for i in hits]
                cc += cphi
                zz += [cols.z[i] for i in hits]
                hit_ptr.append(base + len(hits))
    kinds = dict(graph=np.int64, pair=np.int64, src=np.int64, dst=np.int64, slope=F, z0=F, same=bool)
    table = PairTable(*(np.asarray(rows_out[k], kinds[k]) for k in PairTable._fields))
    return Restated(np.asarray(hit_ptr, np.int64), np.asarray(index, np.int64), np.asarray(rr, F), np.asarray(cc, F),
                    np.asarray(zz, F), table)


def bins_of(edges, v):
    """The number of edges <= v; NaN counts as above every edge."""
    v = np.asarray(v, F)
    with np.errstate(invalid="ignore"):
        b = (np.asarray(edges, F)[None, :] <= v[:, None]).sum(axis=1)
    return np.where(np.isnan(v), len(edges), b)


def expected_counts(table, n_pairs, se, ze):
    """The cut study's counts int64 [P, 2, NS + 1, NZ + 1] for the restated pairs."""
    NS, NZ = len(se), len(ze)
    counts = np.zeros((n_pairs, 2, NS + 1, NZ + 1), np.int64)
    np.add.at(counts, (table.pair, table.same.astype(np.int64), bins_of(se, np.abs(table.slope)),
                       bins_of(ze, np.abs(table.z0))), 1)
    return counts


def kept_mask(table, pairs, cuts):
    """gnn/graph.py:65 on the restated values; cuts = (phi_slope_max, phi_slope_outer_max, z0_max), Python floats that
    round to float32 before the comparison."""
    with np.errstate(over="ignore"):
        psm, pso, z0m = (F(c) for c in cuts)
    cut = np.where(np.asarray(pairs)[table.pair, 0] < INNER_LAYERS, psm, pso).astype(F)
    with np.errstate(invalid="ignore"):
        return (np.abs(table.slope) < cut) & (np.abs(table.z0) < z0m)


def expected_segments(rs, pairs, cuts):
    """(src int32, dst int32, y float32, seg_ptr int64) of the builder for the restated pairs."""
    t = rs.table
    keep = kept_mask(t, pairs, cuts)
    n_graphs = len(rs.hit_ptr) - 1
    seg_ptr = np.concatenate([[0], np.cumsum(np.bincount(t.graph[keep], minlength=n_graphs))]).astype(np.int64)
    return t.src[keep].astype(np.int32), t.dst[keep].astype(np.int32), t.same[keep].astype(F), seg_ptr


def expected_kept(table, pairs, cuts):
    """SegmentCutStudy.kept for the restated pairs: int64 [P, 2] (fake, true)."""
    keep = kept_mask(table, pairs, cuts)
    out = np.zeros((len(pairs), 2), np.int64)
    np.add.at(out, (table.pair[keep], table.same[keep].astype(np.int64)), 1)
    return out


# ---- the two altered forms (numpy, on the restated hits): what a kernel must not compute ------------------------------
def _hit_columns(rs):
    t = rs.table
    return rs.r[t.src], rs.cphi[t.src], rs.z[t.src], rs.r[t.dst], rs.cphi[t.dst], rs.z[t.dst]


def _wrap(d, pi, two_pi):
    d = np.where(d > pi, d - two_pi, d)
    return np.where(d < -pi, d + two_pi, d)


def form_division(r1, p1, z1, r2, p2, z2):
    """The reference's form, vectorised: equal to the scalar restatement bit for bit."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        dphi, dz, dr = _wrap(p2 - p1, PI32, TWO_PI32), z2 - z1, r2 - r1
        return dphi / dr, z1 - r1 * dz / dr


def form_reciprocal(r1, p1, z1, r2, p2, z2):
    """Multiplies by float32(1) / dr where the reference divides by dr."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        dphi, dz, dr = _wrap(p2 - p1, PI32, TWO_PI32), z2 - z1, r2 - r1
        inv = F(1) / dr
        return dphi * inv, z1 - (r1 * dz) * inv


def form_unrounded_dphi(r1, p1, z1, r2, p2, z2):
    """Does not round dphi to float32 before the divide (z0 is the reference's)."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        dphi = _wrap(p2.astype(np.float64) - p1.astype(np.float64), float(PI32), float(TWO_PI32))
        dz, dr = z2 - z1, r2 - r1
        return (dphi / dr.astype(np.float64)).astype(F), z1 - r1 * dz / dr


def alt_reciprocal(rr, pp, zz, i, j):
    """`form_reciprocal` with graph_build.pair_values' signature, for monkeypatching the specification."""
    return form_reciprocal(rr[i], pp[i], zz[i], rr[j], pp[j], zz[j])


def alt_unrounded_dphi(rr, pp, zz, i, j):
    return form_unrounded_dphi(rr[i], pp[i], zz[i], rr[j], pp[j], zz[j])


# ---- the inputs ----------------------------------------------------------------------------------------------------------
def _concat_events(*events):
    ptr = np.concatenate([[0], np.cumsum([e.r.shape[0] for e in events])]).astype(np.int64)
    return synth.HitColumns(*(np.concatenate([e[k] for e in events]) for k in range(5)), ptr)


def _front_event():
    """Three hits: with two sectors, one in the first and two in the second."""
    return synth.HitColumns(np.array([32.1, 71.9, 116.2], F), np.array([0.5, 0.5004, -2.0], F),
                            np.array([10.0, 22.0, -5.0], F), np.array([0, 1, 2], np.int32),
                            np.array([7, 7, 8], np.int64), np.array([0, 3], np.int64))


PROBE_VARIANTS = ("one", "front")


@functools.lru_cache(maxsize=None)
def probe_event(variant):
    """"one": synth.barrel_event(12, 4, seed=3) as one sector; "front": the same event behind a 3-hit event, two
    sectors, so that bucket offsets are neither zero nor multiples of four.  Both with the nine adjacent layer pairs."""
    ev = synth.barrel_event(12, 4, n_events=1, seed=3)
    if variant == "one":
        return Event(ev, ADJACENT, 1)
    assert variant == "front"
    return Event(_concat_events(_front_event(), ev), ADJACENT, 2)


@functools.lru_cache(maxsize=None)
def probe_restated(variant):
    return restate(probe_event(variant))


def probe_chunks(table):
    """[(phi_slope edges, z0 edges)]: all distinct finite |phi_slope| and |z0| in chunks of CHUNK values v, each chunk
    as the sorted union of v and next(v); the shorter axis repeats its last chunk."""
    axes = []
    for vals in (table.slope, table.z0):
        u = np.unique(np.abs(vals[np.isfinite(vals)]))
        axes.append([np.unique(np.concatenate([u[k:k + CHUNK], up(u[k:k + CHUNK])])) for k in range(0, len(u), CHUNK)])
    n = max(len(a) for a in axes)
    return [(axes[0][min(k, len(axes[0]) - 1)], axes[1][min(k, len(axes[1]) - 1)]) for k in range(n)]


CutValue = namedtuple("CutValue", ["v", "outer"])       # a float32 value of the data; does it belong to an outer pair?


@functools.lru_cache(maxsize=None)
def cut_values(variant):
    """(16 |phi_slope| values, 16 |z0| values) of the probe event, each a CutValue.  All lie where `form_reciprocal`
    differs from the division; half of the slope values come from pairs whose first layer is >= 5 (they are cut by
    phi_slope_outer_max); on each side up to four slope values lie where `form_unrounded_dphi` differs too (that form
    changes few values: a difference of two nearby float32 numbers is mostly exact).  Spread evenly by rank."""
    rs = probe_restated(variant)
    t = rs.table
    hc = _hit_columns(rs)
    div, rec, unr = form_division(*hc), form_reciprocal(*hc), form_unrounded_dphi(*hc)
    assert div[0].tobytes() == t.slope.tobytes() and div[1].tobytes() == t.z0.tobytes()
    outer = np.asarray(probe_event(variant).pairs)[t.pair, 0] >= INNER_LAYERS

    def spread(mask, vals, n, without=()):
        u = np.setdiff1d(np.abs(vals[mask]), np.asarray(without, F))
        n = min(n, len(u))
        return u[np.linspace(0, len(u) - 1, n).round().astype(int)].tolist() if n else []

    slopes = []
    for is_outer in (False, True):
        side = outer == is_outer
        both = spread(side & (rec[0] != div[0]) & (unr[0] != div[0]), t.slope, N_CUT_VALUES // 4)
        only = spread(side & (rec[0] != div[0]), t.slope, N_CUT_VALUES // 2 - len(both), without=both)
        slopes += [CutValue(F(v), is_outer) for v in both + only]
    z0s = [CutValue(F(v), False) for v in spread(rec[1] != div[1], t.z0, N_CUT_VALUES)]
    assert len(slopes) == len(z0s) == N_CUT_VALUES
    return slopes, z0s


@functools.lru_cache(maxsize=None)
def fixture_cuts():
    """(phi_slope_max, phi_slope_outer_max, z0_max) of the reference-made fixture `pair_values` (the probe event, one
    sector): values of the data nearest the default cuts 0.001 and 200, each where `form_reciprocal` gives a smaller
    value (which that form would keep), each of a pair that passes the other cut, so that the pair is kept one ulp
    further up and not at the value itself."""
    rs = probe_restated("one")
    t = rs.table
    hc = _hit_columns(rs)
    div, rec = form_division(*hc), form_reciprocal(*hc)
    outer = ADJACENT[t.pair, 0] >= INNER_LAYERS
    a, b = np.abs(t.slope), np.abs(t.z0)

    def nearest(mask, vals, target):
        assert mask.any()
        return F(vals[mask][np.argmin(np.abs(vals[mask] - F(target)))])

    ar, br = np.abs(rec[0]), np.abs(rec[1])
    psm = nearest((ar < a) & ~outer & (b < F(100.0)), a, 0.001)
    pso = nearest((ar < a) & outer & (b < F(100.0)), a, 0.001)
    z0m = nearest((br < b) & (a < np.where(outer, pso, psm)) & (b > F(100.0)), b, 200.0)
    return float(psm), float(pso), float(z0m)


def fixture_edges():
    """(phi_slope edges, z0 edges) of the cut-study fixture `pair_values`: the fixture's cuts and the 16 cut values of
    each axis, each with its upper neighbour."""
    psm, pso, z0m = fixture_cuts()
    slopes, z0s = cut_values("one")
    s = np.array([cv.v for cv in slopes] + [psm, pso], F)
    z = np.array([cv.v for cv in z0s] + [z0m], F)
    return np.unique(np.concatenate([s, up(s)])), np.unique(np.concatenate([z, up(z)]))


def quarter_inside(v):
    """(a Python float a quarter of an ulp above v, one a quarter of an ulp below next(v)): they round to v and to
    next(v)."""
    lo, hi = float(v), float(up(v))
    a, b = lo + 0.25 * (hi - lo), hi - 0.25 * (hi - lo)
    assert lo < a < b < hi and F(a) == F(v) and F(b) == up(v)
    return a, b


# ---- running the code under test: numpy columns take the specification, CUDA tensors the HIP kernels ---------------------
def columns(cols, device=None):
    """The five hit columns as build_graphs and study_segment_cuts take them: numpy, or tensors on `device`."""
    if device is None:
        return tuple(cols[:5])
    return tuple(torch.from_numpy(np.ascontiguousarray(c)).to(device) for c in cols[:5])


def to_numpy(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def run_study(c, ev, se, ze):
    return study_segment_cuts(c[0], c[1], c[2], c[3], ev.pairs, c[4], event_ptr=ev.cols.event_ptr,
                              n_phi_sectors=ev.n_phi_sectors, phi_slope_edges=se, z0_edges=ze)


def run_build(c, ev, cuts):
    return build_graphs(c[0], c[1], c[2], c[3], ev.pairs, particle_id=c[4], event_ptr=ev.cols.event_ptr,
                        n_phi_sectors=ev.n_phi_sectors, phi_slope_max=cuts[0], phi_slope_outer_max=cuts[1],
                        z0_max=cuts[2])


def assert_study_is_restated(c, ev, rs, se, ze):
    s = run_study(c, ev, se, ze)
    np.testing.assert_array_equal(to_numpy(s.counts), expected_counts(rs.table, len(ev.pairs), se, ze))
    return s


def assert_build_is_restated(c, ev, rs, cuts):
    b = run_build(c, ev, cuts)
    src, dst, y, seg_ptr = expected_segments(rs, ev.pairs, cuts)
    np.testing.assert_array_equal(np.asarray(b.seg_ptr), seg_ptr)
    np.testing.assert_array_equal(np.asarray(b.hit_ptr), rs.hit_ptr)
    np.testing.assert_array_equal(to_numpy(b.src), src)
    np.testing.assert_array_equal(to_numpy(b.dst), dst)
    assert to_numpy(b.y).tobytes() == y.tobytes()
    np.testing.assert_array_equal(to_numpy(b.hit_index), rs.hit_index)
    return b


# ---- the checks ------------------------------------------------------------------------------------------------------------
def check_value_probe(c, variant):
    """Every value through the cut study: the whole count array of every call equals the restatement's."""
    ev, rs = probe_event(variant), probe_restated(variant)
    chunks = probe_chunks(rs.table)
    for se, ze in chunks:
        assert_study_is_restated(c, ev, rs, se, ze)
    return len(chunks)


def _segment_keys(b, n_hits):
    return set((to_numpy(b.src).astype(np.int64) * n_hits + to_numpy(b.dst)).tolist())


def check_cuts_on_values(c, variant, axis):
    """Cuts on 16 values of one axis ("slope" or "z0") through the builder, and SegmentCutStudy.kept at those edges."""
    ev, rs = probe_event(variant), probe_restated(variant)
    t = rs.table
    values = cut_values(variant)[0 if axis == "slope" else 1]
    vs = np.array([cv.v for cv in values], F)
    on = np.unique(np.concatenate([vs, up(vs)]))
    if axis == "slope":
        se, ze = np.unique(np.concatenate([on, [F(0.001), F(np.inf)]])), np.array([np.inf], F)
    else:
        se, ze = np.array([np.inf], F), np.unique(np.concatenate([on, [F(np.inf)]]))
    study = assert_study_is_restated(c, ev, rs, se, ze)
    n_hits = int(rs.hit_ptr[-1])
    outer_pair = np.asarray(ev.pairs)[t.pair, 0] >= INNER_LAYERS
    for cv in values:
        v, nxt = float(cv.v), float(up(cv.v))
        if axis == "slope":                          # the other slope cut stays at the default
            cuts_of = (lambda x: (0.001, x, INF)) if cv.outer else (lambda x: (x, 0.001, INF))
            on_v = (np.abs(t.slope) == cv.v) & (outer_pair == cv.outer)
        else:
            cuts_of = lambda x: (INF, INF, x)        # noqa: E731
            on_v = np.abs(t.z0) == cv.v
        assert on_v.any()
        want = set((t.src[on_v] * n_hits + t.dst[on_v]).tolist())
        qa, qb = quarter_inside(cv.v)
        below = assert_build_is_restated(c, ev, rs, cuts_of(v))
        above = assert_build_is_restated(c, ev, rs, cuts_of(nxt))
        k_below, k_above = _segment_keys(below, n_hits), _segment_keys(above, n_hits)
        assert k_below <= k_above and k_above - k_below == want, (axis, cv)
        for q, exact in ((qa, below), (qb, above)):
            b = assert_build_is_restated(c, ev, rs, cuts_of(q))
            assert torch.equal(b.src, exact.src) and torch.equal(b.dst, exact.dst) and torch.equal(b.y, exact.y)
        for x, b in ((v, below), (nxt, above), (qa, below), (qb, above)):
            psm, pso, z0m = cuts_of(x)
            kept = to_numpy(study.kept(psm, z0m, pso))
            np.testing.assert_array_equal(kept, expected_kept(t, ev.pairs, cuts_of(x)))
            assert int(kept.sum()) == b.n_segments and int(kept[:, 1].sum()) == int(to_numpy(b.y).sum())


# ---- hand-made pairs: the corners of the arithmetic ------------------------------------------------------------------------
U = 2.0 ** -22                        # the float32 spacing in [2, 4): f32(pi) is 13176795 U
PHI_A, PHI_B = -1187766 * U, 11989029 * U     # PHI_B + f32(pi) is 6.0 exactly, and PHI_B - PHI_A is f32(pi) exactly
BIG_R = 1e32                          # a centred phi is a multiple of 2^-23, so a subnormal slope needs dr > 1e31

# name: (r1, phi1, z1, r2, phi2, z2): one pair per row, the first hit on the pair's first layer
HAND_MADE = (
    ("dphi_pi", (32.0, PHI_A, 1.0, 72.0, PHI_B, 2.0)),                    # dphi = f32(pi): not wrapped
    ("dphi_pi_above", (32.0, PHI_A - U, 1.0, 72.0, PHI_B, 2.0)),          # one ulp above: wrapped to about -pi
    ("dphi_pi_below", (32.0, PHI_A + U, 1.0, 72.0, PHI_B, 2.0)),
    ("dphi_minus_pi", (32.0, PHI_B, 1.0, 72.0, PHI_A, 2.0)),              # dphi = -f32(pi): not wrapped
    ("dphi_minus_pi_below", (32.0, PHI_B, 1.0, 72.0, PHI_A - U, 2.0)),    # one ulp below: wrapped to about +pi
    ("dphi_minus_pi_above", (32.0, PHI_B, 1.0, 72.0, PHI_A + U, 2.0)),
    ("dr0_plus_inf", (100.0, 0.0, 5.0, 100.0, 0.25, 5.0)),                # dphi > 0 over dr = 0; z0 = 5 - 0 / 0: NaN
    ("dr0_minus_inf", (100.0, 0.25, 5.0, 100.0, 0.0, 7.0)),               # slope -inf, z0 = 5 - 200 / 0: -inf
    ("dr0_nan", (100.0, 0.25, 5.0, 100.0, 0.25, 7.0)),                    # 0 / 0
    ("slope_plus_zero", (32.0, 0.25, 3.0, 72.0, 0.25, 6.0)),
    ("slope_minus_zero", (72.0, 0.25, 3.0, 32.0, 0.25, 6.0)),             # dphi = 0 over dr < 0
    ("slope_subnormal", (0.0, 0.0, 4.0, BIG_R, 3 * U, 8.0)),              # 3 * 2^-22 / 1e32: gradual underflow
    ("z0_minus_zero", (32.0, 0.0, -0.0, 72.0, 0.001, -0.0)),
    ("slope_large_finite", (0.0, 0.0, 1.0, 1e-30, 1.0, 1.0)),             # about 1e30: below a last edge of +inf
)
HAND_MADE_NAMES = tuple(n for n, _ in HAND_MADE)


@functools.lru_cache(maxsize=None)
def hand_made():
    """The table as one input: row k is event k, two hits on layers 2k and 2k + 1, its pair (2k, 2k + 1); one sector.
    The study's row k and the builder's graph k then belong to table row k alone."""
    v = np.array([row for _, row in HAND_MADE], np.float64)
    n = len(HAND_MADE)
    r, phi, z = (np.stack([v[:, k], v[:, k + 3]], axis=1).ravel().astype(F) for k in range(3))
    layer = np.arange(2 * n, dtype=np.int32)
    pid = np.repeat(np.arange(1, n + 1), 2).astype(np.int64)
    pid[1::4] += 100                                              # every second row is a fake pair
    cols = synth.HitColumns(r, phi, z, layer, pid, np.arange(0, 2 * n + 1, 2, dtype=np.int64))
    return Event(cols, layer.reshape(n, 2), 1)


@functools.lru_cache(maxsize=None)
def hand_made_restated():
    return restate(hand_made())


def hand_made_edges():
    """Both axes: 0, the smallest subnormal, every finite value of the table with its upper neighbour, 200 and +inf."""
    t = hand_made_restated().table
    axes = []
    for vals, extra in ((t.slope, 1e-3), (t.z0, 200.0)):
        u = np.abs(vals[np.isfinite(vals)])
        axes.append(np.unique(np.concatenate([[F(0), TINY, F(extra), F(np.inf)], u, up(u)]).astype(F)))
    return axes


def hand_made_cuts():
    """(phi_slope_max = phi_slope_outer_max, z0_max) settings for the builder: on zero's neighbour, on the subnormal
    quotient and its neighbour, infinite, and the defaults."""
    t = hand_made_restated().table
    q = float(np.abs(t.slope[HAND_MADE_NAMES.index("slope_subnormal")]))
    big = float(np.abs(t.slope[HAND_MADE_NAMES.index("slope_large_finite")]))
    return [(float(TINY), INF), (q, INF), (float(up(q)), INF), (INF, INF), (INF, float(TINY)), (big, INF),
            (float(up(big)), INF), (0.001, 200.0)]


def check_hand_made(c):
    ev, rs = hand_made(), hand_made_restated()
    se, ze = hand_made_edges()
    study = assert_study_is_restated(c, ev, rs, se, ze)
    for s_cut, z_cut in hand_made_cuts():
        cuts = (s_cut, s_cut, z_cut)
        b = assert_build_is_restated(c, ev, rs, cuts)
        want = kept_mask(rs.table, ev.pairs, cuts)                  # one pair per graph: the row's kept flag
        np.testing.assert_array_equal(np.diff(np.asarray(b.seg_ptr)), want.astype(np.int64))
        np.testing.assert_array_equal(to_numpy(study.kept(s_cut, z_cut)).sum(axis=1), want.astype(np.int64))


# ---- row and tile edges of k_gb_pairs<0>, k_gb_pairs<1>, k_cs_pairs --------------------------------------------------------
TILE_COUNTS = (129, 513, 128, 512, 127, 511, 257, 1025, 1, 1)      # hits on layers 0 .. 9: 128 rows a task, 512 a tile
TILE_CUTS = (0.001, 0.001, 200.0)                                  # the defaults of gnn/prepareGraphs.py:37-42
TILE_SLOPE_EDGES = np.geomspace(1e-5, 1e-2, 8)
TILE_Z0_EDGES = np.geomspace(10.0, 3000.0, 8)
TILE_VARIANTS = ("alone", "second")


@functools.lru_cache(maxsize=None)
def tile_event(variant):
    """One event, one sector, TILE_COUNTS hits per layer: radii with 0.1 mm jitter, phi in a window of half a radian,
    z = r cot(theta) + 0.5 mm jitter with cot(theta) in [-0.5, 0.5], particle ids from 1 .. 39; rows shuffled.  The two
    single hits of layers 8 and 9 lie on one central line, so that layer 7 finds partners in layer 8.
    "second": the same event behind the 3-hit event, so that no bucket starts at 0."""
    rng = np.random.default_rng(20261)
    r, phi, z, layer = [], [], [], []
    for l, n in enumerate(TILE_COUNTS):
        rl = synth.BARREL_RADII[l] + rng.normal(0.0, 0.1, n)
        cot = rng.uniform(-0.5, 0.5, n)
        pl = rng.uniform(-0.25, 0.25, n)
        if n == 1:
            cot[:], pl[:] = 0.02, 0.01 + 1e-4 * rl
        r.append(rl)
        phi.append(pl)
        z.append(rl * cot + rng.normal(0.0, 0.5, n))
        layer.append(np.full(n, l))
    r, phi, z, layer = (np.concatenate(v) for v in (r, phi, z, layer))
    pid = rng.integers(1, 40, r.shape[0])
    order = rng.permutation(r.shape[0])
    ev = synth.HitColumns(r[order].astype(F), phi[order].astype(F), z[order].astype(F), layer[order].astype(np.int32),
                          pid[order].astype(np.int64), np.array([0, r.shape[0]], np.int64))
    if variant == "alone":
        return Event(ev, ADJACENT, 1)
    assert variant == "second"
    return Event(_concat_events(_front_event(), ev), ADJACENT, 1)


@functools.lru_cache(maxsize=None)
def tile_spec(variant):
    """The numpy specification on the tile event, computed once: (batch, study)."""
    ev = tile_event(variant)
    c = columns(ev.cols)
    return run_build(c, ev, TILE_CUTS), run_study(c, ev, TILE_SLOPE_EDGES, TILE_Z0_EDGES)


def check_tile_edges(c, variant):
    """The code under test against the specification, array for array."""
    ev = tile_event(variant)
    host, host_study = tile_spec(variant)
    b = run_build(c, ev, TILE_CUTS)
    np.testing.assert_array_equal(np.asarray(b.hit_ptr), np.asarray(host.hit_ptr))
    np.testing.assert_array_equal(np.asarray(b.seg_ptr), np.asarray(host.seg_ptr))
    assert to_numpy(b.X).tobytes() == host.X.numpy().tobytes()
    for k in ("src", "dst", "hit_index"):
        np.testing.assert_array_equal(to_numpy(getattr(b, k)), getattr(host, k).numpy(), err_msg=k)
    assert to_numpy(b.y).tobytes() == host.y.numpy().tobytes()
    s = run_study(c, ev, TILE_SLOPE_EDGES, TILE_Z0_EDGES)
    np.testing.assert_array_equal(to_numpy(s.counts), host_study.counts.numpy())
