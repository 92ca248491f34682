"""CPU checks of the muon builder's bound cases (tests/muon_bound_cases.py): the generator reaches the maxima it
names, the interpreter's set and `set_order` agree on exactly these inputs, every explicit order's literal is what this
Python prints, the cut cases sit on f32(10e30) and its neighbours, and a restatement of lane 0 of k_mg_pairs with each
of three plausible defects fails the new cases while it passes the input the suite had (a `tmp` of 16: all but one
graph of it)."""
import functools

import numpy as np
import pytest

import muon_bound_cases as mb
from gnn_fpga_amd import build_muon_graphs, synth
from gnn_fpga_amd import muon_graph as mg


@functools.lru_cache(maxsize=None)
def spec(layout="flat"):
    mu, pu, vpt, veta = mb.batch_columns()
    return build_muon_graphs(mu, pu, vpt, veta, entry_start=3, layout=layout)


def test_generator_reaches_the_maxima():
    top = mb.check_cases(spec())
    assert top == mb.check_cases(spec("padded"))
    # 42 hits, 6 on one signed layer, all 25 values, 320 raw rows; 140 candidates = 3 ballot rounds (T > 128)
    assert top == dict(hits=42, layer_hits=6, distinct=25, candidates=140, rounds=3, rows=320), top
    assert len(mb.seeded_orders()) >= 1000 and len(mb.batch()) <= 1400
    for n in range(1, 26):
        assert sum(1 for m, _, _ in mb.seeded_orders() if m == n) >= 40
    names = [c.name for c in mb.batch()]
    assert len(set(names)) == len(names)
    by = {c.name: c for c in mb.batch()}
    for tag in ("", "_mu"):
        for side in ("plus", "minus"):
            lay = by["full_" + side + tag].layers
            s = 1.0 if side == "plus" else -1.0
            assert len(lay) == 42 and lay.count(10.0 * s) == 6 and lay.count(12.0 * s) == 6
        assert len(set(by["full_most_distinct" + tag].layers)) == 25
        assert mb.candidates(by["full_most_segments" + tag].layers) == 140
    # the raw row counts per source the streaming cases name
    rows = {len(c.rows[0]) for c in mb.batch() if c.group == "stream"}
    assert rows >= {63, 64, 65, 127, 128, 129, 300}


def test_most_segments_is_what_the_search_finds():
    t, signs = mb.search_most_segments()
    layer_of = [mg.EMTF_LUT[mb.ALL_CHAMBERS[k % 21]] for k in range(42)]
    assert t == 140 == mb.candidates([float(s * L) for s, L in zip(mb.SIGNS_MOST_SEGMENTS, layer_of)])
    # the bound of 441 needs two layers of 21 hits each; a layer holds at most 6, and the chain of all twelve
    # layers on one side, 2 2 4 4 2 2 2 4 4 6 4 6 hits, is the longest sum of neighbouring products
    assert sum(a * b for a, b in zip([2, 2, 4, 4, 2, 2, 2, 4, 4, 6, 4], [2, 4, 4, 2, 2, 2, 4, 4, 6, 4, 6])) == 140


def test_interpreter_and_set_order_agree_on_these_inputs():
    n = 0
    for c in mb.batch():
        if c.layers is None:
            continue
        want = list(set(c.layers))
        assert [repr(v) for v in mg.set_order(c.layers)] == [repr(v) for v in want], c.name
        assert mb.expected_order(c) == want
        n += 1
    assert n >= 1000


def test_explicit_literals_are_what_this_python_prints():
    assert len(mb.EXPLICIT) >= 16
    for name, first, second, literal in mb.EXPLICIT:
        vals = [float(v) for v in first + second]
        assert literal is not None and [repr(v) for v in list(set(vals))] == [repr(v) for v in literal], name
    lit = mb.LITERALS
    assert lit["m1_m2"] == lit["m2_m1"][::-1]                              # first come, first slot
    # the tables they reach and the probes they take, by the restatement
    keep = lambda a, b: True  # noqa: E731
    st = {name: mb.lane0([int(v) for v in first + second], keep)[2] for name, first, second, _ in mb.EXPLICIT}
    for name, s in st.items():
        assert [float(v) for v in s["order"]] == lit[name], name
    assert st["mod8_slot4"]["perturbed"].get(7, 0) >= 3 and st["mod8_slot4"]["linear"] == 0
    for name, mask in (("m1_m2_in_32", 31), ("mod32_chain", 31), ("m1_m2_in_128", 127), ("mod128_chain", 127)):
        assert st[name]["perturbed"].get(mask, 0) >= 1 and st[name]["linear"] >= 1, (name, st[name])
    # -1 and -2 start on one slot; the later one is sent to slot 22 (118), where -10 starts: what follows is the only
    # linear probing a table of these 25 values ever does, 3 slots at the most: the 9-slot limit is out of reach
    assert max(s["linear"] for s in st.values()) == 3
    for name, grown in (("grow5_last", [(32, 5)]), ("grow5_last_neg", [(32, 5)]), ("grow5_after_run", [(32, 5)]),
                        ("grow19_last", [(32, 5), (128, 19)]), ("grow19_last_zero", [(32, 5), (128, 19)]),
                        ("grow19_after_run", [(32, 5), (128, 19)]), ("grow19_after_run_dup", [(32, 5), (128, 19)])):
        assert st[name]["grown"] == grown, name
    for name in ("grow5_last", "grow5_last_neg", "grow19_last", "grow19_last_zero"):
        first, second = next((f, s) for n, f, s, _ in mb.EXPLICIT if n == name)
        vals = list(first + second)
        assert vals.index(vals[-1]) == len(vals) - 1 and len(set(vals)) in (5, 19)       # the last hit is new
    for name, k in (("grow5_after_run", 5), ("grow5_after_run_neg", 5), ("grow19_after_run", 19),
                    ("grow19_after_run_dup", 19)):
        first, second = next((f, s) for n, f, s, _ in mb.EXPLICIT if n == name)
        vals, seen, run = list(first + second), set(), 0
        for v in vals:
            if v in seen:
                run += 1
                continue
            seen.add(v)
            if len(seen) == k:
                assert run >= 4, name
                break
            run = 0


def test_cut_cases_sit_on_the_cut():
    lo, hi = np.nextafter(mb.CUT, np.float32(0)), np.nextafter(mb.CUT, np.float32(np.inf))
    assert lo < mb.CUT < hi and mb.CUT == np.float32(10e30)
    pairs = mb.cut_pairs()
    for name, t in (("below", lo), ("at", mb.CUT), ("above", hi)):
        for sign in ("", "_neg"):
            s, z0 = mb.spec_values(*pairs["slope_" + name + sign][:2])
            assert abs(s) == t and (s < 0) == bool(sign) and abs(z0) < 10
            s, z0 = mb.spec_values(*pairs["z0_" + name + sign][:2])
            assert abs(z0) == t and (z0 > 0) == bool(sign) and abs(s) < 10
    assert np.isnan(mb.spec_values(*pairs["dr0_dphi0_nan"][:2])[0])
    assert np.isposinf(mb.spec_values(*pairs["dr0_dphi_inf"][:2])[0])
    h1, h2, _ = pairs["r1_dz_overflows"]
    with np.errstate(over="ignore"):
        assert np.isinf(h1[0] * (h2[2] - h1[2])) and np.isfinite(h2[2] - h1[2])
    assert np.isneginf(mb.spec_values(h1, h2)[1])
    assert [k for k, v in pairs.items() if v[2]] == ["slope_below", "slope_below_neg", "z0_below", "z0_below_neg",
                                                    "plain_kept"]
    res = spec()
    for c in mb.batch():
        if c.group == "cuts":
            assert len(mb.graph_of(res, mb.index_of(c.name))[1]) == int(pairs[c.name[4:]][2]), c.name


def test_streaming_cases_are_what_they_claim():
    res = spec()
    by = {c.name: c for c in mb.batch()}
    for tag in ("", "_mu"):
        def hits(name):
            X, _, _, _, source = mb.graph_of(res, mb.index_of(name + tag))
            e = mb.index_of(name + tag)
            g = int(np.flatnonzero(res.entry - res.entry_start == e)[0])
            rows = res.hit_row[res.batch.hit_ptr[g]:res.batch.hit_ptr[g + 1]]
            mu, pu = mb.batch_columns()[:2]
            sub = np.where(source == 1, rows - mu["event_ptr"][e], rows - pu["event_ptr"][e])
            return X, source, sub
        # the first row of each chamber is kept, in chunk 0, 1 and 2; the copies in the chunks after are not
        X, source, sub = hits("dup_next_chunks")
        assert sub[source == 1].tolist() == [10, 64 + 11, 128 + 12] and (X[source == 1, 0] > 0).all()
        assert (sub[source == 0] // 64).tolist() == [0, 1, 2, 3, 4]       # (one PU chamber per chunk)
        # nothing of chunk 1 is kept; chunk 2 adds rows
        X, source, sub = hits("dup_whole_chunk")
        for k in (0, 1):
            chunk = sub[source == k] // 64
            assert 1 not in chunk and 0 in chunk and 2 in chunk
        # no muon row before 70 survives; the PU source keeps rows of chunk 0
        X, source, sub = hits("truth_empties_chunk")
        assert sub[source == 1].min() == 70 and sub[source == 0].min() == 0
        assert (source == 1).sum() == 21 and (source == 0).sum() == 21
        for n_mu, n_pu in ((64, 129), (128, 300), (65, 64)):
            X, source, sub = hits("cut_%d_%d" % (n_mu, n_pu))
            assert sub.max() < min(n_mu, n_pu) and (source == 0).sum() == 6 and (source == 1).sum() == 6
            c = by["cut_%d_%d%s" % (n_mu, n_pu, tag)]
            assert len(c.rows[0]) == n_mu and len(c.rows[1]) == n_pu


def test_neighbours_of_the_full_entry_on_the_host():
    mb.check_neighbours(spec("padded"), lambda entries: build_muon_graphs(*mb.columns(entries), layout="padded"))


# ---- the new cases can see the defects -------------------------------------------------------------------------------
def _failing(res, names, **defect):
    """The graphs of a flat host MuonGraphs whose segments the restatement (with a defect) gets wrong."""
    b = res.batch
    X, src, dst = (np.asarray(t) for t in (b.X, b.src, b.dst))
    bad = []
    for g in range(b.n_graphs):
        h0, h1, s0, s1 = (int(v) for v in (b.hit_ptr[g], b.hit_ptr[g + 1], b.seg_ptr[g], b.seg_ptr[g + 1]))
        try:
            s, d, _ = mb.restated_graph(X[h0:h1], **defect)
            ok = s == (src[s0:s1] - h0).tolist() and d == (dst[s0:s1] - h0).tolist()
        except (IndexError, ZeroDivisionError):
            ok = False
        if not ok:
            bad.append(names[g])
    return bad


@functools.lru_cache(maxsize=None)
def old_input():
    d = synth.emtf_events(512, seed=2)
    return build_muon_graphs(d["muon"], d["pu"], d["vp_pt"], d["vp_eta"])


def _new_names():
    res = spec()
    return [mb.batch()[int(e) - res.entry_start].name for e in res.entry]


def test_restatement_is_the_specification():
    assert _failing(spec(), _new_names()) == []
    assert _failing(old_input(), list(range(old_input().n_graphs))) == []


def test_old_input_is_far_from_the_bounds():
    hits, kept, layer_hits, distinct = mb.census(old_input())
    assert hits < 28 and kept < 64 and layer_hits < 5 and distinct <= 20


@pytest.mark.parametrize("defect", ["tmp_of_16", "kept_not_carried", "layer_list_of_5"])
def test_defects_fail_new_cases_and_pass_the_old_input(defect):
    bad = _failing(spec(), _new_names(), **mb.DEFECTS[defect])
    assert bad, defect
    old = _failing(old_input(), list(range(old_input().n_graphs)), **mb.DEFECTS[defect])
    if defect == "tmp_of_16":
        # the table is rebuilt with exactly 19 entries and never with more, so 19 is the only size `tmp` is tested at.
        # One graph in 512 of the old input has 19 values and sees this defect, by the accident of its seed; here every
        # order of 19 and more does, at every position the 19th can take
        assert old == [365] and mb.census(old_input())[3] == 19
        assert len(bad) >= 7 * 40
        assert any(n.startswith("explicit_grow19") for n in bad) and any(n.startswith("order_n25") for n in bad)
        for k in range(19, 26):
            assert sum(n.startswith("order_n%d_" % k) and not n.endswith("_mu") for n in bad) == 40
        assert not any(n.startswith("order_n%d_" % k) for n in bad for k in range(1, 19))
        return
    assert old == []
    if defect == "kept_not_carried":
        # every graph of more than 64 kept segments, and no other
        res = spec()
        assert sorted(bad) == sorted(n for n, k in zip(_new_names(), res.n_segments) if k > 64)
        assert "full_most_segments" in bad and "full_most_segments_mu" in bad
    else:
        assert "list_6_1_p" in bad and "list_5_6_m_mu" in bad and "full_plus" in bad
        assert not any(n.startswith("list_5_1") or n.startswith("list_5_5") for n in bad)


def test_a_guard_of_le_cannot_be_seen():
    """`lcnt <= kLayerHits` in place of `<`, with lists of 6: the deduplication leaves a signed layer 6 hits at the
    most (3 chambers x 2 sources), so the guard never decides and no input tells the two apart.  (The kernel's lists
    have 8 slots.)  What a too-short list does is shown by `layer_list_of_5` above."""
    assert max(mb.CAPACITY.values()) == 6
    assert _failing(spec(), _new_names(), **mb.DEFECTS["guard_le_of_6"]) == []
