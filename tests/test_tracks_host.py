"""The track builder's specification (gnn-fpga_amd/tracks.py) against independent restatements - a plain-Python
union-find, scipy's connected_components, a Counter for the matching -, the hand-made cases, the barrel recipe's fixed
numbers, argument errors, and the C ABI's new entry points; no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gnn_fpga_amd
from gnn_fpga_amd import HitGraphBatch, TrackMatch, Tracks, _lib, build_tracks, synth
from gnn_fpga_amd.tracks import build_tracks_numpy, match_tracks_numpy
from tracks_cases import (BARREL, HAND, assert_match_equal, assert_tracks_equal, barrel_batch, hand_batch, kept_restated,
                          match_restated, match_spec, roots_union_find, spec_of, tracks_from_roots)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gnn_track_build_workspace_bytes", "gnn_track_build_labels", "gnn_track_build_lists",
         "gnn_track_match_workspace_bytes", "gnn_track_match")
LIST_KEYS = ("track_of_hit", "n_tracks", "track_ptr", "track_hits", "track_graph", "graph_track_ptr")


def layered(seed):
    g = synth.layered_graph(1000, 1500, seed=seed)
    scores = np.random.default_rng(100 + seed).random(1500).astype(np.float32)
    return g, scores


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("mode", ["components", "best"])
def test_specification_equals_the_union_find_restatement(seed, mode):
    g, scores = layered(seed)
    for thr in (0.2, 0.5, 0.8):
        kept = kept_restated(g.src, g.dst, scores, 1000, thr, mode)
        root = roots_union_find(1000, g.src[kept], g.dst[kept])
        for min_hits in (1, 3):
            spec = build_tracks_numpy(g.src, g.dst, scores, 1000, [0, 1000], thr, mode, min_hits)
            assert np.array_equal(np.flatnonzero(spec["kept"]), kept) and spec["n_kept"] == len(kept)
            assert np.array_equal(spec["root"], root) and spec["status"] == 0
            want = tracks_from_roots(root, [0, 1000], min_hits)
            for k in LIST_KEYS:
                assert np.array_equal(spec[k], want[k]), (thr, min_hits, k)
            if min_hits == 1:
                assert spec["n_tracks"] == np.unique(root).size and spec["track_hits"].size == 1000
        assert 0 < len(kept) < 1500


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_specification_equals_scipy(seed):
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    sparse = pytest.importorskip("scipy.sparse")
    g, scores = layered(seed)
    for mode in ("components", "best"):
        for thr in (0.2, 0.5, 0.8):
            spec = build_tracks_numpy(g.src, g.dst, scores, 1000, [0, 1000], thr, mode, 1)
            a, b = g.src[spec["kept"]], g.dst[spec["kept"]]
            adj = sparse.coo_matrix((np.ones(a.size), (a, b)), shape=(1000, 1000))
            n, label = csgraph.connected_components(adj, directed=False)
            first = np.full(n, 1000)
            np.minimum.at(first, label, np.arange(1000))               # a component's smallest hit
            assert np.array_equal(spec["root"], first[label]) and spec["n_tracks"] == n
            # min_hits = 1: the tracks are scipy's components, numbered by their smallest hit
            assert np.array_equal(spec["track_of_hit"], np.argsort(np.argsort(first))[label])


def run_hand(name, mode):
    batch, e, thr, mh = hand_batch(name)
    return build_tracks(batch, e, thr, mode, mh), spec_of(batch, e, thr, mode, mh)


@pytest.mark.parametrize("mode", ["components", "best"])
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_made_cases_equal_the_restatement(name, mode):
    batch, e, thr, mh = hand_batch(name)
    tracks, spec = run_hand(name, mode)
    assert isinstance(tracks, Tracks) and tracks.track_of_hit.device.type == "cpu"
    assert_tracks_equal(tracks, spec)
    src, dst = batch.src.numpy(), batch.dst.numpy()
    kept = kept_restated(src, dst, e, batch.n_hits, thr, mode)
    assert np.array_equal(np.flatnonzero(spec["kept"]), kept)
    root = roots_union_find(batch.n_hits, src[kept], dst[kept])
    assert np.array_equal(spec["root"], root)
    want = tracks_from_roots(root, batch.hit_ptr, mh)
    for k in LIST_KEYS:
        assert np.array_equal(spec[k], want[k]), k


def test_hand_made_cases_give_what_they_are_made_for():
    toh = lambda name, mode="components": run_hand(name, mode)[1]["track_of_hit"].tolist()      # noqa: E731
    assert toh("chain") == [0] * 5 and toh("chain", "best") == [0] * 5
    assert toh("star") == [0, 0, 0, 0, 0, -1]
    assert toh("star", "best") == [0, -1, 0, 0, -1, -1]            # 3 -> 2 -> 0: the best in and out of hit 2
    assert toh("threshold_equal") == [0, 0, 0, 1, 1, 1]            # a score equal to the threshold joins nothing
    assert toh("nan") == [0, 0, 0, 1, 1, 1]
    assert toh("padded") == [0, 0, 0, -1]
    assert toh("self_loop") == [0, 0, 0, 1]                        # min_hits 1: the lone hit is a track
    assert toh("duplicate") == [0, 0, 0, -1] and run_hand("duplicate", "components")[1]["n_kept"] == 4
    assert run_hand("duplicate", "best")[1]["kept"].tolist() == [True, False, False, True]
    assert toh("no_hits") == [] and toh("no_segments") == [0, 1, 2, 3] and toh("no_segments_min3") == [-1] * 4
    assert toh("min_hits_edge") == [0, 0, 0, -1, -1, -1]
    assert run_hand("best_ties", "best")[1]["kept"].tolist() == [True, False, True, False, True, True]
    assert toh("best_ties", "best") == [-1, 0, -1, 0, 0, 0] and toh("best_ties") == [0] * 6
    # -0.0 and 0.0 tie: the smaller segment id wins; negative scores pass a negative threshold, in order
    assert run_hand("negative_scores", "best")[1]["kept"].tolist() == [False, True, True, False, False]
    spec = run_hand("empty_graphs", "components")[1]
    assert spec["track_graph"].tolist() == [1, 3] and spec["graph_track_ptr"].tolist() == [0, 0, 1, 1, 2, 2]


def test_status_bits_raise_where_sizes_are_read():
    tracks, spec = run_hand("nan", "components")
    assert spec["status"] == 1 and int(tracks.status) == 1 and not spec["kept"][2]
    for use in (tracks.check, lambda: len(tracks), lambda: tracks.track_ptr, lambda: tracks.match(np.zeros(6, np.int64))):
        with pytest.raises(ValueError, match="bit 1"):
            use()
    assert tracks.track_of_hit.tolist() == [0, 0, 0, 1, 1, 1]            # no read-back, no error
    assert run_hand("padded", "components")[1]["status"] == 0           # a padded segment's NaN is not looked at
    tracks, spec = run_hand("cross_graph", "components")
    assert spec["status"] == 2 and spec["root"].tolist() == [0] * 5 + [5]
    with pytest.raises(ValueError, match="bit 2.*block-diagonal"):
        tracks.check()
    # the cross-graph segment is flagged only when it is KEPT
    batch, e, thr, mh = hand_batch("cross_graph")
    e[2] = 0.4
    assert build_tracks(batch, e, thr, "components", mh).check().track_of_hit.tolist() == [0, 0, 0, -1, -1, -1]
    spec = build_tracks_numpy([0, 1, 7], [1, 2, 0], np.float32([0.9, 0.9, 0.9]), 3, [0, 3], 0.5, "components", 3)
    assert spec["status"] == 4 and spec["kept"].tolist() == [True, True, False]
    assert run_hand("chain", "best")[0].check() is not None


def test_argument_errors_come_before_any_work():
    batch, e, thr, mh = hand_batch("chain")
    for kw, what in (({"threshold": float("nan")}, "threshold"), ({"threshold": float("inf")}, "threshold"),
                     ({"min_hits": 0}, "min_hits"), ({"min_hits": 2.5}, "min_hits"), ({"mode": "walk"}, "mode")):
        with pytest.raises(ValueError, match=what):
            build_tracks(batch, e, **kw)
    with pytest.raises(ValueError, match="4 segments, the scores 3"):
        build_tracks(batch, e[:3])
    with pytest.raises(ValueError, match="particle_id has 4 entries"):
        build_tracks(batch, e).match(np.zeros(4, np.int64))
    assert gnn_fpga_amd.build_tracks is build_tracks and gnn_fpga_amd.Tracks is Tracks
    assert gnn_fpga_amd.TrackMatch is TrackMatch
    # torch CPU tensors and [B, E] shapes take the specification too
    t = build_tracks(batch, torch.from_numpy(e).reshape(2, 2))
    assert t.track_of_hit.tolist() == [0] * 5 and len(t) == 1 and t.track_hits.tolist() == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_best_mode_gives_simple_paths_on_layered_graphs(seed):
    g = synth.layered_graph(1000, 1500, seed=seed)
    scores = synth.scores_from_labels(g.y, seed=seed)
    spec = build_tracks_numpy(g.src, g.dst, scores, 1000, [0, 1000], 0.3, "best", 1)
    a, b = g.src[spec["kept"]], g.dst[spec["kept"]]
    assert spec["n_kept"] > 100
    assert np.bincount(a, minlength=1000).max() == 1 and np.bincount(b, minlength=1000).max() == 1
    assert np.diff(spec["track_ptr"]).max() <= 10                    # never more hits than layers
    comp = build_tracks_numpy(g.src, g.dst, scores, 1000, [0, 1000], 0.3, "components", 1)
    assert np.diff(comp["track_ptr"]).max() > 10                     # (what the filter is for)


@pytest.mark.parametrize("mode", ["components", "best"])
def test_a_batch_equals_its_graphs_built_alone(mode):
    graphs = [synth.layered_graph(60 + 17 * s, 150 + 40 * s, seed=s) for s in range(5)]
    scores = [synth.scores_from_labels(g.y, seed=s) for s, g in enumerate(graphs)]
    batch = HitGraphBatch.from_graphs(graphs)
    whole = build_tracks(batch, np.concatenate(scores), 0.5, mode, 3)
    toh, hits, ptr, graph_of, hit_off, t_off = [], [], [0], [], 0, 0
    for i, (g, e) in enumerate(zip(graphs, scores)):
        one = build_tracks(HitGraphBatch.from_graphs([g]), e, 0.5, mode, 3)
        t = one.track_of_hit.numpy().astype(np.int64)
        toh.append(np.where(t >= 0, t + t_off, -1))
        hits.append(one.track_hits.numpy() + hit_off)
        ptr.extend((one.track_ptr.numpy()[1:] + ptr[-1]).tolist())
        graph_of += [i] * len(one)
        hit_off += g.X.shape[0]
        t_off += len(one)
    assert len(whole) == t_off and t_off > 5
    assert np.array_equal(whole.track_of_hit.numpy(), np.concatenate(toh))
    assert np.array_equal(whole.track_hits.numpy(), np.concatenate(hits))
    assert whole.track_ptr.tolist() == ptr and whole.track_graph.tolist() == graph_of
    assert np.array_equal(np.diff(whole.graph_track_ptr.numpy()), np.bincount(graph_of, minlength=5))


def test_components_do_not_depend_on_the_order_of_the_segments():
    g, scores = layered(5)
    spec = build_tracks_numpy(g.src, g.dst, scores, 1000, [0, 1000], 0.5, "components", 3)
    p = np.random.default_rng(9).permutation(1500)
    again = build_tracks_numpy(g.src[p], g.dst[p], scores[p], 1000, [0, 1000], 0.5, "components", 3)
    for k in ("root",) + LIST_KEYS:
        assert np.array_equal(spec[k], again[k])


# ---- matching ------------------------------------------------------------------------------------------------------------
def test_matching_equals_the_counter_restatement():
    big = 2 ** 52 + 1
    #        graph 0 (hits 0 - 9)                                | graph 1 (hits 10 - 17)
    toh = [0, 0, 0, 0, 1, 1, 1, -1, 2, 2,                          3, 3, 3, 3, 4, 4, -1, -1]
    pid = [7, 7, 5, 5, 0, -3, -4, 7, big, big + 1,                 7, 7, 7, -1, big + 1, big + 1, big + 1, 5]
    hp = [0, 10, 18]
    spec = match_tracks_numpy(toh, 5, pid, hp, 2)
    assert_match_equal(type("M", (), {k: torch.from_numpy(np.asarray(v)) for k, v in spec.items()}),
                       match_restated(toh, 5, pid, hp, 2))
    # track 0: particles 5 and 7 tie at two hits, the smaller id wins; 2 x 2 is not more than its 4 hits
    # track 1: noise only; track 2: ids above 2^52 that differ by one, a tie again
    # track 3: particle 7 of GRAPH 1 (three hits there, all in the track): a particle counts once per sector graph
    # track 4: two of the three hits of particle 2^52 + 2 in graph 1
    assert spec["majority_particle"].tolist() == [5, 0, big, 7, big + 1]
    assert spec["majority_hits"].tolist() == [2, 0, 1, 3, 2] and spec["particle_hits"].tolist() == [2, 0, 1, 3, 3]
    assert spec["matched"].tolist() == [False, False, False, True, True]
    # particles with >= 2 hits: graph 0: 5 (2), 7 (3); graph 1: 7 (3), 2^52 + 2 (3)
    assert spec["counts"].tolist() == [5, 2, 4, 2]
    assert TrackMatch.rates(spec["counts"]) == (0.5, 0.6)
    assert TrackMatch.rates(spec["counts"] + spec["counts"]) == (0.5, 0.6)          # the counts add across batches


def test_matching_with_empty_denominators():
    batch, e, thr, mh = hand_batch("no_segments_min3")
    m = build_tracks(batch, e, thr, "components", mh).match(np.asarray([-1, 0, -2, 0]))
    assert m.counts.tolist() == [0, 0, 0, 0] and m.efficiency == 0.0 and m.fake_rate == 0.0
    assert m.majority_particle.numel() == 0 and m.matched.dtype == torch.bool
    batch, e, thr, mh = hand_batch("no_hits")
    m = build_tracks(batch, e).match(np.zeros(0, np.int64))
    assert m.counts.tolist() == [0, 0, 0, 0] and (m.efficiency, m.fake_rate) == (0.0, 0.0)
    batch, e, thr, mh = hand_batch("chain")                         # one noise-only track: all of it fake
    m = build_tracks(batch, e).match(np.zeros(5, np.int64))
    assert m.counts.tolist() == [1, 0, 0, 0] and (m.efficiency, m.fake_rate) == (0.0, 1.0)


@pytest.mark.parametrize("mode", ["components", "best"])
def test_matching_on_layered_graphs_equals_the_counter_restatement(mode):
    graphs = [synth.layered_graph(200, 500, seed=s) for s in range(3)]
    batch = HitGraphBatch.from_graphs(graphs)
    rng = np.random.default_rng(4)
    scores = rng.random(1500).astype(np.float32)
    pid = rng.integers(-3, 40, size=600) + np.where(rng.random(600) < 0.3, 2 ** 53, 0)
    tracks = build_tracks(batch, scores, 0.6, mode, 2)
    m = tracks.match(pid)
    assert len(tracks) > 10
    assert_match_equal(m, match_restated(tracks.track_of_hit.numpy(), len(tracks), pid, batch.hit_ptr, 2))
    assert_match_equal(m, match_spec(tracks, pid))


@pytest.mark.parametrize("row", sorted(BARREL))
def test_barrel_recipe_reproduces_the_fixed_numbers(row):
    shape, want = BARREL[row]
    batch, scores, pid = barrel_batch(row)
    assert (batch.n_graphs, batch.n_hits, batch.n_segments) == shape
    for mode, (kept, n_tracks, largest, matched, reconstructable, found) in want.items():
        tracks = build_tracks(batch, scores, 0.5, mode, 3)
        m = tracks.match(pid)
        assert int(tracks.n_kept) == kept and len(tracks) == n_tracks
        assert int(np.diff(tracks.track_ptr.numpy()).max()) == largest
        assert m.counts.tolist() == [n_tracks, matched, reconstructable, found]
        assert m.efficiency == found / reconstructable and m.fake_rate == 1 - matched / n_tracks
        assert_match_equal(m, match_restated(tracks.track_of_hit.numpy(), n_tracks, pid, batch.hit_ptr, 3))
    assert np.count_nonzero(scores > np.float32(0.5)) == want["components"][0]      # the candidates


# ---- the C ABI and the build ---------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    with open(os.path.join(REPO, "include", "gnn_hip.h")) as fh:
        hdr = fh.read()
    lib = _lib.load()
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, hdr) and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert "GNN_ABI_VERSION 7" in hdr and _lib.GNN_ABI_VERSION == 7 and lib.gnn_abi_version() == 7
    doc = hdr.split("csrc/track_build.hip; ABI 7")[1].split("gnn_track_match(")[0]
    for cite in ("reference has no counterpart", "gnn/estimator.py:137-146", "draw_sample"):
        assert cite in doc
    assert "GNN_TRACKS_COMPONENTS %d" % _lib.TRACKS_MODES["components"] in hdr
    assert "GNN_TRACKS_BEST %d" % _lib.TRACKS_MODES["best"] in hdr


def test_workspace_sizes_and_bad_arguments():
    lib = _lib.load()
    ws = lib.gnn_track_build_workspace_bytes
    for bad in ((-1, 0), (0, -1), (2 ** 31, 0), (0, 2 ** 31)):
        assert ws(*bad) == 0
    assert "n_hits" in lib.gnn_last_error().decode()
    assert 0 < ws(0, 0) < ws(100, 100) < ws(10000, 100000)
    wm = lib.gnn_track_match_workspace_bytes
    assert wm(-1, 0) == 0 and wm(2 ** 31, 0) == 0 and wm(10, 11) == 0 and "n_tracks" in lib.gnn_last_error().decode()
    assert 0 < wm(0, 0) < wm(1000, 10) < wm(1000, 1000) < wm(100000, 1000)

    sizes = (ctypes.c_int64 * 4)()
    out = ctypes.addressof(sizes)

    def labels(n_segments=0, n_hits=0, n_graphs=1, threshold=0.5, mode=0, min_hits=3, ws=None, ws_bytes=0, sizes=out):
        return lib.gnn_track_build_labels(None, None, None, n_segments, n_hits, None, n_graphs, threshold, mode,
                                          min_hits, ws, ws_bytes, None, None, sizes, None)
    for kw, name in (({"n_hits": -1}, "n_hits"), ({"n_segments": 2 ** 31}, "n_segments"), ({"n_graphs": -1}, "n_graphs"),
                     ({"threshold": float("nan")}, "threshold"), ({"threshold": float("-inf")}, "threshold"),
                     ({"mode": 2}, "mode"), ({"min_hits": 0}, "min_hits"), ({"sizes": None}, "sizes_out"),
                     ({"n_segments": 5}, "src"), ({"n_hits": 5}, "root")):
        assert labels(**kw) == _lib.GNN_ERR_BADARG, kw
        assert name in lib.gnn_last_error().decode(), (kw, lib.gnn_last_error())
    assert labels() == _lib.GNN_ERR_WORKSPACE and "workspace" in lib.gnn_last_error().decode()
    assert labels(ws=out, ws_bytes=8) == _lib.GNN_ERR_WORKSPACE

    def lists(n_hits=0, n_graphs=1, n_tracks=0, n_track_hits=0, ptr=out):
        return lib.gnn_track_build_lists(None, n_hits, None, n_graphs, n_tracks, n_track_hits, None, 0, ptr, None, None,
                                         ptr, None)
    for kw, name in (({"n_hits": -1}, "n_hits"), ({"n_graphs": 2 ** 31}, "n_graphs"), ({"n_tracks": 1}, "n_tracks"),
                     ({"n_hits": 5, "n_tracks": 2, "n_track_hits": 1}, "n_track_hits"),
                     ({"n_hits": 5, "n_tracks": 2, "n_track_hits": 6}, "n_track_hits"), ({"ptr": None}, "track_ptr"),
                     ({"n_hits": 5, "n_tracks": 1, "n_track_hits": 3}, "track_hits"), ({"n_hits": 5}, "track_of_hit")):
        assert lists(**kw) == _lib.GNN_ERR_BADARG, kw
        assert name in lib.gnn_last_error().decode(), (kw, lib.gnn_last_error())
    assert lists() == _lib.GNN_ERR_WORKSPACE

    def match(n_hits=0, n_graphs=1, n_tracks=0, min_hits=3, counts=out):
        return lib.gnn_track_match(None, None, n_hits, None, n_graphs, None, n_tracks, min_hits, None, 0, None, None,
                                   None, None, counts, None)
    for kw, name in (({"n_hits": 2 ** 31}, "n_hits"), ({"n_graphs": -1}, "n_graphs"), ({"n_tracks": 1}, "n_tracks"),
                     ({"min_hits": 0}, "min_hits"), ({"counts": None}, "counts"), ({"n_hits": 5}, "particle_id")):
        assert match(**kw) == _lib.GNN_ERR_BADARG, kw
        assert name in lib.gnn_last_error().decode(), (kw, lib.gnn_last_error())
    assert match() == _lib.GNN_ERR_WORKSPACE


def test_units_and_hand_link_scripts_name_the_unit():
    from variant_scripts import assert_variant_libraries_link
    assert_variant_libraries_link("track_build")
    with open(os.path.join(REPO, "gnn-fpga_amd", "csrc", "track_build.hip")) as fh:
        src = fh.read()
    assert src.index("#pragma clang fp contract(off)") < src.index('#include "builder_sort.h"')
    for banned in ("hipLaunchCooperativeKernel", "cooperative_groups", "atomicAdd(float", "__threadfence"):
        assert banned not in src
    assert src.count("// bounded:") >= 2                              # every open-ended loop says why it ends


def test_new_kernels_have_no_scratch():
    path = os.path.join(REPO, "build", "track_build.remarks")
    if not os.path.exists(path):
        pytest.fail("build/track_build.remarks is missing: build the library first")
    with open(path) as fh:
        text = fh.read()
    blocks = re.split(r"remark: Function Name: ", text)[1:]
    ours = [b for b in blocks if "k_tb_" in b.split()[0]]
    assert len(ours) >= 20                                        # nineteen kernels, k_tb_hook in two forms
    for b in ours:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, b.split()[0]
