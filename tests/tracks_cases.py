"""Inputs the track builder's host and GPU tests share: the hand-made cases, the barrel recipe of the issue's table,
independent restatements of the definitions in plain Python, and the array-for-array comparison."""
from collections import Counter

import numpy as np
import torch

from gnn_fpga_amd import HitGraphBatch, build_graphs, synth
from gnn_fpga_amd.tracks import build_tracks_numpy, match_tracks_numpy

NAN = float("nan")

# name -> (n_hits, [(src, dst, score), ...], hit_ptr or None, threshold, min_hits)
HAND = {
    "chain": (5, [(0, 1, 0.9), (1, 2, 0.8), (2, 3, 0.7), (3, 4, 0.6)], None, 0.5, 3),
    "star": (6, [(2, 0, 0.9), (2, 1, 0.8), (3, 2, 0.7), (4, 2, 0.6)], None, 0.5, 3),
    # {0, 1, 2} and {3, 4, 5} joined only by a segment whose score EQUALS the threshold: not joined
    "threshold_equal": (6, [(0, 1, 0.9), (1, 2, 0.9), (2, 3, 0.5), (3, 4, 0.9), (4, 5, 0.9)], None, 0.5, 3),
    "nan": (6, [(0, 1, 0.9), (1, 2, 0.9), (2, 3, NAN), (3, 4, 0.9), (4, 5, 0.9)], None, 0.5, 3),
    "padded": (4, [(0, 1, 0.9), (-1, -1, 0.99), (1, 2, 0.9), (-1, -1, NAN), (-1, -1, 0.99)], None, 0.5, 3),
    "self_loop": (4, [(0, 1, 0.9), (1, 1, 0.99), (1, 2, 0.9), (3, 3, 0.99)], None, 0.5, 1),
    "duplicate": (4, [(0, 1, 0.9), (0, 1, 0.9), (1, 2, 0.7), (1, 2, 0.8)], None, 0.5, 3),
    "no_hits": (0, [], None, 0.5, 3),
    "no_segments": (4, [], None, 0.5, 1),
    "no_segments_min3": (4, [], None, 0.5, 3),
    # components of exactly min_hits (3) and min_hits - 1 (2) hits
    "min_hits_edge": (6, [(0, 1, 0.9), (1, 2, 0.9), (3, 4, 0.9)], None, 0.5, 3),
    "cross_graph": (6, [(0, 1, 0.9), (1, 2, 0.9), (2, 3, 0.9), (3, 4, 0.9), (4, 5, 0.2)], (0, 3, 6), 0.5, 3),
    # hit 0 starts two segments of equal score, hit 3 ends two: the smallest segment id wins
    "best_ties": (6, [(0, 2, 0.75), (0, 1, 0.75), (1, 3, 0.75), (2, 3, 0.75), (3, 4, 0.9), (4, 5, 0.9)], None, 0.5, 3),
    "negative_scores": (5, [(0, 1, -0.5), (0, 2, -0.25), (2, 3, -0.0), (2, 4, 0.0), (1, 3, -1.5)], None, -1.0, 2),
    "empty_graphs": (6, [(0, 1, 0.9), (1, 2, 0.9), (3, 4, 0.9), (4, 5, 0.9)], (0, 0, 3, 3, 6, 6), 0.5, 3),
}


def hand_batch(name):
    """(HitGraphBatch on the CPU, scores float32, threshold, min_hits) of a hand-made case."""
    n, segs, hp, thr, mh = HAND[name]
    src = np.asarray([s[0] for s in segs], dtype=np.int32)
    dst = np.asarray([s[1] for s in segs], dtype=np.int32)
    e = np.asarray([s[2] for s in segs], dtype=np.float32)
    hp = [0, n] if hp is None else list(hp)
    sp = [0] + [len(segs)] * (len(hp) - 1)
    return HitGraphBatch(np.zeros((n, 3), np.float32), src, dst, hit_ptr=hp, seg_ptr=sp), e, thr, mh


def spec_of(batch, scores, threshold, mode, min_hits):
    s = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)      # noqa: E731
    return build_tracks_numpy(s(batch.src), s(batch.dst), s(scores).reshape(-1), batch.n_hits, batch.hit_ptr, threshold,
                              mode, min_hits)


def assert_tracks_equal(tracks, spec):
    """Every array of a Tracks against the specification's dict, element for element."""
    h = lambda t: t.detach().cpu().numpy()               # noqa: E731
    assert tracks.track_of_hit.dtype == torch.int32 and tracks.root_of_hit.dtype == torch.int32
    assert tracks.n_tracks.dim() == 0 and tracks.status.dim() == 0
    assert int(tracks.status) == spec["status"]
    assert np.array_equal(h(tracks.root_of_hit), spec["root"])
    assert np.array_equal(h(tracks.track_of_hit), spec["track_of_hit"])
    assert int(tracks.n_tracks) == spec["n_tracks"] and int(tracks.n_kept) == spec["n_kept"]
    if spec["status"]:
        return
    assert len(tracks) == spec["n_tracks"]
    for k in ("track_ptr", "track_hits", "track_graph", "graph_track_ptr"):
        got = getattr(tracks, k)
        assert got.dtype == torch.int32 and got.device == tracks.track_of_hit.device, k
        assert np.array_equal(h(got), spec[k]), k


def assert_match_equal(m, spec):
    h = lambda t: t.detach().cpu().numpy()               # noqa: E731
    assert m.majority_particle.dtype == torch.int64 and m.counts.dtype == torch.int64 and m.matched.dtype == torch.bool
    for k in ("majority_particle", "majority_hits", "particle_hits", "matched", "counts"):
        assert np.array_equal(h(getattr(m, k)), spec[k]), k


def match_spec(tracks, particle_id):
    s = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)      # noqa: E731
    return match_tracks_numpy(s(tracks.track_of_hit), len(tracks), s(particle_id), tracks.hit_ptr, tracks.min_hits)


# ---- independent restatements ------------------------------------------------------------------------------------------
def kept_restated(src, dst, scores, n_hits, threshold, mode):
    """The kept segments, segment by segment in plain Python."""
    thr = np.float32(threshold)
    cand = [j for j in range(len(src)) if 0 <= src[j] < n_hits and 0 <= dst[j] < n_hits and src[j] != dst[j]
            and scores[j] > thr]
    if mode == "components":
        return cand
    bo, bi = {}, {}
    for j in cand:                                       # ascending id: a later segment wins only with a LARGER score
        if src[j] not in bo or scores[j] > scores[bo[src[j]]]:
            bo[src[j]] = j
        if dst[j] not in bi or scores[j] > scores[bi[dst[j]]]:
            bi[dst[j]] = j
    return [j for j in cand if bo[src[j]] == j and bi[dst[j]] == j]


def roots_union_find(n_hits, a, b):
    parent = list(range(n_hits))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for u, v in zip(a, b):
        ru, rv = find(int(u)), find(int(v))
        if ru != rv:
            parent[max(ru, rv)] = min(ru, rv)
    return np.asarray([find(x) for x in range(n_hits)], dtype=np.int64)


def tracks_from_roots(root, hit_ptr, min_hits):
    """Numbering and lists from the roots alone, in plain Python."""
    members = {}
    for h, r in enumerate(root.tolist()):
        members.setdefault(r, []).append(h)
    tracks = [members[r] for r in sorted(members) if len(members[r]) >= min_hits]
    toh = np.full(len(root), -1, dtype=np.int32)
    for t, hits in enumerate(tracks):
        toh[hits] = t
    hp = list(hit_ptr)
    graph = [max(g for g in range(len(hp) - 1) if hp[g] <= hits[0] < hp[g + 1]) for hits in tracks]
    gptr = [sum(1 for hits in tracks if hits[0] < hp[g]) for g in range(len(hp))]
    return {"track_of_hit": toh, "n_tracks": len(tracks),
            "track_ptr": np.cumsum([0] + [len(t) for t in tracks]).astype(np.int32),
            "track_hits": np.asarray([h for t in tracks for h in t], dtype=np.int32),
            "track_graph": np.asarray(graph, dtype=np.int32), "graph_track_ptr": np.asarray(gptr, dtype=np.int32)}


def match_restated(track_of_hit, n_tracks, pid, hit_ptr, min_hits):
    hp = list(hit_ptr)
    graph = [g for g in range(len(hp) - 1) for _ in range(hp[g + 1] - hp[g])]
    pid = [int(p) for p in pid]
    particle = Counter((graph[h], pid[h]) for h in range(len(pid)) if pid[h] > 0)
    votes = [Counter() for _ in range(n_tracks)]
    size = [0] * n_tracks
    for h, t in enumerate(np.asarray(track_of_hit).tolist()):
        if t >= 0:
            size[t] += 1
            if pid[h] > 0:
                votes[t][(graph[h], pid[h])] += 1
    maj, mh, ph, matched = [], [], [], []
    for t in range(n_tracks):
        if votes[t]:
            key, c = min(votes[t].items(), key=lambda kv: (-kv[1], kv[0][1]))
            maj.append(key[1]); mh.append(c); ph.append(particle[key])
        else:
            maj.append(0); mh.append(0); ph.append(0)
        matched.append(2 * mh[-1] > size[t] and 2 * mh[-1] > ph[-1])
    counts = [n_tracks, sum(matched), sum(1 for c in particle.values() if c >= min_hits),
              sum(1 for t in range(n_tracks) if matched[t] and ph[t] >= min_hits)]
    return {"majority_particle": np.asarray(maj, dtype=np.int64), "majority_hits": np.asarray(mh, dtype=np.int32),
            "particle_hits": np.asarray(ph, dtype=np.int32), "matched": np.asarray(matched, dtype=bool),
            "counts": np.asarray(counts, dtype=np.int64)}


# ---- the barrel recipe --------------------------------------------------------------------------------------------------
# (n_tracks, n_noise, n_events, sectors, seed) -> graphs, hits, segments and, per mode, (kept, tracks, largest track,
# matched, reconstructable, found): a prototype of the definitions, checked against scipy, gave these numbers
BARREL = {
    (40, 40, 2, 1, 3): ((2, 880, 1436), {"components": (846, 28, 141, 13, 80, 13), "best": (716, 85, 10, 79, 80, 79)}),
    (300, 300, 2, 2, 4): ((4, 6600, 43625), {"components": (11790, 8, 1770, 4, 623, 4),
                                             "best": (5175, 743, 10, 577, 623, 577)}),
}
BARREL_PAIRS = [(i, i + 1) for i in range(9)]


def barrel_batch(row, device=None):
    """(batch, scores float32, particle_id int64 [n_hits] in the batch's hit order) of a row of BARREL; on `device`
    the graphs are built there."""
    n_tracks, n_noise, n_events, k, seed = row
    ev = synth.barrel_event(n_tracks, n_noise, n_events, seed=seed)
    cols = [ev.r, ev.phi, ev.z, ev.layer]
    pid = ev.particle_id
    if device is not None:
        cols = [torch.from_numpy(c).to(device) for c in cols]
        pid = torch.from_numpy(pid).to(device)
    batch = build_graphs(*cols, BARREL_PAIRS, particle_id=pid, event_ptr=ev.event_ptr, n_phi_sectors=k,
                         phi_slope_max=0.002, z0_max=400.0)
    y = batch.y.cpu().numpy()
    scores = synth.scores_from_labels(y, seed=seed)
    hit_pid = pid[batch.hit_index]
    if device is not None:
        scores = torch.from_numpy(scores).to(device)
    return batch, scores, hit_pid


# ---- paths and stars ----------------------------------------------------------------------------------------------------
def path_graph(n, numbering, seed):
    """One path of n hits as a synth.HitGraph with scores: hit ids along the path `ascending`, `descending` or in a
    seeded `permuted` order; the segments in a seeded shuffled order; all scores distinct, in (0.6, 0.9]."""
    rng = np.random.default_rng(seed)
    ids = {"ascending": np.arange(n), "descending": np.arange(n)[::-1], "permuted": rng.permutation(n)}[numbering]
    order = rng.permutation(n - 1)
    src, dst = ids[:-1][order].astype(np.int32), ids[1:][order].astype(np.int32)
    scores = (0.6 + 0.3 * (rng.permutation(n - 1) + 1) / (n - 1)).astype(np.float32)
    assert np.unique(scores).size == n - 1
    return synth.HitGraph(np.zeros((n, 3), np.float32), src, dst, np.ones(n - 1, np.float32)), scores
