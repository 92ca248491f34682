"""Track candidates from scored segments, and track-level efficiency and fake rate, on the GPU.

The reference stops at one score per segment (`Estimator.predict`, gnn/estimator.py:137-146); its notebooks draw
the scored segments (`draw_sample(..., alpha_labels=True)`) and gnn/Graph_dev.ipynb says "I haven't tried
multi-track finding yet".  This module is the stage after that: hits to tracks, and how many particles came out as
tracks.  There is nothing of the reference to compare with; the definitions below are the specification, and
`build_tracks_numpy` / `match_tracks_numpy` implement them literally.  CUDA tensors run csrc/track_build.hip,
numpy arrays and CPU tensors the specification.

Candidate segment j: src[j] >= 0 (src < 0 is a padded segment, skipped whatever its score), src[j] != dst[j], both
ends inside [0, n_hits) and scores[j] > float32(threshold) - strictly, so never for a NaN score.
Kept segments: mode "components" - every candidate; mode "best" - with bo(h) the candidate starting at hit h with
the largest score (ties, -0 = +0 among them, to the smallest segment id) and bi(h) the same among the candidates
ending at h, segment j is kept iff bo(src[j]) == j and bi(dst[j]) == j: a hit then has at most one kept segment in
and one out, and tracks are simple paths.
Root of a hit: the smallest hit id of its connected component over the kept segments, undirected.  A component of
at least `min_hits` hits is a track; tracks are numbered 0, 1, ... in ascending order of root, so - hits being
numbered graph by graph - they come out grouped by graph.
Status (0 = fine): bit 1 a NaN score on a segment with src >= 0; bit 2 a kept segment whose hits lie in different
graphs of hit_ptr (the batch is not block-diagonal); bit 4 an endpoint outside [0, n_hits) on a segment with
src >= 0 (such a segment is no candidate).

Matching: particle ids <= 0 belong to no particle (TrackML's noise id 0, synth.barrel_event's negative noise ids);
a particle is a (graph, id) pair, so one split over phi sectors counts once per sector graph.  Per track:
majority_particle - the id with the most hits in the track, ties to the smallest id, 0 when the track holds only
noise; majority_hits - its hits in the track; particle_hits - all its hits in the graph, in a track or not;
matched - 2 majority_hits > track size and 2 majority_hits > particle_hits (the strict double majority: at most one
track matches a particle).  counts int64 [4]: tracks, matched tracks, reconstructable particles (at least min_hits
hits in their graph), reconstructable particles that are the majority of a matched track.

Fit: `Tracks.fit(x, y, z)` gives every track its curvature, direction, impact parameter, z0, cot(theta) and two chi2
(`TrackFit`); `fit_tracks_numpy` is the specification and csrc/track_fit.hip equals it bit for bit - see the comment
above it.  `TrackFit.good(...)` is the quality cut, `TrackMatch.select(mask)` the counts after it.
"""
import numpy as np
import torch

from .metrics import _ratio

MODES = ("components", "best")
TB_STATUS_NAN, TB_STATUS_CROSS, TB_STATUS_RANGE = 1, 2, 4
_STATUS_WORDS = ((TB_STATUS_NAN, "bit 1: a NaN score"),
                 (TB_STATUS_CROSS, "bit 2: a kept segment joins hits of two graphs - the batch is not block-diagonal"),
                 (TB_STATUS_RANGE, "bit 4: a segment endpoint outside [0, n_hits)"))


def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _check_hit_ptr(hit_ptr, n_hits):
    hp = np.asarray(hit_ptr, dtype=np.int64).reshape(-1)
    if hp.size < 1 or hp[0] != 0 or hp[-1] != n_hits or np.any(np.diff(hp) < 0):
        raise ValueError("hit_ptr must run non-decreasing from 0 to the number of hits (%d)" % n_hits)
    return hp


def _graph_of(hit_ptr, hits):
    """The graph that owns each hit (empty graphs own none)."""
    return np.searchsorted(hit_ptr, hits, side="right") - 1


def _order_key(e):
    """uint32 keys that order float32 scores (NaN excluded by the caller), -0 and +0 the same key."""
    u = np.where(e == 0, np.float32(0), e).astype(np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def _best_of(end, key, seg, n_hits):
    """Per hit the candidate (among `seg`, whose ends are `end` and keys `key`) with the largest key, ties to the
    smallest segment id; -1 where a hit has none."""
    pack = (key.astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - seg.astype(np.uint64))
    best = np.zeros(n_hits, dtype=np.uint64)
    np.maximum.at(best, end, pack)
    return np.where(best > 0, np.int64(0xFFFFFFFF) - (best & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)


def _roots(n_hits, a, b):
    """The smallest hit id of every hit's component over the undirected segments (a[k], b[k]): rounds of "every
    component takes the smallest label among its neighbours" until nothing changes.  A label is always a hit of the
    same component and never grows, and the component's smallest hit keeps its own: at the end that is the label."""
    label = np.arange(n_hits, dtype=np.int64)
    while True:
        la, lb = label[a], label[b]
        new = label.copy()
        np.minimum.at(new, la, lb)
        np.minimum.at(new, lb, la)
        while True:                                     # follow the labels' labels to the end
            nxt = new[new]
            if np.array_equal(nxt, new):
                break
            new = nxt
        if np.array_equal(new, label):
            return label
        label = new


def build_tracks_numpy(src, dst, scores, n_hits, hit_ptr, threshold=0.5, mode="components", min_hits=3):
    """The specification on host arrays (see the module docstring).  Returns a dict: kept (bool [n_segments]),
    n_kept, root (int32 [n_hits]), track_of_hit (int32 [n_hits]), n_tracks, track_ptr (int32 [n_tracks + 1]),
    track_hits (int32), track_graph (int32 [n_tracks]), graph_track_ptr (int32 [n_graphs + 1]), status."""
    src = np.asarray(src).reshape(-1).astype(np.int64)
    dst = np.asarray(dst).reshape(-1).astype(np.int64)
    e = np.ascontiguousarray(np.asarray(scores, dtype=np.float32).reshape(-1))
    if not (src.shape == dst.shape == e.shape):
        raise ValueError("src, dst and scores differ in size")
    n_hits, min_hits = int(n_hits), int(min_hits)
    hp = _check_hit_ptr(hit_ptr, n_hits)
    real = src >= 0
    in_range = real & (src < n_hits) & (dst >= 0) & (dst < n_hits)
    status = (TB_STATUS_NAN if np.any(real & np.isnan(e)) else 0) | (TB_STATUS_RANGE if np.any(real & ~in_range) else 0)
    with np.errstate(invalid="ignore"):
        cand = in_range & (src != dst) & (e > np.float32(threshold))
    if mode == "components":
        kept = cand
    elif mode == "best":
        j = np.flatnonzero(cand)
        key = _order_key(e[j])
        bo, bi = _best_of(src[j], key, j, n_hits), _best_of(dst[j], key, j, n_hits)
        kept = np.zeros(e.size, dtype=bool)
        kept[j] = (bo[src[j]] == j) & (bi[dst[j]] == j)
    else:
        raise ValueError("mode must be one of %s, got %r" % (MODES, mode))
    a, b = src[kept], dst[kept]
    if np.any(_graph_of(hp, a) != _graph_of(hp, b)):
        status |= TB_STATUS_CROSS
    root = _roots(n_hits, a, b)
    size = np.bincount(root, minlength=n_hits)
    is_track = (root == np.arange(n_hits)) & (size >= min_hits)
    number = np.cumsum(is_track) - is_track                       # exclusive: tracks with a smaller root
    track_of_hit = np.where(is_track[root], number[root], -1) if n_hits else np.zeros(0, np.int64)
    roots = np.flatnonzero(is_track)
    n_tracks = int(roots.size)
    track_ptr = np.concatenate([[0], np.cumsum(size[roots])])
    in_track = np.flatnonzero(track_of_hit >= 0)
    track_hits = in_track[np.argsort(track_of_hit[in_track], kind="stable")]      # ascending hit id within a track
    track_graph = _graph_of(hp, roots)
    graph_track_ptr = np.searchsorted(roots, hp, side="left")                    # roots below the graph's first hit
    i32 = np.int32
    return {"kept": kept, "n_kept": int(np.count_nonzero(kept)), "root": root.astype(i32),
            "track_of_hit": track_of_hit.astype(i32), "n_tracks": n_tracks, "track_ptr": track_ptr.astype(i32),
            "track_hits": track_hits.astype(i32), "track_graph": track_graph.astype(i32),
            "graph_track_ptr": graph_track_ptr.astype(i32), "status": int(status)}


def match_tracks_numpy(track_of_hit, n_tracks, particle_id, hit_ptr, min_hits=3):
    """The specification of the matching on host arrays.  Returns a dict: majority_particle (int64 [n_tracks]),
    majority_hits, particle_hits (int32), matched (bool), counts (int64 [4])."""
    t = np.asarray(track_of_hit).reshape(-1).astype(np.int64)
    pid = np.asarray(particle_id).reshape(-1).astype(np.int64)
    if t.shape != pid.shape:
        raise ValueError("particle_id has %d entries, the batch %d hits" % (pid.size, t.size))
    n, n_tracks, min_hits = t.size, int(n_tracks), int(min_hits)
    hp = _check_hit_ptr(hit_ptr, n)
    graph = _graph_of(hp, np.arange(n))
    # particles: the distinct (graph, id) pairs with id > 0, in that order; index[h] = the hit's particle or -1
    real = np.flatnonzero(pid > 0)
    order = real[np.lexsort((pid[real], graph[real]))]
    new = np.ones(order.size, dtype=bool)
    new[1:] = (pid[order][1:] != pid[order][:-1]) | (graph[order][1:] != graph[order][:-1])
    index = np.full(n, -1, dtype=np.int64)
    index[order] = np.cumsum(new) - 1
    n_particles = int(new.sum())
    hits_of = np.bincount(index[real], minlength=n_particles)
    id_of = pid[order[new]]
    track_size = np.bincount(t[t >= 0], minlength=n_tracks)
    maj = np.zeros(n_tracks, dtype=np.int64)
    maj_hits = np.zeros(n_tracks, dtype=np.int64)
    part_hits = np.zeros(n_tracks, dtype=np.int64)
    both = np.flatnonzero((t >= 0) & (index >= 0))
    pairs, cnt = np.unique(t[both] * max(n_particles, 1) + index[both], return_counts=True)
    pt, pk = pairs // max(n_particles, 1), pairs % max(n_particles, 1)
    by = np.lexsort((pk, -cnt, pt))                     # per track: most hits first, ties to the smallest index
    first = np.ones(by.size, dtype=bool)
    first[1:] = pt[by][1:] != pt[by][:-1]
    w = by[first]
    maj[pt[w]], maj_hits[pt[w]], part_hits[pt[w]] = id_of[pk[w]], cnt[w], hits_of[pk[w]]
    matched = (2 * maj_hits > track_size) & (2 * maj_hits > part_hits)
    counts = np.array([n_tracks, np.count_nonzero(matched), np.count_nonzero(hits_of >= min_hits),
                       np.count_nonzero(matched & (part_hits >= min_hits))], dtype=np.int64)
    return {"majority_particle": maj, "majority_hits": maj_hits.astype(np.int32),
            "particle_hits": part_hits.astype(np.int32), "matched": matched, "counts": counts}


# ---- the track fit -----------------------------------------------------------------------------------------------------
# Per track, from its hits' (x, y, z) in mm: Karimaki's non-iterative circle fit (NIM A305 (1991) 187), unweighted, and a
# straight line z = z0 + cot r in (r, z) - the reference's own z0 variable (the segment cut of gnn/graph.py), not the
# arc-length fit of a true helix.  `fit_tracks_numpy` is the specification and csrc/track_fit.hip restates it operation
# for operation: float64 throughout, every operation rounded on its own (no FMA), every sum sequential over the
# track's hits in list order from 0.0.
# Sign convention: the point of closest approach to the origin is (d s, -d c), (c, s) is the direction there, pointing
# from the innermost hit to the outermost, and rho > 0 bends clockwise.
FIT_MOMENTS = ("x", "y", "z", "r2", "xx", "xy", "yy", "xr2", "yr2", "r2r2", "r", "rz", "zz")
FIT_PARAMS = ("rho", "c", "s", "d", "chi2_circle", "cot", "z0", "chi2_line")
FIT_STATUS_FEW, FIT_STATUS_MANY, FIT_STATUS_NONFINITE = 1, 2, 4
FIT_STATUS_CIRCLE, FIT_STATUS_LINE, FIT_STATUS_RANGE = 8, 16, 32
_FIT_UNFIT = FIT_STATUS_FEW | FIT_STATUS_MANY | FIT_STATUS_NONFINITE | FIT_STATUS_RANGE
_FIT_BLANK = FIT_STATUS_MANY | FIT_STATUS_NONFINITE | FIT_STATUS_RANGE
PT_GEV_PER_TESLA_MM = 2.99792458e-4            # pt [GeV] = 0.299792458 B [T] R [m]


def _check_max_hits(max_hits):
    if int(max_hits) != max_hits or max_hits < 3 or max_hits >= 2 ** 31:
        raise ValueError("max_hits must be an integer >= 3, got %r" % (max_hits,))
    return int(max_hits)


def fit_tracks_numpy(track_ptr, track_hits, x, y, z, max_hits=32):
    """The specification of the fit on host arrays (see the comment above).  track t owns
    track_hits[track_ptr[t]:track_ptr[t+1]]; x, y, z [n_hits] are cast to float64.  Returns a dict: moments float64
    [n_tracks, 13] (FIT_MOMENTS), params float64 [n_tracks, 8] (FIT_PARAMS), n_hits int32 [n_tracks], status int32
    [n_tracks]: 0 fitted; bit 1 fewer than 3 hits (moments only); bit 2 more than max_hits hits (hits not visited,
    all NaN); bit 4 a non-finite coordinate (all NaN); bit 8 degenerate circle (its five parameters NaN); bit 16
    degenerate line (its three parameters NaN); bit 32 a hit id outside [0, n_hits) (not read, all NaN).  Bits 8 and 16
    are decided only where none of 1, 2, 4 and 32 is set."""
    max_hits = _check_max_hits(max_hits)
    ptr = np.asarray(track_ptr).reshape(-1).astype(np.int64)
    hits = np.asarray(track_hits).reshape(-1).astype(np.int64)
    x, y, z = (np.ascontiguousarray(np.asarray(v).reshape(-1), dtype=np.float64) for v in (x, y, z))
    if not (x.shape == y.shape == z.shape):
        raise ValueError("x, y and z differ in size")
    if ptr.size < 1 or ptr[0] != 0 or ptr[-1] != hits.size or np.any(np.diff(ptr) < 0):
        raise ValueError("track_ptr must run non-decreasing from 0 to the number of track hits (%d)" % hits.size)
    n_hits, T = x.size, ptr.size - 1
    n = ptr[1:] - ptr[:-1]
    status = np.where(n < 3, FIT_STATUS_FEW, 0) | np.where(n > max_hits, FIT_STATUS_MANY, 0)
    visit = n <= max_hits
    S = np.zeros((13, T))
    xi, yi, ri = np.zeros(T), np.zeros(T), np.zeros(T)             # the hit of smallest r2 so far, the earlier on a tie
    xo, yo, ro = np.zeros(T), np.zeros(T), np.zeros(T)             # the hit of largest r2
    with np.errstate(all="ignore"):
        for k in range(int(n[visit].max()) if np.any(visit) else 0):
            on = np.flatnonzero(visit & (k < n))
            h = hits[ptr[on] + k]
            inside = (h >= 0) & (h < n_hits)
            status[on[~inside]] |= FIT_STATUS_RANGE
            on, h = on[inside], h[inside]
            hx, hy, hz = x[h], y[h], z[h]
            status[on[~(np.isfinite(hx) & np.isfinite(hy) & np.isfinite(hz))]] |= FIT_STATUS_NONFINITE
            r2 = hx * hx + hy * hy
            r = np.sqrt(r2)
            for m, term in enumerate((hx, hy, hz, r2, hx * hx, hx * hy, hy * hy, hx * r2, hy * r2, r2 * r2, r, r * hz,
                                      hz * hz)):
                S[m, on] = S[m, on] + term
            lo = (r2 < ri[on]) | (k == 0)
            hi = (r2 > ro[on]) | (k == 0)
            xi[on], yi[on], ri[on] = np.where(lo, hx, xi[on]), np.where(lo, hy, yi[on]), np.where(lo, r2, ri[on])
            xo[on], yo[on], ro[on] = np.where(hi, hx, xo[on]), np.where(hi, hy, yo[on]), np.where(hi, r2, ro[on])
        nf = n.astype(np.float64)
        mx, my, mz, mr2, mxx, mxy, myy, mxr, myr, mrr, mr, mrz, mzz = (S[m] / nf for m in range(13))
        Cxx, Cxy, Cyy = mxx - mx * mx, mxy - mx * my, myy - my * my
        Cxr, Cyr, Crr = mxr - mx * mr2, myr - my * mr2, mrr - mr2 * mr2
        a = 2.0 * (Crr * Cxy - Cxr * Cyr)
        b = Crr * (Cxx - Cyy) - Cxr * Cxr + Cyr * Cyr
        h = np.sqrt(a * a + b * b)
        cp = np.sqrt((1.0 + b / h) / 2.0)                          # b >= 0: the cosine first
        sp = (a / h) / (2.0 * cp)
        sq = np.sqrt((1.0 - b / h) / 2.0)                          # b < 0: the sine first, with the sign of a
        sn = np.where(a >= 0, sq, -sq)
        cn = (a / h) / (2.0 * sn)
        c, s = np.where(b >= 0, cp, cn), np.where(b >= 0, sp, sn)
        flip = c * (xo - xi) + s * (yo - yi) < 0
        c, s = np.where(flip, -c, c), np.where(flip, -s, s)
        kappa = (s * Cxr - c * Cyr) / Crr
        delta = -kappa * mr2 + s * mx - c * my
        w = 1.0 - 4.0 * delta * kappa
        u = np.sqrt(w)
        rho = 2.0 * kappa / u
        d = 2.0 * delta / (1.0 + u)
        f = 1.0 + rho * d
        chi2c = nf * f * f * (s * s * Cxx - 2.0 * s * c * Cxy + c * c * Cyy - kappa * kappa * Crr)
        Crz, Cr, Czz = mrz - mr * mz, mr2 - mr * mr, mzz - mz * mz
        cot = Crz / Cr
        z0 = mz - cot * mr
        chi2l = nf * (Czz - cot * Crz)
        fit = (status & _FIT_UNFIT) == 0
        status |= np.where(fit & ~((Crr > 0) & (h > 0) & (w > 0)), FIT_STATUS_CIRCLE, 0)
        status |= np.where(fit & ~(Cr > 0), FIT_STATUS_LINE, 0)
    nan = np.float64("nan")
    no_circle = (status & (_FIT_UNFIT | FIT_STATUS_CIRCLE)) != 0
    no_line = (status & (_FIT_UNFIT | FIT_STATUS_LINE)) != 0
    params = np.stack([np.where(no_circle, nan, v) for v in (rho, c, s, d, chi2c)] +
                      [np.where(no_line, nan, v) for v in (cot, z0, chi2l)], axis=1) if T else np.zeros((0, 8))
    moments = np.where(((status & _FIT_BLANK) != 0)[:, None], nan, S.T)
    return {"moments": np.ascontiguousarray(moments), "params": np.ascontiguousarray(params),
            "n_hits": n.astype(np.int32), "status": status.astype(np.int32)}


def xy_from_polar(r, phi):
    """float64 (x, y) = (r cos phi, r sin phi) of select_hits' columns, after the cast to float64; tensors stay tensors
    on their device, anything else comes back as numpy."""
    if torch.is_tensor(r) or torch.is_tensor(phi):
        r, phi = (torch.as_tensor(v).to(torch.float64) for v in (r, phi))
        return r * torch.cos(phi), r * torch.sin(phi)
    r, phi = np.asarray(r, dtype=np.float64), np.asarray(phi, dtype=np.float64)
    return r * np.cos(phi), r * np.sin(phi)


class TrackFit:
    """The fit of every track of a batch (`Tracks.fit`), on the tracks' device: `moments` float64 [n_tracks, 13]
    (FIT_MOMENTS), `params` float64 [n_tracks, 8] (FIT_PARAMS), `n_hits` and `status` int32 [n_tracks] (0: fitted, see
    `fit_tracks_numpy`).  Views of params: `curvature` (1/mm, > 0 bends clockwise), `direction` [n_tracks, 2] (the unit
    vector at the point of closest approach), `d0`, `z0` (mm), `cot_theta`, `chi2_circle`, `chi2_line` (mm^2).  `phi`
    and `pt()` are derived by torch ops."""

    def __init__(self, moments, params, n_hits, status):
        self.moments, self.params, self.n_hits, self.status = moments, params, n_hits, status

    curvature = property(lambda self: self.params[:, 0])
    direction = property(lambda self: self.params[:, 1:3])
    d0 = property(lambda self: self.params[:, 3])
    chi2_circle = property(lambda self: self.params[:, 4])
    cot_theta = property(lambda self: self.params[:, 5])
    z0 = property(lambda self: self.params[:, 6])
    chi2_line = property(lambda self: self.params[:, 7])

    @property
    def phi(self):
        """The direction's angle, atan2(s, c)."""
        return torch.atan2(self.params[:, 2], self.params[:, 1])

    def pt(self, b_field_tesla=2.0):
        """Transverse momentum in GeV for lengths in mm: 2.99792458e-4 B / |rho|; inf for a straight track, NaN where
        the circle was not fitted."""
        return PT_GEV_PER_TESLA_MM * float(b_field_tesla) / self.curvature.abs()

    def good(self, max_chi2_circle_per_hit, max_chi2_line_per_hit, min_hits=3):
        """bool [n_tracks]: status 0, at least min_hits hits, chi2_circle <= max_chi2_circle_per_hit * n and
        chi2_line <= max_chi2_line_per_hit * n."""
        n = self.n_hits.to(torch.float64)
        return ((self.status == 0) & (self.n_hits >= int(min_hits))
                & (self.chi2_circle <= float(max_chi2_circle_per_hit) * n)
                & (self.chi2_line <= float(max_chi2_line_per_hit) * n))


def _status_error(status):
    return ValueError("track builder status %d (%s)" % (status, "; ".join(w for b, w in _STATUS_WORDS if status & b)
                                                         or "unknown bits"))


class TrackMatch:
    """Tracks against truth particles (`Tracks.match`): per-track majority_particle (int64), majority_hits,
    particle_hits (int32), matched (bool), and `counts` int64 [4] = tracks, matched tracks, reconstructable
    particles, reconstructable particles found - on the device of the tracks.  The counts add across batches, and
    across ranks with one all_reduce.  `efficiency` and `fake_rate` read the counts back."""

    def __init__(self, majority_particle, majority_hits, particle_hits, matched, counts, min_hits=3):
        self.majority_particle, self.majority_hits = majority_particle, majority_hits
        self.particle_hits, self.matched, self.counts = particle_hits, matched, counts
        self.min_hits = int(min_hits)

    def select(self, mask):
        """The counts of the tracks where `mask` (bool [n_tracks], a TrackFit.good(...) say) is true: int64 [4] =
        selected tracks, matched ones among them, the reconstructable particles (unchanged), those of them found by a
        selected track.  `rates(match.select(mask))` is the efficiency and fake rate after the cut.  Torch ops on the
        tracks' device, nothing read back."""
        mask = torch.as_tensor(mask).to(device=self.matched.device, dtype=torch.bool).reshape(-1)
        if mask.shape != self.matched.shape:
            raise ValueError("the mask has %d entries, there are %d tracks" % (mask.numel(), self.matched.numel()))
        hit = self.matched & mask
        return torch.stack([mask.sum(), hit.sum(), self.counts[2].to(torch.int64),
                            (hit & (self.particle_hits >= self.min_hits)).sum()])

    @staticmethod
    def rates(counts):
        """(efficiency, fake_rate) of a counts vector (summed over batches or ranks, say): [3] / [2] and
        1 - [1] / [0], 0.0 on an empty denominator."""
        c = _host(counts).astype(np.int64)
        return float(_ratio(c[3], c[2])), (1.0 - float(_ratio(c[1], c[0])) if c[0] else 0.0)

    @property
    def efficiency(self):
        return self.rates(self.counts)[0]

    @property
    def fake_rate(self):
        return self.rates(self.counts)[1]


class Tracks:
    """The tracks of one batch (`build_tracks`).  Without any read-back: `track_of_hit` int32 [n_hits] (-1: the hit is
    in no track), `root_of_hit` int32 [n_hits], `n_tracks`, `n_kept` (kept segments) and `status` (0-d tensors).  At
    first use, after ONE read-back of the sizes: `track_ptr` int32 [n_tracks + 1], `track_hits` int32 (track t owns
    track_hits[track_ptr[t] : track_ptr[t+1]], ascending hit id), `track_graph` int32 [n_tracks], `graph_track_ptr`
    int32 [n_graphs + 1] and `len(tracks)`.  A nonzero status raises ValueError there, and in `check()`."""

    def __init__(self, track_of_hit, root_of_hit, sizes, hit_ptr, mode, threshold, min_hits, lists=None, ws=None,
                 hit_ptr_dev=None):
        self.track_of_hit, self.root_of_hit, self._sizes = track_of_hit, root_of_hit, sizes
        self.n_tracks, self.n_kept, self.status = sizes[0], sizes[2], sizes[3]
        self.hit_ptr = hit_ptr
        self.n_hits, self.n_graphs = int(track_of_hit.shape[0]), len(hit_ptr) - 1
        self.mode, self.threshold, self.min_hits = mode, threshold, min_hits
        self._lists, self._ws, self._hit_ptr_dev, self._host_sizes = lists, ws, hit_ptr_dev, None

    @property
    def device(self):
        return self.track_of_hit.device

    def _read(self):
        if self._host_sizes is None:
            self._host_sizes = tuple(int(v) for v in self._sizes.cpu().tolist())      # the one read-back
        if self._host_sizes[3]:
            raise _status_error(self._host_sizes[3])
        return self._host_sizes

    def check(self):
        """Raise ValueError if the builder flagged its input (reads the sizes back)."""
        self._read()
        return self

    def _fill(self):
        n_tracks, n_track_hits = self._read()[:2]
        if self._lists is None:
            from . import _lib
            self._lists = _lib.track_build_lists(self._ws, self.track_of_hit, self._hit_ptr_dev, n_tracks, n_track_hits)
            self._ws = None
        return self._lists

    track_ptr = property(lambda self: self._fill()[0])
    track_hits = property(lambda self: self._fill()[1])
    track_graph = property(lambda self: self._fill()[2])
    graph_track_ptr = property(lambda self: self._fill()[3])

    def __len__(self):
        return self._read()[0]

    def match(self, particle_id):
        """Match the tracks to truth particles: particle_id int64 [n_hits] in the batch's hit order
        (pid[batch.hit_index] for a batch of build_graphs).  Returns a TrackMatch."""
        n = int(particle_id.numel() if torch.is_tensor(particle_id) else np.asarray(particle_id).size)
        if n != self.n_hits:
            raise ValueError("particle_id has %d entries, the batch %d hits" % (n, self.n_hits))
        n_tracks = len(self)
        if self.track_of_hit.is_cuda:
            from . import _lib
            pid = torch.as_tensor(particle_id).reshape(-1).to(device=self.device, dtype=torch.int64).contiguous()
            maj, mh, ph, matched, counts = _lib.track_match(self.track_of_hit, pid, self._hit_ptr_dev, self.track_ptr,
                                                            n_tracks, self.min_hits)
            return TrackMatch(maj, mh, ph, matched.to(torch.bool), counts, self.min_hits)
        spec = match_tracks_numpy(self.track_of_hit.numpy(), n_tracks, _host(particle_id), self.hit_ptr, self.min_hits)
        t = torch.from_numpy
        return TrackMatch(t(spec["majority_particle"]), t(spec["majority_hits"]), t(spec["particle_hits"]),
                          t(spec["matched"]), t(spec["counts"]), self.min_hits)

    def fit(self, x, y, z, max_hits=32):
        """Fit every track: x, y, z [n_hits] in the batch's hit order, in mm (col[batch.hit_index] for a batch of
        build_graphs; `xy_from_polar` makes x, y of select_hits' r, phi), tensors or numpy, float32 or float64.  CUDA
        tracks run csrc/track_fit.hip, CPU tracks `fit_tracks_numpy`; tracks of more than `max_hits` hits are flagged,
        not fitted.  Returns a TrackFit."""
        max_hits = _check_max_hits(max_hits)
        for name, v in (("x", x), ("y", y), ("z", z)):
            n = int(v.numel() if torch.is_tensor(v) else np.asarray(v).size)
            if n != self.n_hits:
                raise ValueError("%s has %d entries, the batch %d hits" % (name, n, self.n_hits))
        track_ptr, track_hits = self.track_ptr, self.track_hits          # (the one read-back, if not yet made)
        if self.track_of_hit.is_cuda:
            from . import _lib
            cols = [torch.as_tensor(v).reshape(-1).to(device=self.device, dtype=torch.float64).contiguous()
                    for v in (x, y, z)]
            return TrackFit(*_lib.track_fit(track_ptr, track_hits, *cols, max_hits))
        spec = fit_tracks_numpy(track_ptr.numpy(), track_hits.numpy(), _host(x), _host(y), _host(z), max_hits)
        return TrackFit(*(torch.from_numpy(spec[k]) for k in ("moments", "params", "n_hits", "status")))


def build_tracks(batch, scores, threshold=0.5, mode="components", min_hits=3):
    """Tracks of a HitGraphBatch from its segments' scores (float32 [n_segments], or [B, E] as SegmentClassifier
    returns them for a dense-shaped batch).  CUDA scores (the batch on the same device) run the kernels,
    asynchronously and without a read-back; CPU tensors and numpy arrays run `build_tracks_numpy`.  Returns Tracks."""
    if mode not in MODES:
        raise ValueError("mode must be one of %s, got %r" % (MODES, mode))
    if not np.isfinite(threshold):
        raise ValueError("threshold must be finite, got %r" % (threshold,))
    if int(min_hits) != min_hits or min_hits < 1:
        raise ValueError("min_hits must be an integer >= 1, got %r" % (min_hits,))
    n = int(scores.numel() if torch.is_tensor(scores) else np.asarray(scores).size)
    if n != batch.n_segments:
        raise ValueError("the batch has %d segments, the scores %d" % (batch.n_segments, n))
    if batch.n_hits >= 2 ** 31 or batch.n_segments >= 2 ** 31:
        raise ValueError("n_hits and n_segments must be below 2^31")
    threshold, min_hits = float(np.float32(threshold)), int(min_hits)
    hp = _check_hit_ptr(batch.hit_ptr, batch.n_hits)
    if torch.is_tensor(scores) and scores.is_cuda:
        from . import _lib
        dev = scores.device
        if not batch.src.is_cuda or batch.src.device != dev:
            raise ValueError("the scores are on %s, the batch on %s" % (dev, batch.src.device))
        e = scores.detach().reshape(-1)
        e = e if e.dtype == torch.float32 and e.is_contiguous() else e.to(torch.float32).contiguous()
        hpd = batch.derived("device", "hit_ptr", lambda b: torch.from_numpy(hp).to(dev))    # uploaded once per device
        ws, root, track_of_hit, sizes = _lib.track_build_labels(batch.src, batch.dst, e, batch.n_hits, hpd, threshold,
                                                                mode, min_hits)
        return Tracks(track_of_hit, root, sizes, hp, mode, threshold, min_hits, ws=ws, hit_ptr_dev=hpd)
    spec = build_tracks_numpy(_host(batch.src), _host(batch.dst), _host(scores), batch.n_hits, hp, threshold, mode,
                              min_hits)
    t = torch.from_numpy
    sizes = torch.tensor([spec["n_tracks"], spec["track_hits"].size, spec["n_kept"], spec["status"]], dtype=torch.int64)
    lists = tuple(t(spec[k]) for k in ("track_ptr", "track_hits", "track_graph", "graph_track_ptr"))
    return Tracks(t(spec["track_of_hit"]), t(spec["root"]), sizes, hp, mode, threshold, min_hits, lists=lists)
