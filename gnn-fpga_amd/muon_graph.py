"""Muon trigger graphs from EMTF hits: the reference's muon graph preparation on the GPU.

Replaces gnn/prepareMuonGraphs.py `main` from the `tree.pandas.df` reads (:171-173) through `save_graphs` (:263) for
one (muon file, PU file) pair, with gnn/Muon_graph.py `construct_graph` (:119-162) and its segment selection
(:60-115).  `build_muon_graphs` returns every graph the reference's regrouping makes, in its order (ascending
entry), as one HitGraphBatch with F = 11, plus the file each graph would be saved to or not.

Inputs: `muon` and `pu` are mappings with the ten hit_features columns of :169-170 (HIT_FEATURES: float32 z,
theta, phi, r; integer bend, tp1, tp2, station, ring, type) and `event_ptr` [n_entries + 1]; entry entry_start + e
owns rows event_ptr[e] .. event_ptr[e+1], the subentry is the position in the entry.  `vp_pt`, `vp_eta` are the flat
rows of the vp frame (:173).

What it computes, exactly as the reference does (line numbers of prepareMuonGraphs.py unless marked):

* layer: L = EMTF_LUT[type, station, ring] (:49-92, :175-176), -99 when the chamber has none;
* cross-frame filter (:178-179): row (e, s) survives in BOTH sources iff both sources have row (e, s) and both rows
  have L != -99 (the two lines align the frames on (entry, subentry); the second one filters PU against the already
  filtered muon frame), so a PU entry is cut to the muon entry's row count;
* signed layer (:189-190): L * np.sign(z) in float64; z = +-0 gives +0 (np.sign(-0.0) is +0.0): a node no
  layer pair uses;
* truth filter (:192) on muon rows only: tp1 == 0 and tp2 == 0;
* deduplication (:202, :209): per source and entry the first row of every (type, station, ring) in row order (the
  z sign is not part of the key), after the filters; at most 21 rows per source (EMTF_LUT has 21 chambers);
* mixing by ordinal (:193-213): the k-th PU entry that has rows is mixed with the k-th muon entry that has rows,
  PU rows first; PU entries with k >= the number of such muon entries are dropped.  The mixed frames are then
  regrouped by entry (:232): graph e holds the muon rows of e and the PU rows of e, muon rows first when
  muon ordinal(e) < PU ordinal(e) (an earlier entry lost all its muon rows to the truth filter), PU rows first
  otherwise.  muon_only (`--muononly`, :35-36, :230; any value given on the command line is true): the
  deduplicated muon rows only;
* layer pairs (:234-246): the distinct signed layers in Python set iteration order (`set_order`, an exact emulation
  of CPython 3's set insertion for these <= 25 values, pinned to the interpreter by a test), the positive ones
  P and the negative ones M in that order, pairs (P[i], P[i+1]) then (M[i+1], M[i]);
* segments (Muon_graph.py:60-115): per pair, every l1 hit in frame order with every l2 hit in frame order, float32
  and in this order of operations: dphi = phi2 - phi1, minus f32(2 pi) if > f32(pi), then plus f32(2 pi) if
  < -f32(pi); phi_slope = dphi / (r2 - r1); z0 = z1 - (r1 * (z2 - z1)) / (r2 - r1); kept iff
  |phi_slope| < f32(10e30) and |z0| < f32(10e30), so r2 == r1 (inf or NaN) is never kept; src = the l1 hit (Ro),
  dst = the l2 hit (Ri);
* X (Muon_graph.py:142) = float32(float64(column)) for the ten features, then the signed layer; y = 1.0 iff both
  hits are muon rows (Muon_graph.py:155-157);
* pt, eta (:254): row e of the flat vp frame (entry - start), not the vp row of entry e: an entry with zero or two
  vp rows shifts every later graph, as in the reference;
* written (Muon_graph.py:134-138, :198-204): a graph with no layer pair makes pd.concat([]) raise, so
  construct_graph returns None and save_graph writes no file; the file numbers still count it.  A graph whose pairs
  keep no segment is written, with zero segments.

Differences from the reference: (1) a type, station or ring outside [0, 5) (the reference's numpy index wraps a
negative one and raises on one >= 5), a non-finite z anywhere in either input and a malformed event_ptr raise
ValueError (the device builder flags them in its status word); (2) where the vp row of a graph does not exist the
reference raises IndexError: here pt = eta = NaN and `vp_missing` is set for that graph; (3) integer columns must
have an integer dtype of at most 32 bits (the reference takes whatever ROOT gives), float columns float32;
(4) graphs that are not written are still in the batch (`written` False), with their hits and no segments.

CUDA tensors run csrc/muon_graph.hip (two calls around one read-back of the sizes, or layout="padded": fixed slots
and no read-back at all); numpy arrays or CPU tensors run `build_muon_graphs_numpy`, the specification.
"""
import numpy as np
import torch

from .graph_build import _host, _raise_builder_status, wrap_dphi32
from .hitgraph import HitGraphBatch

HIT_FEATURES = ("vh_sim_z", "vh_sim_theta", "vh_sim_phi", "vh_sim_r", "vh_bend", "vh_sim_tp1", "vh_sim_tp2",
                "vh_station", "vh_ring", "vh_type")
FLOAT_COLUMNS = HIT_FEATURES[:4]
INT_COLUMNS = HIT_FEATURES[4:]
N_FEATURES = len(HIT_FEATURES) + 1          # + the signed layer (:225)

# gnn/prepareMuonGraphs.py:71-92: (type, station, ring) -> layer; every other index of the [5, 5, 5] table is -99
EMTF_LUT = {(1, 1, 4): 3, (1, 1, 1): 3, (1, 1, 2): 4, (1, 1, 3): 4, (1, 2, 1): 8, (1, 2, 2): 8, (1, 3, 1): 9,
            (1, 3, 2): 9, (1, 4, 1): 11, (1, 4, 2): 11, (2, 1, 2): 5, (2, 2, 2): 6, (2, 3, 1): 10, (2, 3, 2): 10,
            (2, 3, 3): 10, (2, 4, 1): 12, (2, 4, 2): 12, (2, 4, 3): 12, (3, 1, 1): 2, (3, 2, 1): 7, (4, 1, 1): 1}
LUT_SIZE = 5
MAX_GRAPH_HITS = 2 * len(EMTF_LUT)          # 21 chambers per source survive the deduplication: 42, exact
MAX_GRAPH_SEGMENTS = len(EMTF_LUT) ** 2     # the pairs form a bipartite graph over <= 42 hits: <= 21 * 21
MAX_ENTRIES = (2 ** 31 - 1) // MAX_GRAPH_SEGMENTS   # padded segment slots stay int32

MG_STATUS_INDEX = 1       # csrc/muon_graph.hip: a type, station or ring outside [0, 5)
MG_STATUS_FINITE = 2      # a non-finite z
MG_STATUS_EVENTS = 4      # an event_ptr not 0 .. n_rows, non-decreasing (or an entry of 2^31 rows or more)
_STATUS_WORDS = ((MG_STATUS_INDEX, "a type, station or ring outside [0, 5)"), (MG_STATUS_FINITE, "a non-finite z"),
                 (MG_STATUS_EVENTS, "malformed event_ptr"))
# per-graph flags of the device builder
MG_GRAPH_PRESENT, MG_GRAPH_WRITTEN, MG_GRAPH_VP_MISSING = 1, 2, 4

_CUT32 = np.float32(10e30)                  # Muon_graph.py:60: phi_slope_max = z0_max = 10e30, compared in float32


def lut_array():
    """EMTF_LUT as the reference's int32 [5, 5, 5] table."""
    t = np.full((LUT_SIZE,) * 3, -99, dtype=np.int32)
    for k, v in EMTF_LUT.items():
        t[k] = v
    return t


def _py_hash(v):
    """CPython's hash of an integral float: the integer, except hash(-1.0) == -2."""
    h = int(v)
    return -2 if h == -1 else h


def set_order(values):
    """list(set(values)) for integral floats, by emulating CPython's set insertion (Objects/setobject.c): a table of
    8 slots, linear probes of up to 9 slots while they stay inside the table, then perturbed probing (PERTURB_SHIFT
    5, perturb = the hash as an unsigned 64-bit word); after an insertion into an empty slot with fill * 5 >=
    mask * 3 the table grows to the first power of two above 4 * used and the entries are reinserted in slot
    order.  Iteration is in slot order.  Equal values (0.0 and -0.0 included) keep the first one inserted."""
    mask, table, fill = 7, [None] * 8, 0

    def probe(table, mask, h, v):
        """The slot v is in (found True) or goes to (found False)."""
        i = h & mask
        perturb = h % (1 << 64)
        while True:
            if table[i] is None:
                return i, False
            if table[i] == v:
                return i, True
            if i + 9 <= mask:
                for j in range(i + 1, i + 10):
                    if table[j] is None:
                        return j, False
                    if table[j] == v:
                        return j, True
            perturb >>= 5
            i = (i * 5 + 1 + perturb) & mask

    for v in values:
        v = float(v)
        slot, found = probe(table, mask, _py_hash(v), v)
        if found:
            continue
        table[slot] = v
        fill += 1
        if fill * 5 >= mask * 3:
            size = 8
            while size <= fill * 4:
                size <<= 1
            old, table, mask = table, [None] * size, size - 1
            for w in old:
                if w is not None:
                    table[probe(table, mask, _py_hash(w), w)[0]] = w
    return [v for v in table if v is not None]


def layer_pairs(order):
    """gnn/prepareMuonGraphs.py:236-246: consecutive positive values, then consecutive negative values reversed."""
    p = [v for v in order if v > 0.0]
    m = [v for v in order if v < 0.0]
    return [(p[i], p[i + 1]) for i in range(len(p) - 1)] + [(m[i + 1], m[i]) for i in range(len(m) - 1)]


class MuonGraphs:
    """The result of build_muon_graphs.

    batch        HitGraphBatch, X [N, 11] float32, src / dst int32, y float32; graph g = hits hit_ptr[g] ..
                 hit_ptr[g+1], segments seg_ptr[g] .. seg_ptr[g+1]
    entry        [G] int64: the entry of each graph (entry_start + e)
    pt, eta      [G] float32: from vp row e (NaN where that row does not exist: vp_missing)
    written      [G] bool: False where the reference writes no file (no layer pair)
    vp_missing   [G] bool
    hit_source   [N] int8 (numpy) / int32 (device): 0 = PU row, 1 = muon row (-1: a padding hit)
    hit_row      [N] int64: the hit's row in its source's columns (-1: a padding hit)
    layout       "flat": the graphs back to back; "padded": graph slot e (entry entry_start + e, present or not) owns
                 hits [42 e, 42 e + 42) and segments [441 e, 441 e + 441); unused hits are X = 0 rows, unused
                 segments src = dst = -1 with y = 0
    present      [G] bool: the slot holds a graph (always True for "flat")
    n_hits, n_segments  [G] int32 per graph (padded: the used part of each slot)
    status       device int32 [1] of the padded layout (0 = fine; check() raises on anything else), else None
    """

    def __init__(self, batch, entry, pt, eta, written, vp_missing, hit_source, hit_row, layout="flat", present=None,
                 n_hits=None, n_segments=None, status=None, entry_start=0):
        self.batch, self.entry, self.pt, self.eta = batch, entry, pt, eta
        self.entry_start = entry_start
        self.written, self.vp_missing, self.hit_source, self.hit_row = written, vp_missing, hit_source, hit_row
        self.layout, self.status = layout, status
        self.present = present
        self.n_hits, self.n_segments = n_hits, n_segments

    @property
    def n_graphs(self):
        return self.batch.n_graphs

    def check(self):
        """Raise ValueError if the padded build flagged its input (reads the status word back: a synchronisation)."""
        if self.status is not None:
            _raise_status(int(self.status.cpu()[0]))
        return self


def _raise_status(st):
    _raise_builder_status("muon graph builder", _STATUS_WORDS, st)


def _columns(src, name, device):
    """Validate one source's columns; returns {column: array or tensor} with event_ptr int64."""
    try:
        cols = {k: src[k] for k in HIT_FEATURES + ("event_ptr",)}
    except (KeyError, TypeError, IndexError):
        raise ValueError("%s needs the columns %s and event_ptr" % (name, ", ".join(HIT_FEATURES))) from None
    n = None
    for k in HIT_FEATURES:
        c = cols[k]
        if device != (torch.is_tensor(c) and c.is_cuda):
            raise ValueError("%s.%s: every column must be a CUDA tensor or every one a host array" % (name, k))
        dt = c.dtype
        if k in FLOAT_COLUMNS:
            if dt in (np.float64, torch.float64):
                raise ValueError("%s.%s is float64: the reference's cuts are float32 arithmetic on float32 columns; "
                                 "convert explicitly if that is what you mean" % (name, k))
            if dt not in (np.float32, torch.float32):
                raise ValueError("%s.%s must be float32, got %s" % (name, k, dt))
        elif torch.is_tensor(c):
            if dt not in (torch.int8, torch.int16, torch.int32, torch.uint8):
                raise ValueError("%s.%s must be an integer tensor of at most 32 bits, got %s" % (name, k, dt))
        elif not (np.issubdtype(dt, np.integer) and np.dtype(dt).itemsize <= 4 and dt != np.uint32):
            raise ValueError("%s.%s must be an integer array of at most 32 bits, got %s" % (name, k, dt))
        if len(c.shape) != 1:
            raise ValueError("%s.%s must be one-dimensional" % (name, k))
        if n is None:
            n = int(c.shape[0])
        elif int(c.shape[0]) != n:
            raise ValueError("%s.%s has %d rows, %s.%s has %d" % (name, k, int(c.shape[0]), name, HIT_FEATURES[0], n))
    ep = cols["event_ptr"]
    if len(ep.shape) != 1 or int(ep.shape[0]) < 1:
        raise ValueError("%s.event_ptr must be one-dimensional with n_entries + 1 values" % name)
    if device:
        if not torch.is_tensor(ep) or ep.device != cols["vh_sim_z"].device:
            raise ValueError("%s.event_ptr must be a tensor on %s" % (name, cols["vh_sim_z"].device))
        if ep.dtype.is_floating_point or ep.dtype == torch.bool:
            raise ValueError("%s.event_ptr must be integer" % name)
        cols["event_ptr"] = ep.to(torch.int64).contiguous()
        for k in HIT_FEATURES:
            cols[k] = cols[k].contiguous() if k in FLOAT_COLUMNS else cols[k].to(torch.int32).contiguous()
    else:
        ep = _host(ep)
        if not np.issubdtype(ep.dtype, np.integer):
            raise ValueError("%s.event_ptr must be integer" % name)
        ep = ep.astype(np.int64)
        if ep[0] != 0 or ep[-1] != n or np.any(np.diff(ep) < 0):
            raise ValueError("%s.event_ptr must run non-decreasing from 0 to the number of rows (%d)" % (name, n))
        cols["event_ptr"] = ep
        for k in HIT_FEATURES:
            cols[k] = _host(cols[k]).astype(np.float32 if k in FLOAT_COLUMNS else np.int64)
    return cols, n


def build_muon_graphs(muon, pu, vp_pt, vp_eta, *, entry_start=0, muon_only=False, layout="flat"):
    """Every muon graph of one (muon, PU) pair of inputs (see the module docstring): a MuonGraphs.

    CUDA tensors run the HIP builder: layout="flat" reads the sizes back once between its two calls; "padded" reads
    nothing back (malformed input is then reported by `result.check()`), so build and model(result.batch) can run
    without a host synchronisation between them.  numpy arrays run the specification."""
    if layout not in ("flat", "padded"):
        raise ValueError("layout must be 'flat' or 'padded'")
    device = torch.is_tensor(muon.get("vh_sim_z") if hasattr(muon, "get") else None) and muon["vh_sim_z"].is_cuda
    mu, n_mu = _columns(muon, "muon", device)
    pu_, n_pu = _columns(pu, "pu", device)
    E = int(mu["event_ptr"].shape[0]) - 1
    if int(pu_["event_ptr"].shape[0]) - 1 != E:
        raise ValueError("muon and pu must cover the same entries: %d and %d" % (E, int(pu_["event_ptr"].shape[0]) - 1))
    if E < 1:
        raise ValueError("no entries (the reference's pd.concat of no frames raises)")
    if E > MAX_ENTRIES:
        raise ValueError("more than %d entries" % MAX_ENTRIES)
    if int(entry_start) != entry_start:
        raise ValueError("entry_start must be an integer")
    for name, v in (("vp_pt", vp_pt), ("vp_eta", vp_eta)):
        if device != (torch.is_tensor(v) and v.is_cuda):
            raise ValueError("%s must be on the same side as the hit columns" % name)
        if v.dtype not in (np.float32, torch.float32) or len(v.shape) != 1:
            raise ValueError("%s must be a one-dimensional float32 array" % name)
    if int(vp_pt.shape[0]) != int(vp_eta.shape[0]):
        raise ValueError("vp_pt and vp_eta must have the same length")
    if device:
        from . import _lib
        dev = mu["vh_sim_z"].device
        for name, c in list(pu_.items()) + [("vp_pt", vp_pt), ("vp_eta", vp_eta)]:
            if c.device != dev:
                raise ValueError("%s is on %s, the muon columns on %s" % (name, c.device, dev))
        vp = (vp_pt.contiguous(), vp_eta.contiguous())
        if layout == "padded":
            return _lib.muon_graph_padded(mu, pu_, E, n_mu, n_pu, bool(muon_only), vp, int(entry_start))
        return _lib.muon_graph_flat(mu, pu_, E, n_mu, n_pu, bool(muon_only), vp, int(entry_start))
    res = build_muon_graphs_numpy(mu, pu_, _host(vp_pt), _host(vp_eta), int(entry_start), bool(muon_only))
    return pad(res, E) if layout == "padded" else res


def _source_rows(cols, lut):
    """Validated LUT layers of one source's rows ([n] int32, -99 for no layer)."""
    t, s, r = (cols[k] for k in ("vh_type", "vh_station", "vh_ring"))
    bad = (t < 0) | (t >= LUT_SIZE) | (s < 0) | (s >= LUT_SIZE) | (r < 0) | (r >= LUT_SIZE)
    if np.any(bad):
        raise ValueError("a type, station or ring outside [0, 5): the reference's LUT index")
    if not np.all(np.isfinite(cols["vh_sim_z"])):
        raise ValueError("a non-finite z")
    return lut[t, s, r]


def _dedup(rows, t, s, r):
    """Positions of the first row of every (type, station, ring) among `rows`, in row order."""
    seen, keep = set(), []
    for i in rows:
        k = (int(t[i]), int(s[i]), int(r[i]))
        if k not in seen:
            seen.add(k)
            keep.append(i)
    return keep


def build_muon_graphs_numpy(muon, pu, vp_pt, vp_eta, entry_start, muon_only):
    """The specification (validated host columns, as build_muon_graphs passes them): a MuonGraphs on the CPU."""
    lut = lut_array()
    src = (pu, muon)                                   # hit_source 0 = PU, 1 = muon
    lay = [_source_rows(c, lut) for c in src]
    E = muon["event_ptr"].shape[0] - 1
    kept = [[None] * E, [None] * E]                   # per source and entry: absolute rows after deduplication
    for e in range(E):
        b = [c["event_ptr"][e] for c in src]
        n = min(int(c["event_ptr"][e + 1]) - int(c["event_ptr"][e]) for c in src)
        sub = np.arange(n)
        ok = (lay[0][b[0] + sub] != -99) & (lay[1][b[1] + sub] != -99)          # :178-179
        m = muon
        truth = ok & (m["vh_sim_tp1"][b[1] + sub] == 0) & (m["vh_sim_tp2"][b[1] + sub] == 0)   # :192
        for k, sel in ((0, ok), (1, truth)):
            c = src[k]
            kept[k][e] = _dedup(b[k] + sub[sel], c["vh_type"], c["vh_station"], c["vh_ring"])
    has = [np.array([len(kept[k][e]) > 0 for e in range(E)], dtype=bool) for k in (0, 1)]
    ordinal = [np.cumsum(h) - h for h in has]
    n_mu = int(has[1].sum())
    use_pu = has[0] & (ordinal[0] < n_mu) & (not muon_only)
    Xs, srcs, dsts, ys = [], [], [], []
    entry, pt, eta, written, vp_missing, hsrc, hrow = [], [], [], [], [], [], []
    hit_ptr, seg_ptr = [0], [0]
    for e in range(E):
        parts = []
        if has[1][e]:
            parts.append(1)
        if use_pu[e]:
            parts.insert(0 if not (has[1][e] and ordinal[1][e] < ordinal[0][e]) else 1, 0)
        if not parts:
            continue
        hits = [(k, row) for k in parts for row in kept[k][e]]
        source = np.array([k for k, _ in hits], dtype=np.int8)
        X = np.zeros((len(hits), N_FEATURES), dtype=np.float32)
        signed = np.zeros(len(hits), dtype=np.float64)
        for j, (k, row) in enumerate(hits):
            c = src[k]
            signed[j] = np.float64(lay[k][row]) * np.float64(np.sign(c["vh_sim_z"][row]))     # :189-190
            X[j, :10] = [np.float32(np.float64(c[f][row])) for f in HIT_FEATURES]
        X[:, 10] = signed.astype(np.float32)
        r, phi, z = (X[:, HIT_FEATURES.index(f)] for f in ("vh_sim_r", "vh_sim_phi", "vh_sim_z"))
        pairs = layer_pairs(set_order(signed.tolist()))
        a_all, b_all = [], []
        for l1, l2 in pairs:
            a = np.flatnonzero(signed == l1)
            b = np.flatnonzero(signed == l2)
            i = np.repeat(a, b.size)                # the merge on "entry": left rows, then right rows, in frame order
            j = np.tile(b, a.size)
            dphi = wrap_dphi32(phi[j] - phi[i])
            dz = z[j] - z[i]
            dr = r[j] - r[i]
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                slope = dphi / dr
                z0 = z[i] - r[i] * dz / dr
            assert slope.dtype == z0.dtype == np.float32
            keep = (np.abs(slope) < _CUT32) & (np.abs(z0) < _CUT32)
            a_all.append(i[keep])
            b_all.append(j[keep])
        a = np.concatenate(a_all) if a_all else np.zeros(0, np.int64)
        b = np.concatenate(b_all) if b_all else np.zeros(0, np.int64)
        Xs.append(X)
        srcs.append(a + hit_ptr[-1])
        dsts.append(b + hit_ptr[-1])
        ys.append(((source[a] == 1) & (source[b] == 1)).astype(np.float32))
        hsrc.append(source)
        hrow.append(np.array([row for _, row in hits], dtype=np.int64))
        hit_ptr.append(hit_ptr[-1] + len(hits))
        seg_ptr.append(seg_ptr[-1] + a.size)
        entry.append(entry_start + e)
        written.append(len(pairs) > 0)
        miss = e >= vp_pt.shape[0]                                                 # :254, iloc[entry - start]
        vp_missing.append(miss)
        pt.append(np.float32(np.nan) if miss else vp_pt[e])
        eta.append(np.float32(np.nan) if miss else vp_eta[e])
    cat = (lambda v, dt, shape=(0,): np.concatenate(v).astype(dt) if v else np.zeros(shape, dt))
    batch = HitGraphBatch(cat(Xs, np.float32, (0, N_FEATURES)), cat(srcs, np.int32), cat(dsts, np.int32),
                          y=cat(ys, np.float32), hit_ptr=hit_ptr, seg_ptr=seg_ptr, _checked=True)
    G = len(entry)
    return MuonGraphs(batch, np.array(entry, np.int64), np.array(pt, np.float32), np.array(eta, np.float32),
                      np.array(written, bool), np.array(vp_missing, bool), cat(hsrc, np.int8), cat(hrow, np.int64),
                      present=np.ones(G, bool), n_hits=np.diff(hit_ptr).astype(np.int32),
                      n_segments=np.diff(seg_ptr).astype(np.int32), entry_start=entry_start)


def pad(res, n_entries):
    """The padded layout of a host MuonGraphs: slot e = entry entry_start + e (see MuonGraphs)."""
    H, S, G = MAX_GRAPH_HITS, MAX_GRAPH_SEGMENTS, n_entries
    b = res.batch
    X = np.zeros((G * H, N_FEATURES), np.float32)
    src, dst = np.full(G * S, -1, np.int32), np.full(G * S, -1, np.int32)
    y = np.zeros(G * S, np.float32)
    hs, hr = np.full(G * H, -1, np.int8), np.full(G * H, -1, np.int64)
    pt, eta = np.full(G, np.nan, np.float32), np.full(G, np.nan, np.float32)
    written, vpm, present = np.zeros(G, bool), np.zeros(G, bool), np.zeros(G, bool)
    nh, ns = np.zeros(G, np.int32), np.zeros(G, np.int32)
    Xf, sf, df, yf = (t.numpy() for t in (b.X, b.src, b.dst, b.y))
    for g in range(b.n_graphs):
        h0, h1, s0, s1 = (int(v) for v in (b.hit_ptr[g], b.hit_ptr[g + 1], b.seg_ptr[g], b.seg_ptr[g + 1]))
        e = int(res.entry[g]) - res.entry_start
        X[e * H:e * H + h1 - h0] = Xf[h0:h1]
        src[e * S:e * S + s1 - s0] = sf[s0:s1] - h0 + e * H
        dst[e * S:e * S + s1 - s0] = df[s0:s1] - h0 + e * H
        y[e * S:e * S + s1 - s0] = yf[s0:s1]
        hs[e * H:e * H + h1 - h0] = res.hit_source[h0:h1]
        hr[e * H:e * H + h1 - h0] = res.hit_row[h0:h1]
        pt[e], eta[e], written[e], vpm[e] = res.pt[g], res.eta[g], res.written[g], res.vp_missing[g]
        present[e], nh[e], ns[e] = True, h1 - h0, s1 - s0
    batch = HitGraphBatch(X, src, dst, y=y, hit_ptr=np.arange(G + 1) * H, seg_ptr=np.arange(G + 1) * S,
                          _checked=True)
    return MuonGraphs(batch, res.entry_start + np.arange(G, dtype=np.int64), pt, eta, written, vpm, hs, hr,
                      layout="padded", present=present, n_hits=nh, n_segments=ns, entry_start=res.entry_start)
