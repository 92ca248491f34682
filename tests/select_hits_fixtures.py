"""What the hit selection's host and GPU tests share: the fixtures of tests/golden/select_hits (the reference's
select_hits, run by tools/gen_select_hits_golden.py) and the comparison against them."""
import glob
import os

import numpy as np
import torch

from gnn_fpga_amd import HitGraphBatch, select_hits

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "select_hits")
CASES = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLD, "*.npz")))
TABLES = (("hits", ("hit_id", "x", "y", "z", "volume_id", "layer_id")), ("truth", ("hit_id", "particle_id")),
          ("particles", ("particle_id", "px", "py")))
COLUMNS = ("r", "phi", "z", "layer", "particle_id", "hit_id", "row")
_cache = {}


def load(case):
    if case not in _cache:
        with np.load(os.path.join(GOLD, case + ".npz")) as f:
            _cache[case] = {k: f[k] for k in f.files}
    return _cache[case]


def tables(f, device=None):
    """The three input tables of a fixture (fresh dicts; on `device` as tensors when given; event_ptr stays host)."""
    put = (lambda a: a) if device is None else (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device))
    out = []
    for name, cols in TABLES:
        tb = {k: put(f["%s_%s" % (name, k)]) for k in cols}
        tb["event_ptr"] = f["%s_event_ptr" % name]
        out.append(tb)
    return out


def to_device(ev, device):
    """synth.trackml_events' tables on `device`."""
    put = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(device)          # noqa: E731
    return [{k: (v if k == "event_ptr" else put(v)) for k, v in ev[name].items()} for name, _ in TABLES]


def select(f, device=None, phi=True, **kw):
    """select_hits on a fixture's tables with its pt_min and no_missing_hits, phi handed in unless phi=False."""
    p = None
    if phi:
        p = f["phi"] if device is None else torch.from_numpy(f["phi"]).to(device)
    kw.setdefault("pt_min", float(f["pt_min"]))
    kw.setdefault("no_missing_hits", bool(f["no_missing_hits"]))
    return select_hits(*tables(f, device), phi=p, **kw)


def host(sel, k):
    return getattr(sel, k).cpu().numpy()


def assert_equals_reference(sel, f, phi=True):
    """Every column of a selection against the reference's, bit for bit (phi only when it was handed in)."""
    assert np.array_equal(np.asarray(sel.event_ptr), f["ref_event_ptr"]) and len(sel) == f["ref_row"].shape[0]
    assert sel.layer.dtype == torch.int32 and sel.particle_id.dtype == sel.row.dtype == sel.hit_id.dtype == torch.int64
    for k in ("row", "hit_id", "layer", "particle_id"):
        assert np.array_equal(host(sel, k), f["ref_" + k]), k
    for k in ("r", "z") + (("phi",) if phi else ()):
        assert sel.__dict__[k].dtype == torch.float32
        assert np.array_equal(host(sel, k).view(np.uint32), f["ref_" + k].view(np.uint32)), k


def assert_same(a, b):
    """Two selections, bit for bit."""
    assert np.array_equal(np.asarray(a.event_ptr), np.asarray(b.event_ptr))
    for k in COLUMNS:
        u, v = host(a, k), host(b, k)
        assert u.dtype == v.dtype and u.shape == v.shape, k
        assert np.array_equal(u.view(np.uint32) if u.dtype == np.float32 else u,
                              v.view(np.uint32) if v.dtype == np.float32 else v), k


def chain_reference_batch(f):
    """The chain fixture's reference graphs as one HitGraphBatch (the layout of tests/golden/graph_build)."""
    G = int(f["n_graphs"])
    X = [f["g%d_X" % g] for g in range(G)]
    hit_ptr = np.cumsum([0] + [x.shape[0] for x in X]).astype(np.int64)
    src, dst, y, seg_ptr = [], [], [], [0]
    for g in range(G):
        n_seg = f["g%d_y" % g].shape[0]
        a, b = np.full(n_seg, -1, np.int64), np.full(n_seg, -1, np.int64)
        a[f["g%d_Ro_cols" % g]] = f["g%d_Ro_rows" % g]                 # Ro / Ri .nonzero(): one hit per segment
        b[f["g%d_Ri_cols" % g]] = f["g%d_Ri_rows" % g]
        assert a.min(initial=0) >= 0 and b.min(initial=0) >= 0
        src.append(a + hit_ptr[g])
        dst.append(b + hit_ptr[g])
        y.append(f["g%d_y" % g].astype(np.float32))
        seg_ptr.append(seg_ptr[-1] + n_seg)
    return HitGraphBatch(np.concatenate(X).astype(np.float32), np.concatenate(src).astype(np.int32),
                         np.concatenate(dst).astype(np.int32), y=np.concatenate(y), hit_ptr=hit_ptr,
                         seg_ptr=np.asarray(seg_ptr, np.int64))


def assert_graphs_equal(batch, ref):
    assert np.array_equal(np.asarray(batch.hit_ptr), np.asarray(ref.hit_ptr))
    assert np.array_equal(np.asarray(batch.seg_ptr), np.asarray(ref.seg_ptr))
    assert np.array_equal(batch.X.cpu().numpy().view(np.uint32), ref.X.cpu().numpy().view(np.uint32))
    for k in ("src", "dst", "y"):
        assert torch.equal(getattr(batch, k).cpu(), getattr(ref, k).cpu()), k
