"""Helpers of the full-event graph tests: the fixtures of tests/golden/event_graphs (written by
tools/gen_event_graphs_golden.py from the reference's notebook cells) and the comparison against them."""
import glob
import os

import numpy as np

from gnn_fpga_amd import build_event_graphs

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "event_graphs")
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, "*.npz")))
COLS = ("r", "phi", "z", "volid", "layid", "barcode")


def load(case):
    return dict(np.load(os.path.join(GOLD, case + ".npz")))


def build(f, cols=None, **kw):
    """build_event_graphs with the fixture's cuts and bounds on its columns (or `cols` in their place)."""
    args = dict(dphi_max=float(f["dphi_max"]), dz_max=float(f["dz_max"]))
    if f["bounds"].size:
        args.update(zip(("n_nodes_min", "n_nodes_max", "n_edges_max"), (int(v) for v in f["bounds"])))
    args.update(kw)
    cols = [f[k] for k in COLS] if cols is None else cols
    return build_event_graphs(*cols, f["event_ptr"], **args)


def assert_equals_reference(g, f):
    """Every array of the result against the fixture: no case and no element left out."""
    b = g.batch
    hp, sp = f["ref_hit_ptr"], f["ref_seg_ptr"]
    assert np.array_equal(g.event_index.cpu().numpy(), f["ref_event_index"])
    assert np.array_equal(b.hit_ptr, hp) and np.array_equal(b.seg_ptr, sp)          # per-event sizes
    assert len(g) == len(hp) - 1
    X = b.X.cpu().numpy()
    assert X.dtype == np.float32 and X.shape == f["ref_X"].shape
    assert np.array_equal(X.view(np.uint32), f["ref_X"].view(np.uint32))
    off = np.repeat(hp[:-1], np.diff(sp))                                            # the fixture's ids are local
    assert np.array_equal(b.src.cpu().numpy(), f["ref_src"] + off)
    assert np.array_equal(b.dst.cpu().numpy(), f["ref_dst"] + off)
    y = b.y.cpu().numpy()
    assert y.dtype == np.float32 and np.array_equal(y, f["ref_y"].astype(np.float32))
