"""Loading of tests/golden/toy_graphs/*.npz (tools/gen_toy_graphs_golden.py: the reference notebooks' data cells, run)
for the host and GPU tests of the toy graph builders; each fixture is loaded once and never changed."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "toy_graphs")
SHAPES = ("l10_t5", "l10_t4", "l3_t2", "l2_t1", "edge")
NORMS = (None, "row", "kw")
_CACHE = {}


def load(name):
    if name not in _CACHE:
        with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
            d = {k: z[k] for k in z.files}
        for v in d.values():
            v.setflags(write=False)
        _CACHE[name] = d
    return _CACHE[name]


def dense(d, prefix="A"):
    """The dense float32 [E, N, N] matrix of a fixture's coordinate form."""
    a = np.zeros(tuple(int(v) for v in d["A_shape"]), dtype=np.float32)
    a[d[prefix + "_batch"], d[prefix + "_rows"], d[prefix + "_cols"]] = d[prefix + "_vals"]
    return a


def lists(a, W, transposed=False):
    """compress_adjacency's contract in numpy: (cnt [E, N], idx, val [E, N, W]) of a dense [E, N, N] matrix - entries
    != 0, ascending index, zero-padded; the column lists with `transposed`."""
    if transposed:
        a = a.transpose(0, 2, 1)
    nz = a != 0
    cnt = nz.sum(axis=-1).astype(np.int32)
    assert int(cnt.max(initial=0)) <= W
    order = np.argsort(~nz, axis=-1, kind="stable")[..., :W]                 # the non-zeros first, ascending index
    keep = np.arange(order.shape[-1]) < cnt[..., None]
    idx = np.where(keep, order, 0).astype(np.int32)
    val = np.where(keep, np.take_along_axis(a, order, axis=-1), np.float32(0)).astype(np.float32)
    return cnt, idx, val


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
