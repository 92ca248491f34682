"""GPU checks of the toy graph builders (csrc/toy_graphs.hip, gnn_fpga_amd/toy_graphs.py) against the reference
notebooks' own cells (tests/golden/toy_graphs, tools/gen_toy_graphs_golden.py) and the numpy specification in synth.py.

Hits: every array bit for bit - X, y0, the counts, indices and values of the row and of the column lists, for all three
norms; the edge fixture's hit pairs decide within rounding of a border, which a contracted FMA would decide otherwise.

Segments: X, y and the slope bit for bit.  A kernel value is exp of an argument that IS bit-equal, through two exp
implementations: where the reference is a normal number the distance is at most SEG_ULP_BOUND ulps; where it is
sub-normal or zero the absolute error is at most FLT_MIN and the entry may be listed or not.  Every figure is printed
before it is asserted (run with -s)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import toy_graphs_fixtures as fx
from gnn_fpga_amd import _lib, synth, toy_graphs
from gnn_fpga_amd.gcn import GCNBinaryClassifier, GCRNBinaryClassifier, compress_adjacency

pytestmark = pytest.mark.gpu
FLT_MIN = np.finfo(np.float32).tiny
# Measured once on an MI355X against all five segment fixtures (profiles/toy_graphs_probe.txt): the largest distance
# between the kernel's expf and numpy's float32 exp where numpy's value is a normal number is SEG_ULP_MEASURED ulps.
# The bound adds 2 ulps of margin for a different but equally good expf; numpy's own float32 exp sits up to 2 ulps from
# the rounded fp64 value on these inputs.
SEG_ULP_MEASURED = 2
SEG_ULP_BOUND = SEG_ULP_MEASURED + 2
SUBNORMAL_SHARE_MAX = 0.05                   # of the structural entries; the reference measures 0.027
SHARE_MIN_ENTRIES = 5000                     # (a handful of events is too small a sample for a share)
EVENT_COUNTS = (0, 1, 3, 65, 257)            # cross every events-per-workgroup boundary (1, 6, 32, 42, 128, 256)
# (n_layers, n_tracks): events per workgroup 1 / 6 (segments / hits), 32 / 42, 256 / 128
SYNTH_SHAPES = ((10, 5), (3, 2), (2, 1))
DET_R = {10: synth.TOY_DET_R, 3: (0.0, 1.0, 3.0), 2: (0.0, 2.0)}


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                              # (a copy: the fixtures are read-only)


def host_lists(adj):
    return {k: getattr(adj, k).cpu().numpy() for k in ("row_cnt", "row_idx", "row_val", "col_cnt", "col_idx", "col_val")}


def expected_width(kind, L, T, norm=None):
    nodes = T * T * (L - 1) if kind == "seg" else L * T
    return min(2 * T + (1 if norm == "kw" else 0), nodes)


def synth_hits(E, L, T, seed):
    """Sorted hits of E seeded events: (hit_x float32 [E, L T], hit_y int64)."""
    tracks = synth.toy_tracks(E, T, seed=seed, det_r=DET_R[L]).transpose(0, 2, 1)
    order = np.argsort(tracks, axis=-1, kind="stable")
    return np.take_along_axis(tracks, order, axis=-1).reshape(E, L * T), order.reshape(E, L * T)


# ---- hits: bit for bit ---------------------------------------------------------------------------------------------------
def check_hits(got, X, A, y0, n_iso, W):
    assert fx.same_bits(got.X.cpu().numpy(), X) and fx.same_bits(got.y0.cpu().numpy(), y0)
    assert got.adj.shape == A.shape and got.adj.width == W
    g = host_lists(got.adj)
    for side, transposed in (("row", False), ("col", True)):
        cnt, idx, val = fx.lists(A, W, transposed)
        assert np.array_equal(g[side + "_cnt"], cnt), side
        assert np.array_equal(g[side + "_idx"], idx), side
        assert fx.same_bits(g[side + "_val"], val), side
    assert got.n_isolated.dtype == torch.int64 and got.n_isolated.is_cuda
    assert int(got.n_isolated.item()) == n_iso


@pytest.mark.parametrize("norm", fx.NORMS)
@pytest.mark.parametrize("shape", fx.SHAPES)
def test_hits_equal_the_notebook(hip, shape, norm):
    d = fx.load("hits_" + shape)
    L = d["det_r"].shape[0]
    T = d["hit_x"].shape[1] // L
    got = toy_graphs.build_toy_hit_graphs(dev(d["hit_x"]), dev(d["hit_y"]), det_r=d["det_r"],
                                          seed_size=int(d["seed_size"]), norm=norm)
    check_hits(got, d["X"], fx.dense(d, norm or "none"), d["y0"], d["iso_rows"].shape[0], expected_width("hits", L, T, norm))


@pytest.mark.parametrize("E", EVENT_COUNTS)
@pytest.mark.parametrize("L,T", SYNTH_SHAPES[:1] + ((10, 4),) + SYNTH_SHAPES[1:])
def test_hits_equal_the_specification_at_every_event_count(hip, L, T, E):
    x, y = synth_hits(E, L, T, seed=7 + E)
    x = x.copy()
    if E:
        x[0, 0] = 0.0                                                        # (an isolated hit)
    for norm, target, seed_size, xin in ((None, 0, 3, x), ("row", 1, 2, x.astype(np.float64)), ("kw", 0, 0, x)):
        X, A, y0 = synth.toy_hit_graphs_from_hits(xin, y, det_r=DET_R[L], seed_size=seed_size, norm=norm, target=target)
        binary = synth.toy_hit_graphs_from_hits(xin, y, det_r=DET_R[L], norm=None)[1]
        got = toy_graphs.build_toy_hit_graphs(dev(xin), dev(y.astype(np.int32)), det_r=DET_R[L], seed_size=seed_size,
                                              norm=norm, target=target)
        check_hits(got, X, A, y0, int((binary.sum(axis=1) == 0).sum()), expected_width("hits", L, T, norm))


# ---- segments --------------------------------------------------------------------------------------------------------------
def check_segments(got, X, A, y, structural, W, what):
    """`structural`: the bool [S, S] (or [E, S, S]) mask of the entries cell 12 sets.  Returns the largest ulp distance
    over the entries whose reference is a normal number."""
    assert fx.same_bits(got.X.cpu().numpy(), X) and fx.same_bits(got.y.cpu().numpy(), y)      # the slope is X[..., 4]
    assert got.adj.shape == A.shape and got.adj.width == W
    assert got.adj.col_idx is got.adj.row_idx and got.adj.col_val is got.adj.row_val and got.adj.col_cnt is got.adj.row_cnt
    D = got.adj.to_dense().cpu().numpy()
    structural = np.broadcast_to(structural, A.shape)
    assert not D[~structural].any()                                          # nothing listed outside the structure
    ref, val = A[structural], D[structural]
    normal = ref >= FLT_MIN
    ulps = np.abs(val[normal].view(np.int32).astype(np.int64) - ref[normal].view(np.int32).astype(np.int64))
    worst = int(ulps.max(initial=0))
    small = float(np.abs(val[~normal].astype(np.float64) - ref[~normal].astype(np.float64)).max(initial=0.0))
    share = float(((ref > 0) & (ref < FLT_MIN)).mean()) if ref.size else 0.0
    print("\n%s: %d structural entries, %d normal: worst %d ulps (bound %d); sub-normal or zero: worst absolute error "
          "%.3e (bound %.3e); sub-normal share %.4f" % (what, ref.size, int(normal.sum()), worst, SEG_ULP_BOUND, small,
                                                       FLT_MIN, share))
    assert worst <= SEG_ULP_BOUND
    assert small <= FLT_MIN
    if ref.size >= SHARE_MIN_ENTRIES:
        assert share <= SUBNORMAL_SHARE_MAX
    # where the reference is normal the entry IS listed, so the lists agree there in structure as well
    assert (val[normal] != 0).all()
    return worst


def structure(L, T):
    s = np.arange(T * T * (L - 1))
    l, a, b = s // (T * T), (s // T) % T, s % T
    touch = (l[:, None] + 1 == l[None, :]) & (b[:, None] == a[None, :])
    return touch | touch.T


@pytest.mark.parametrize("shape", fx.SHAPES)
def test_segments_against_the_notebook(hip, shape):
    d = fx.load("seg_" + shape)
    L = d["det_r"].shape[0]
    T = d["hit_x"].shape[1] // L
    got = toy_graphs.build_toy_segment_graphs(dev(d["hit_x"]), dev(d["hit_y"]), det_r=d["det_r"], sigma=float(d["sigma"]))
    mask = np.zeros(tuple(d["A_shape"]), bool)
    mask[d["A_batch"], d["A_rows"], d["A_cols"]] = True
    check_segments(got, d["X"], fx.dense(d), d["y"], mask, expected_width("seg", L, T), "seg_" + shape)


@pytest.mark.parametrize("E", EVENT_COUNTS)
@pytest.mark.parametrize("L,T", SYNTH_SHAPES)
def test_segments_against_the_specification_at_every_event_count(hip, L, T, E):
    x, y = synth_hits(E, L, T, seed=11 + E)
    X, A, ys = synth.toy_segment_graphs_from_hits(x, y, det_r=DET_R[L])
    got = toy_graphs.build_toy_segment_graphs(dev(x), dev(y), det_r=DET_R[L])
    check_segments(got, X, A, ys, structure(L, T), expected_width("seg", L, T), "synth (%d, %d) x %d" % (L, T, E))


# ---- the lists are compress_adjacency's, bit exact ---------------------------------------------------------------------
def built(kind, E=65, norm="row"):
    if kind == "seg":
        x, y = synth_hits(E, 10, 5, seed=3)
        g = toy_graphs.build_toy_segment_graphs(dev(x), dev(y))
        return g.X, g.y, g.adj
    x, y = synth_hits(E, 10, 4, seed=4)
    x = x.copy()
    x[0, 0] = 0.0
    g = toy_graphs.build_toy_hit_graphs(dev(x), dev(y), norm=norm)
    return g.X, g.y0, g.adj


@pytest.mark.parametrize("kind,norm", [("seg", None), ("hits", None), ("hits", "row"), ("hits", "kw")])
def test_lists_are_what_compress_adjacency_gives(hip, kind, norm):
    _, _, adj = built(kind, norm=norm)
    dense = adj.to_dense()
    assert torch.equal(adj.to_dense(transposed=True), dense)
    again = compress_adjacency(dense)
    assert again.width <= adj.width
    g, c = host_lists(adj), host_lists(again)
    W = again.width
    for side in ("row", "col"):
        assert np.array_equal(g[side + "_cnt"], c[side + "_cnt"])
        assert np.array_equal(g[side + "_idx"][..., :W], c[side + "_idx"]) and not g[side + "_idx"][..., W:].any()
        assert fx.same_bits(g[side + "_val"][..., :W], c[side + "_val"]) and not g[side + "_val"][..., W:].any()
        keep = np.arange(adj.width) < g[side + "_cnt"][..., None]
        assert not g[side + "_idx"][~keep].any() and not g[side + "_val"][~keep].any()       # zero-padded
        assert (g[side + "_val"][keep] != 0).all()


def step(model, x, a, y):
    model.train()
    model.zero_grad()
    out = model(x, a)
    nn.BCEWithLogitsLoss()(out, y).backward()
    return out.detach().clone(), [p.grad.detach().clone() for p in model.parameters()]


@pytest.mark.parametrize("kind", ["seg", "hits"])
def test_model_logits_and_gradients_are_bit_identical(hip, kind):
    X, y, adj = built(kind)
    torch.manual_seed(0)
    model = (GCNBinaryClassifier(5, [16] * 3) if kind == "seg" else GCRNBinaryClassifier(3, [8] * 4)).cuda()
    out, grads = step(model, X, adj, y)
    out2, grads2 = step(model, X, compress_adjacency(adj.to_dense()), y)
    assert torch.equal(out, out2) and float(out.abs().max()) > 0
    assert all(torch.equal(a, b) for a, b in zip(grads, grads2))
    # adj[j:j+32] is a view, and a model input
    s = adj[32:64]
    assert len(s) == 32 and s.row_idx.data_ptr() == adj.row_idx[32].data_ptr() and s.row_idx.is_contiguous()
    assert s.col_val.data_ptr() == adj.col_val[32].data_ptr()
    with torch.no_grad():
        model.eval()
        assert torch.equal(model(X[32:64], s), model(X, adj)[32:64])
        assert torch.equal(model(X[64:96], adj[64:96]), model(X, adj)[64:])


# ---- the sort --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["seg_" + s for s in fx.SHAPES] + ["hits_edge"])
def test_sort_toy_tracks_agrees_with_numpy(hip, name):
    d = fx.load(name)
    L = d["det_r"].shape[0]
    E, T = d["hit_x"].shape[0], d["hit_x"].shape[1] // L
    x, y = d["hit_x"].reshape(E, L, T), d["hit_y"].reshape(E, L, T)
    tracks = np.empty_like(x)
    np.put_along_axis(tracks, y, x, axis=-1)                                 # undo the notebook's sort
    assert np.array_equal(np.argsort(tracks, axis=-1, kind="stable"), y)     # (numpy's argsort, the ties included)
    hx, hy = toy_graphs.sort_toy_tracks(dev(tracks.transpose(0, 2, 1)))
    assert hy.dtype == torch.int64 and fx.same_bits(hx.cpu().numpy(), d["hit_x"])
    assert np.array_equal(hy.cpu().numpy(), d["hit_y"])


def test_sort_feeds_the_builders(hip):
    tracks = dev(synth.toy_tracks(3, 5, seed=1))
    hx, hy = toy_graphs.sort_toy_tracks(tracks)
    g = toy_graphs.build_toy_segment_graphs(hx, hy, check=False)
    X, _, y = synth.toy_segment_graphs_from_hits(hx.cpu().numpy(), hy.cpu().numpy())
    assert fx.same_bits(g.X.cpu().numpy(), X) and fx.same_bits(g.y.cpu().numpy(), y)
    h = toy_graphs.build_toy_hit_graphs(hx, hy, det_r=synth.TOY_DET_R, check=False)
    assert h.X.shape == (3, 50, 3) and h.adj.width == 10


# ---- validation past the device check --------------------------------------------------------------------------------------
def test_validation_of_device_tensors(hip):
    """dtype, shape, non-finite positions, the kernels' shape limits."""
    x32, y5 = torch.rand(2, 50, device="cuda"), torch.zeros(2, 50, dtype=torch.int64, device="cuda")
    with pytest.raises(TypeError, match="float32"):
        toy_graphs.build_toy_segment_graphs(x32.double(), y5)
    with pytest.raises(TypeError, match="float64 or torch.float32"):
        toy_graphs.build_toy_hit_graphs(x32.half(), y5, det_r=range(10))
    with pytest.raises(TypeError, match="integer"):
        toy_graphs.build_toy_segment_graphs(x32, y5.float())
    with pytest.raises(ValueError, match="n_layers = 10"):
        toy_graphs.build_toy_segment_graphs(x32[:, :45], y5[:, :45])
    with pytest.raises(ValueError, match="n_layers"):
        toy_graphs.build_toy_segment_graphs(x32, y5[:1])
    with pytest.raises(RuntimeError, match="requires grad"):
        toy_graphs.build_toy_segment_graphs(x32.clone().requires_grad_(), y5)
    bad = x32.clone()
    bad[1, 7] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        toy_graphs.build_toy_segment_graphs(bad, y5)
    bad[1, 7] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        toy_graphs.build_toy_hit_graphs(bad, y5, det_r=range(10))
    z = lambda n: torch.zeros(1, n, dtype=torch.int64, device="cuda")        # noqa: E731
    with pytest.raises(RuntimeError, match="1 to 16 tracks"):
        toy_graphs.build_toy_segment_graphs(torch.rand(1, 34, device="cuda"), z(34), det_r=(0, 1))
    with pytest.raises(RuntimeError, match="at most 4096"):
        toy_graphs.build_toy_hit_graphs(torch.rand(1, 4100, device="cuda"), z(4100), det_r=range(1025))
    with pytest.raises(_lib.GnnHipError):
        toy_graphs.build_toy_hit_graphs(x32, y5.cpu(), det_r=range(10))
