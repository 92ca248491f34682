"""graph_build on the MI355X: the HIP builder against the reference-made fixtures and the numpy specification,
run-to-run identity, hit_index, hits to scores, and the C ABI's argument checks."""
import ctypes

import numpy as np
import pytest
import torch

from gnn_fpga_amd import HitGraphBatch, synth
from gnn_fpga_amd.graph_build import build_graphs
from gnn_fpga_amd.synth import HitGraph
from test_graph_build_host import CASES, load_case, ref_endpoints

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def on_dev(cols):
    return synth.HitColumns(*(torch.from_numpy(np.ascontiguousarray(c)).to(DEV) for c in cols[:5]), cols.event_ptr)


def build_both(cols, pairs, **kw):
    d = on_dev(cols)
    host = build_graphs(cols.r, cols.phi, cols.z, cols.layer, pairs, **kw)
    kw_dev = dict(kw)
    if kw.get("particle_id") is not None:
        kw_dev["particle_id"] = d.particle_id
    dev = build_graphs(d.r, d.phi, d.z, d.layer, pairs, **kw_dev)
    torch.cuda.synchronize()
    return host, dev


def assert_same(host, dev):
    assert dev.X.is_cuda and dev.src.is_cuda
    np.testing.assert_array_equal(dev.hit_ptr, host.hit_ptr)
    np.testing.assert_array_equal(dev.seg_ptr, host.seg_ptr)
    assert dev.X.cpu().numpy().tobytes() == host.X.numpy().tobytes()
    assert torch.equal(dev.src.cpu(), host.src) and torch.equal(dev.dst.cpu(), host.dst)
    assert (dev.y is None) == (host.y is None)
    if host.y is not None:
        assert dev.y.cpu().numpy().tobytes() == host.y.numpy().tobytes()
    assert torch.equal(dev.hit_index.cpu(), host.hit_index)


@pytest.mark.parametrize("name", CASES)
def test_device_reproduces_reference(hip, name):
    cols, pairs, kw, graphs = load_case(name)
    kw["particle_id"] = torch.from_numpy(cols.particle_id).to(DEV)
    d = on_dev(cols)
    b = build_graphs(d.r, d.phi, d.z, d.layer, pairs, **kw)
    assert b.n_graphs == len(graphs)
    X, src, dst, y = (t.cpu().numpy() for t in (b.X, b.src, b.dst, b.y))
    for g, ref in enumerate(graphs):
        h0, h1, s0, s1 = int(b.hit_ptr[g]), int(b.hit_ptr[g + 1]), int(b.seg_ptr[g]), int(b.seg_ptr[g + 1])
        assert X[h0:h1].tobytes() == ref["X"].tobytes(), g
        rs, rd = ref_endpoints(ref)
        np.testing.assert_array_equal(src[s0:s1] - h0, rs)
        np.testing.assert_array_equal(dst[s0:s1] - h0, rd)
        assert y[s0:s1].tobytes() == ref["y"].tobytes()


# (n_tracks, n_noise, n_events, n_phi_sectors, seed): 1 .. 256 events, 1 and 8 sectors, layers beyond one 512-hit LDS
# tile (1 sector, 600 - 1500 tracks), tiny and empty events
SOAK = [(200, 50, 1, 8, 0), (200, 50, 1, 1, 1), (600, 0, 1, 1, 2), (1000, 100, 1, 1, 3), (1000, 0, 1, 8, 4),
        (1500, 200, 2, 1, 5), (50, 10, 16, 8, 6), (50, 10, 16, 1, 7), (20, 5, 64, 8, 8), (10, 3, 256, 8, 9),
        (5, 0, 256, 1, 10), (1, 0, 32, 8, 11), (0, 3, 8, 8, 12), (0, 1, 4, 1, 13), (300, 300, 3, 8, 14),
        (100, 0, 7, 3, 15), (120, 40, 5, 16, 16), (1000, 0, 4, 8, 17), (2, 0, 100, 8, 18), (700, 50, 1, 2, 19),
        (1000, 0, 256, 8, 20)]


@pytest.mark.parametrize("case", SOAK, ids=["t%d_n%d_e%d_s%d" % c[:4] for c in SOAK])
def test_device_equals_spec(hip, case):
    n_tracks, n_noise, n_events, S, seed = case
    cols = synth.barrel_event(n_tracks, n_noise, n_events=n_events, seed=seed)
    l = np.arange(10)
    pairs = np.stack([l[:-1], l[1:]], axis=1)
    host, dev = build_both(cols, pairs, particle_id=cols.particle_id, event_ptr=cols.event_ptr, n_phi_sectors=S)
    assert_same(host, dev)
    if n_tracks <= 1:
        assert np.any(np.diff(host.seg_ptr) == 0)                # graphs without segments


def test_device_equals_spec_other_pairs_and_cuts(hip):
    cols = synth.barrel_event(400, 100, n_events=3, seed=21)
    inf = float("inf")
    for pairs, kw in (([[0, 1], [2, 4], [0, 1], [7, 5]], dict(phi_slope_max=0.002, phi_slope_outer_max=0.0005)),
                      ([[3, 3], [9, 0]], dict(z0_max=50.0)),
                      ([[0, 1], [1, 2]], dict(phi_slope_max=inf, z0_max=inf)),
                      ([], {})):
        host, dev = build_both(cols, pairs, event_ptr=cols.event_ptr, n_phi_sectors=4, **kw)
        assert_same(host, dev)
    # no particle ids: no y
    host, dev = build_both(cols, [[0, 1]], event_ptr=cols.event_ptr)
    assert dev.y is None
    assert_same(host, dev)


def test_two_builds_identical_and_hit_index(hip):
    cols = synth.barrel_event(1000, 200, n_events=4, seed=22)
    d = on_dev(cols)
    l = np.arange(10)
    pairs = np.stack([l[:-1], l[1:]], axis=1)
    a, b = (build_graphs(d.r, d.phi, d.z, d.layer, pairs, particle_id=d.particle_id, event_ptr=cols.event_ptr,
                         n_phi_sectors=8) for _ in range(2))
    for k in ("X", "src", "dst", "y", "hit_index"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    hi = a.hit_index
    assert torch.equal(a.X[:, 0], (d.r[hi].double() / 1000.0).float())
    assert torch.equal(a.X[:, 2], (d.z[hi].double() / 1000.0).float())
    assert int(torch.unique(hi).numel()) == hi.numel()


def test_errors_raise(hip):
    cols = synth.barrel_event(20, 5, seed=23)
    d = on_dev(cols)
    bad = d.layer.clone()
    bad[4] = -2
    with pytest.raises(ValueError, match="negative"):
        build_graphs(d.r, d.phi, d.z, bad, [[0, 1]])
    with pytest.raises(ValueError, match="float64"):
        build_graphs(d.r.double(), d.phi, d.z, d.layer, [[0, 1]])


@pytest.mark.parametrize("use_plan", [True, "auto"])
def test_hits_to_scores(hip, use_plan):
    from gnn_fpga_amd.model import SegmentClassifier
    cols, pairs, kw, graphs = load_case("default_2k")
    kw["particle_id"] = torch.from_numpy(cols.particle_id).to(DEV)
    d = on_dev(cols)
    torch.manual_seed(0)
    model = SegmentClassifier(input_dim=3, hidden_dim=8, n_iters=4).to(DEV).eval()
    model.use_plan = use_plan
    built = build_graphs(d.r, d.phi, d.z, d.layer, pairs, **kw)
    refs = []
    for ref in graphs:
        rs, rd = ref_endpoints(ref)
        refs.append(HitGraph(ref["X"], rs.astype(np.int32), rd.astype(np.int32), ref["y"]))
    ref_batch = HitGraphBatch.from_graphs(refs).to(DEV)
    with torch.no_grad():
        got = model(built)
        want = model(ref_batch)
    assert got.shape == want.shape == (sum(g["y"].shape[0] for g in graphs),)
    assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()


def test_abi_bad_arguments(hip):
    lib = hip.load()
    r = torch.zeros(16, dtype=torch.float32, device=DEV)
    lay = torch.zeros(16, dtype=torch.int32, device=DEV)
    ep = torch.tensor([0, 16], dtype=torch.int64, device=DEV)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    out = torch.zeros(16, dtype=torch.int64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    good = np.array([[0, 1]], np.int32)
    badp = np.array([[0, 10]], np.int32)
    negp = np.array([[-1, 1]], np.int32)

    def sizes(n=16, n_events=1, pairs=good, n_pairs=1, n_layers=10, S=1, rp=r.data_ptr(), sp=out.data_ptr()):
        return lib.gnn_graph_build_sizes(rp, r.data_ptr(), r.data_ptr(), lay.data_ptr(), n, ep.data_ptr(), n_events,
                                         pairs.ctypes.data, n_pairs, n_layers, S, 0.001, 0.001, 200.0, ws.data_ptr(),
                                         ws.numel(), sp, out[8:].data_ptr(), out[10:].data_ptr(), st)

    assert sizes() == 0
    torch.cuda.synchronize()
    assert sizes(n=-1) == hip.GNN_ERR_BADARG
    assert sizes(n_events=0) == hip.GNN_ERR_BADARG
    assert sizes(S=0) == hip.GNN_ERR_BADARG
    assert sizes(pairs=badp) == hip.GNN_ERR_BADARG
    assert sizes(pairs=negp) == hip.GNN_ERR_BADARG
    assert sizes(n_pairs=-1) == hip.GNN_ERR_BADARG
    assert sizes(rp=None) == hip.GNN_ERR_BADARG
    assert sizes(sp=None) == hip.GNN_ERR_BADARG
    assert lib.gnn_graph_build_workspace_bytes(16, 1, badp.ctypes.data, 1, 10, 1) == 0
    assert lib.gnn_graph_build_workspace_bytes(16, 1, good.ctypes.data, 1, 10, 0) == 0
    sz = hip.GnnGraphBuildSizes()
    fill = lambda s_, S=1, pairs=good: lib.gnn_graph_build_fill(  # noqa: E731
        None, 16, 1, pairs.ctypes.data, 1, 10, S, 0.001, 0.001, 200.0, 1000.0, 1.0, 1000.0, s_, ws.data_ptr(),
        ws.numel(), out.data_ptr(), out.data_ptr(), out.data_ptr(), None, out.data_ptr(), st)
    assert fill(None) == hip.GNN_ERR_BADARG
    sz.status = 1
    sz.n_graphs = 1
    assert fill(ctypes.byref(sz)) == hip.GNN_ERR_BADARG              # flagged sizes are refused
    sz.status = 0
    assert fill(ctypes.byref(sz), S=0) == hip.GNN_ERR_BADARG
    assert fill(ctypes.byref(sz), pairs=badp) == hip.GNN_ERR_BADARG
    torch.cuda.synchronize()
