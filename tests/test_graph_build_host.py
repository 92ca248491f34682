"""graph_build on the host: the numpy specification against the reference-made fixtures
(tests/golden/graph_build, tools/gen_graph_golden.py), batch layout, validation."""
import glob
import os

import numpy as np
import pytest
import torch

from gnn_fpga_amd import HitGraphBatch, synth
from gnn_fpga_amd.graph_build import build_graphs

GB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_build")
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GB, "*.npz")))


def load_case(name):
    f = np.load(os.path.join(GB, name + ".npz"))
    cols = synth.HitColumns(f["r"], f["phi"], f["z"], f["layer"], f["particle_id"], f["event_ptr"])
    psm, pso, z0m = (float(c) for c in f["cuts"])
    kw = dict(particle_id=cols.particle_id, event_ptr=cols.event_ptr, n_phi_sectors=int(f["n_phi_sectors"]),
              phi_slope_max=psm, phi_slope_outer_max=pso, z0_max=z0m)
    graphs = [{k: f["g%d_%s" % (g, k)] for k in ("X", "Ri_rows", "Ri_cols", "Ro_rows", "Ro_cols", "y")}
              for g in range(int(f["n_graphs"]))]
    return cols, f["layer_pairs"], kw, graphs


def ref_endpoints(g):
    """src / dst per segment id from the reference's Ri / Ro nonzero arrays."""
    e = g["y"].shape[0]
    src = np.full(e, -1, np.int64)
    dst = np.full(e, -1, np.int64)
    src[g["Ro_cols"]] = g["Ro_rows"]
    dst[g["Ri_cols"]] = g["Ri_rows"]
    return src, dst


def build(cols, pairs, **kw):
    return build_graphs(cols.r, cols.phi, cols.z, cols.layer, pairs, **kw)


def test_fixture_set_present_and_small():
    assert len(CASES) >= 7
    assert sum(os.path.getsize(os.path.join(GB, c + ".npz")) for c in CASES) < 1.5e6


@pytest.mark.parametrize("name", CASES)
def test_numpy_spec_reproduces_reference(name):
    cols, pairs, kw, graphs = load_case(name)
    b = build(cols, pairs, **kw)
    assert b.n_graphs == len(graphs)
    X, src, dst, y = b.X.numpy(), b.src.numpy(), b.dst.numpy(), b.y.numpy()
    for g, ref in enumerate(graphs):
        h0, h1 = int(b.hit_ptr[g]), int(b.hit_ptr[g + 1])
        s0, s1 = int(b.seg_ptr[g]), int(b.seg_ptr[g + 1])
        assert h1 - h0 == ref["X"].shape[0] and s1 - s0 == ref["y"].shape[0], g
        assert X[h0:h1].tobytes() == ref["X"].tobytes(), g            # bit for bit
        rs, rd = ref_endpoints(ref)
        np.testing.assert_array_equal(src[s0:s1] - h0, rs)
        np.testing.assert_array_equal(dst[s0:s1] - h0, rd)
        assert y[s0:s1].tobytes() == ref["y"].tobytes()


@pytest.mark.parametrize("name", CASES)
def test_batch_matches_from_sparse_arrays(name):
    cols, pairs, kw, graphs = load_case(name)
    b = build(cols, pairs, **kw)
    for g, ref in enumerate(graphs):
        rb = HitGraphBatch.from_sparse_arrays(ref["X"], ref["Ri_rows"], ref["Ri_cols"], ref["Ro_rows"],
                                              ref["Ro_cols"], ref["y"])
        h0, s0, s1 = int(b.hit_ptr[g]), int(b.seg_ptr[g]), int(b.seg_ptr[g + 1])
        assert torch.equal(b.X[h0:int(b.hit_ptr[g + 1])], rb.X)
        assert torch.equal(b.src[s0:s1] - h0, rb.src) and torch.equal(b.dst[s0:s1] - h0, rb.dst)
        assert torch.equal(b.y[s0:s1], rb.y)


def test_graph_order_hit_ptr_and_hit_index():
    cols = synth.barrel_event(40, 20, n_events=3, seed=5)
    S = 4
    b = build(cols, [[0, 1], [1, 2]], event_ptr=cols.event_ptr, n_phi_sectors=S, particle_id=cols.particle_id)
    assert b.n_graphs == 3 * S
    hi = b.hit_index.numpy()
    edges = np.linspace(-np.pi, np.pi, S + 1)
    for g in range(b.n_graphs):
        e, s = divmod(g, S)
        rows = hi[b.hit_ptr[g]:b.hit_ptr[g + 1]]
        assert np.all(np.diff(rows) > 0)                                   # frame order
        assert np.all((rows >= cols.event_ptr[e]) & (rows < cols.event_ptr[e + 1]))
        ph = cols.phi[rows].astype(np.float64)
        assert np.all((ph > edges[s]) & (ph < edges[s + 1]))
        seg = slice(b.seg_ptr[g], b.seg_ptr[g + 1])
        for a in (b.src.numpy()[seg], b.dst.numpy()[seg]):
            assert np.all((a >= b.hit_ptr[g]) & (a < b.hit_ptr[g + 1]))
    # every hit not on an edge is in exactly one graph
    assert hi.shape[0] == cols.r.shape[0] and np.array_equal(np.sort(hi), np.arange(cols.r.shape[0]))
    np.testing.assert_array_equal(b.X.numpy()[:, 0], (cols.r[hi].astype(np.float64) / 1000.0).astype(np.float32))
    assert np.all(b.y.numpy()[(cols.particle_id[hi[b.src.numpy()]] == cols.particle_id[hi[b.dst.numpy()]])] == 1)


def test_no_particle_id_no_y():
    cols = synth.barrel_event(30, 5, seed=1)
    b = build(cols, [[0, 1]])
    assert b.y is None and b.n_segments > 0


def test_empty_graphs():
    # a sector whose layers never pair up, and an event without hits: graphs with no segments (the reference
    # raises from pd.concat([]) here)
    cols = synth.barrel_event(20, 0, n_events=1, seed=2)
    keep = cols.layer == 0
    ep = np.array([0, int(keep.sum()), int(keep.sum())], np.int64)
    b = build_graphs(cols.r[keep], cols.phi[keep], cols.z[keep], cols.layer[keep], [[0, 1]], event_ptr=ep,
                     n_phi_sectors=2, particle_id=cols.particle_id[keep])
    assert b.n_graphs == 4 and b.n_segments == 0 and b.y.shape == (0,)
    assert b.hit_ptr[2] == keep.sum() and b.hit_ptr[-1] == keep.sum()
    np.testing.assert_array_equal(b.seg_ptr, np.zeros(5))


def test_infinite_thresholds_give_all_pairs():
    cols = synth.barrel_event(7, 3, seed=3)
    inf = float("inf")
    b = build(cols, [[0, 1], [3, 2]], phi_slope_max=inf, z0_max=inf)
    n = [np.sum(cols.layer == l) for l in range(4)]
    assert b.n_segments == n[0] * n[1] + n[3] * n[2]


def test_outer_cut_chosen_by_first_layer():
    cols = synth.barrel_event(200, 0, seed=4)
    wide = build(cols, [[5, 6]], phi_slope_max=1e-9, phi_slope_outer_max=0.01).n_segments
    narrow = build(cols, [[5, 6]], phi_slope_max=0.01, phi_slope_outer_max=1e-9).n_segments
    assert wide > 0 and narrow == 0
    assert build(cols, [[4, 5]], phi_slope_max=1e-9, phi_slope_outer_max=0.01).n_segments == 0


def test_validation_errors():
    cols = synth.barrel_event(10, 2, seed=0)
    with pytest.raises(ValueError, match="float64"):
        build_graphs(cols.r.astype(np.float64), cols.phi, cols.z, cols.layer, [[0, 1]])
    with pytest.raises(ValueError, match="entries"):
        build_graphs(cols.r, cols.phi[:-1], cols.z, cols.layer, [[0, 1]])
    with pytest.raises(ValueError, match="entries"):
        build_graphs(cols.r, cols.phi, cols.z, cols.layer, [[0, 1]], particle_id=cols.particle_id[:3])
    bad = cols.layer.copy()
    bad[3] = -1
    with pytest.raises(ValueError, match="negative"):
        build_graphs(cols.r, cols.phi, cols.z, bad, [[0, 1]])
    with pytest.raises(ValueError, match="event_ptr"):
        build_graphs(cols.r, cols.phi, cols.z, cols.layer, [[0, 1]], event_ptr=[0, 60, 40, cols.r.shape[0]])
    with pytest.raises(ValueError, match="event_ptr"):
        build_graphs(cols.r, cols.phi, cols.z, cols.layer, [[0, 1]], event_ptr=[0, 5])
    with pytest.raises(ValueError, match="n_phi_sectors"):
        build_graphs(cols.r, cols.phi, cols.z, cols.layer, [[0, 1]], n_phi_sectors=0)
    with pytest.raises(ValueError, match="negative"):
        build_graphs(cols.r, cols.phi, cols.z, cols.layer, [[0, -1]])


def test_barrel_event_columns():
    c = synth.barrel_event(100, 30, n_events=2, seed=9)
    assert c.r.dtype == c.phi.dtype == c.z.dtype == np.float32
    assert c.layer.dtype == np.int32 and c.particle_id.dtype == np.int64 and c.event_ptr.dtype == np.int64
    assert c.event_ptr.tolist() == [0, 1030, 2060]
    assert np.all((c.phi >= -np.pi) & (c.phi <= np.pi)) and set(np.unique(c.layer)) == set(range(10))
    again = synth.barrel_event(100, 30, n_events=2, seed=9)
    assert all(np.array_equal(a, b) for a, b in zip(c, again))
