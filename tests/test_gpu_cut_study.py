"""The cut study and the layer census on the MI355X: the HIP kernels against the numpy specifications (whole arrays),
the reference-made fixtures, the graph builder's own segment counts, run-to-run identity and the C ABI's argument
checks."""
import numpy as np
import pytest
import torch

from gnn_fpga_amd import count_layer_transitions, study_segment_cuts, synth
from gnn_fpga_amd.graph_build import build_graphs
from test_cut_study_host import (ADJACENT, CASES, CENSUS_CASES, SLOPE_EDGES, Z0_EDGES, GB_CASES, gb_study_args,
                                 load_case)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def on_dev(cols):
    return synth.HitColumns(*(torch.from_numpy(np.ascontiguousarray(c)).to(DEV) for c in cols[:5]), cols.event_ptr)


def study_both(cols, pairs, **kw):
    d = on_dev(cols)
    host = study_segment_cuts(cols.r, cols.phi, cols.z, cols.layer, pairs, cols.particle_id, **kw)
    dev = study_segment_cuts(d.r, d.phi, d.z, d.layer, pairs, d.particle_id, **kw)
    assert dev.counts.is_cuda and dev.counts.dtype == torch.int64 and dev.counts.shape == host.counts.shape
    return host, dev


def assert_same(host, dev):
    np.testing.assert_array_equal(dev.counts.cpu().numpy(), host.counts.numpy())


# ---- device equals the reference and the specification ------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_device_reproduces_reference_counts(hip, name):
    cols, pairs, kw, counts, _ = load_case(name)
    d = on_dev(cols)
    s = study_segment_cuts(d.r, d.phi, d.z, d.layer, pairs, d.particle_id, **kw)
    np.testing.assert_array_equal(s.counts.cpu().numpy(), counts)


@pytest.mark.parametrize("name", GB_CASES)
def test_device_on_graph_build_fixtures(hip, name):
    cols, pairs, skw, cuts, graphs = gb_study_args(name)
    host, dev = study_both(cols, pairs, **skw)
    assert_same(host, dev)
    kept = dev.kept(*cuts)
    assert kept.is_cuda
    assert int(kept.sum()) == sum(g["y"].shape[0] for g in graphs)
    assert int(kept[:, 1].sum()) == int(sum(g["y"].sum() for g in graphs))


def test_device_kept_equals_device_builder(hip):
    cols = synth.barrel_event(300, 100, n_events=3, seed=51)
    d = on_dev(cols)
    s = study_segment_cuts(d.r, d.phi, d.z, d.layer, ADJACENT, d.particle_id, event_ptr=cols.event_ptr,
                           n_phi_sectors=4, phi_slope_edges=[2e-4, 6e-4, 2e-3], z0_edges=[50.0, 150.0])
    for psm, pso, z0m in ((6e-4, 2e-3, 150.0), (2e-3, 2e-4, 50.0)):
        b = build_graphs(d.r, d.phi, d.z, d.layer, ADJACENT, particle_id=d.particle_id, event_ptr=cols.event_ptr,
                         n_phi_sectors=4, phi_slope_max=psm, phi_slope_outer_max=pso, z0_max=z0m)
        kept = s.kept(psm, z0m, pso)
        assert b.n_segments > 0
        assert int(kept.sum()) == b.n_segments and int(kept[:, 1].sum()) == int(b.y.sum())


# (n_tracks, n_noise, n_events, n_phi_sectors, seed): more than one 512-hit LDS tile and more than one 128-row task per
# pair; two large events; many tiny graphs; empty layers and graphs without pairs
SHAPES = [(600, 0, 1, 1, 2), (1500, 200, 2, 1, 5), (10, 3, 256, 8, 9), (0, 3, 8, 8, 12), (1, 0, 32, 8, 11)]


@pytest.mark.parametrize("case", SHAPES, ids=["t%d_n%d_e%d_s%d" % c[:4] for c in SHAPES])
def test_device_equals_spec(hip, case):
    n_tracks, n_noise, n_events, S, seed = case
    cols = synth.barrel_event(n_tracks, n_noise, n_events=n_events, seed=seed)
    pairs = ADJACENT if n_tracks < 1500 else ADJACENT[[0, 4, 8]]           # (the specification's time)
    host, dev = study_both(cols, pairs, event_ptr=cols.event_ptr, n_phi_sectors=S, phi_slope_edges=SLOPE_EDGES,
                           z0_edges=Z0_EDGES)
    assert_same(host, dev)
    if n_tracks >= 600:
        assert int(host.counts[:, :, -1, -1].sum()) > 0                                # the register-counted cell
        assert int(host.counts[:, :, :-1, :-1].sum()) > 0 and int(host.counts[:, :, -1, :-1].sum()) > 0


def hand_made_pair(n1, n2, seed):
    """One event, layers 0 and 1 with exactly n1 and n2 hits; a fifth of the l2 hits continue an l1 hit's track."""
    rng = np.random.default_rng(seed)
    n = n1 + n2
    layer = np.concatenate([np.zeros(n1, np.int32), np.ones(n2, np.int32)])
    r = np.where(layer == 0, 32.0, 72.0) + rng.normal(0, 0.1, n)
    phi = rng.uniform(-3.1, 3.1, n)
    z = rng.uniform(-300, 300, n)
    pid = np.arange(1, n + 1, dtype=np.int64)
    m = min(n1, n2 // 5)
    pid[n1:n1 + m] = pid[:m]
    phi[n1:n1 + m] = phi[:m] + rng.uniform(-3e-4, 3e-4, m) * 40.0
    z[n1:n1 + m] = z[:m] * (72.0 / 32.0) + rng.normal(0, 0.5, m)
    order = rng.permutation(n)
    return synth.HitColumns(r[order].astype(np.float32), phi[order].astype(np.float32), z[order].astype(np.float32),
                            layer[order], pid[order], np.array([0, n], np.int64))


@pytest.mark.parametrize("n1,n2", [(128, 512), (129, 513), (128, 513), (129, 512)])
def test_tile_and_task_boundaries(hip, n1, n2):
    cols = hand_made_pair(n1, n2, seed=n1 + n2)
    host, dev = study_both(cols, [[0, 1], [1, 0]], phi_slope_edges=SLOPE_EDGES, z0_edges=Z0_EDGES)
    assert_same(host, dev)
    assert int(host.counts[0].sum()) == n1 * n2 == int(host.counts[1].sum())
    assert int(host.counts[0, 1].sum()) == min(n1, n2 // 5) and int(host.counts[0, 1, :-1, :-1].sum()) > 0


def test_one_edge_per_axis_the_cell_cap_and_repeated_pairs(hip):
    cols = synth.barrel_event(200, 50, seed=52)
    host, dev = study_both(cols, [[0, 1]], phi_slope_edges=[1e-3], z0_edges=[200.0])
    assert tuple(dev.counts.shape) == (1, 2, 2, 2)
    assert_same(host, dev)
    # 64 x 64 = 4096 cells exactly: log-spaced edges put pairs all over the table
    se, ze = np.geomspace(1e-6, 0.05, 63), np.geomspace(0.1, 3000.0, 63)
    host, dev = study_both(cols, ADJACENT[:3], phi_slope_edges=se, z0_edges=ze)
    assert_same(host, dev)
    assert int((host.counts > 0).sum()) > 1000
    # 2047 + 1 edges: the most the cap allows on one axis
    host, dev = study_both(cols, [[4, 5]], phi_slope_edges=np.geomspace(1e-7, 0.1, 2047), z0_edges=[100.0])
    assert_same(host, dev)
    pairs = [[0, 1], [2, 4], [0, 1], [7, 5], [0, 1]]
    host, dev = study_both(cols, pairs, n_phi_sectors=2, phi_slope_edges=SLOPE_EDGES, z0_edges=Z0_EDGES)
    assert_same(host, dev)
    assert torch.equal(dev.counts[0], dev.counts[2]) and torch.equal(dev.counts[0], dev.counts[4])
    with pytest.raises(ValueError, match="at most 4096"):
        d = on_dev(cols)
        study_segment_cuts(d.r, d.phi, d.z, d.layer, [[0, 1]], d.particle_id, phi_slope_edges=np.arange(1, 65),
                           z0_edges=np.arange(1, 65))


def test_two_runs_identical_and_sum_of_chunks(hip):
    cols = synth.barrel_event(500, 100, n_events=4, seed=53)
    d = on_dev(cols)
    kw = dict(n_phi_sectors=2, phi_slope_edges=SLOPE_EDGES, z0_edges=Z0_EDGES)
    a, b = (study_segment_cuts(d.r, d.phi, d.z, d.layer, ADJACENT, d.particle_id, event_ptr=cols.event_ptr, **kw)
            for _ in range(2))
    assert a.counts.cpu().numpy().tobytes() == b.counts.cpu().numpy().tobytes()
    m, ep = int(cols.event_ptr[2]), cols.event_ptr
    first = study_segment_cuts(d.r[:m], d.phi[:m], d.z[:m], d.layer[:m], ADJACENT, d.particle_id[:m],
                               event_ptr=ep[:3], **kw)
    second = study_segment_cuts(d.r[m:], d.phi[m:], d.z[m:], d.layer[m:], ADJACENT, d.particle_id[m:],
                                event_ptr=ep[2:] - m, **kw)
    assert torch.equal((first + second).counts, a.counts)


def test_device_errors_raise(hip):
    cols = synth.barrel_event(20, 5, seed=54)
    d = on_dev(cols)
    kw = dict(phi_slope_edges=SLOPE_EDGES, z0_edges=Z0_EDGES)
    bad = d.layer.clone()
    bad[4] = -2
    with pytest.raises(ValueError, match="negative"):
        study_segment_cuts(d.r, d.phi, d.z, bad, [[0, 1]], d.particle_id, **kw)
    with pytest.raises(ValueError, match="float64"):
        study_segment_cuts(d.r.double(), d.phi, d.z, d.layer, [[0, 1]], d.particle_id, **kw)
    with pytest.raises(ValueError, match="tensor on"):
        study_segment_cuts(d.r, d.phi, d.z, d.layer, [[0, 1]], cols.particle_id, **kw)
    nan = d.r.clone()
    nan[3] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        count_layer_transitions(nan, d.layer, d.particle_id)
    with pytest.raises(ValueError, match="layer outside"):
        count_layer_transitions(d.r, d.layer, d.particle_id, n_layers=4)
    # NaN r in the study is no error: such a pair sits in the last bin of both axes, as the builder never keeps it
    host = study_segment_cuts(*(c.cpu().numpy() for c in (nan, d.phi, d.z, d.layer)), ADJACENT, cols.particle_id, **kw)
    dev = study_segment_cuts(nan, d.phi, d.z, d.layer, ADJACENT, d.particle_id, **kw)
    assert_same(host, dev)


def test_abi_bad_arguments(hip):
    lib = hip.load()
    r = torch.zeros(16, dtype=torch.float32, device=DEV)
    lay = torch.zeros(16, dtype=torch.int32, device=DEV)
    pid = torch.zeros(16, dtype=torch.int64, device=DEV)
    ep = torch.tensor([0, 16], dtype=torch.int64, device=DEV)
    edges = torch.arange(1, 65, dtype=torch.float32, device=DEV)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    out = torch.zeros(2 * 65 * 65 + 1, dtype=torch.int64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    good = np.array([[0, 1]], np.int32)
    badp = np.array([[0, 10]], np.int32)

    def study(n=16, n_events=1, pairs=good, n_pairs=1, n_layers=10, S=1, NS=4, NZ=3, rp=r.data_ptr(),
              pp=pid.data_ptr(), ep_=ep.data_ptr(), se=edges.data_ptr(), cp=out.data_ptr(), sp=out[-1:].data_ptr(),
              wb=ws.numel()):
        return lib.gnn_cut_study(rp, r.data_ptr(), r.data_ptr(), lay.data_ptr(), pp, n, ep_, n_events,
                                 pairs.ctypes.data, n_pairs, n_layers, S, se, NS, edges.data_ptr(), NZ, ws.data_ptr(),
                                 wb, cp, sp, st)

    assert study() == 0
    torch.cuda.synchronize()
    assert int(out[-1]) == 0 and int(out[:2 * 5 * 4].sum()) == 0          # 16 hits on layer 0: no (0, 1) pair
    assert study(NS=63, NZ=63) == 0
    assert study(NS=63, NZ=64) == hip.GNN_ERR_UNSUPPORTED and b"4096" in lib.gnn_last_error()
    assert study(NS=0) == hip.GNN_ERR_BADARG and study(NZ=0) == hip.GNN_ERR_BADARG
    assert study(n=-1) == hip.GNN_ERR_BADARG and study(n_events=0) == hip.GNN_ERR_BADARG
    assert study(S=0) == hip.GNN_ERR_BADARG and study(pairs=badp) == hip.GNN_ERR_BADARG
    assert study(n_pairs=-1) == hip.GNN_ERR_BADARG
    for missing in ("rp", "pp", "ep_", "se", "cp", "sp"):
        assert study(**{missing: None}) == hip.GNN_ERR_BADARG, missing
    assert study(wb=64) == hip.GNN_ERR_WORKSPACE
    assert study(n=2 ** 25) == hip.GNN_ERR_UNSUPPORTED

    def census(n=16, n_events=1, L=10, rp=r.data_ptr(), tp=out.data_ptr(), sp=out[-1:].data_ptr(), wb=ws.numel()):
        return lib.gnn_layer_census(rp, lay.data_ptr(), pid.data_ptr(), n, ep.data_ptr(), n_events, L, 0, 0,
                                    ws.data_ptr(), wb, tp, sp, st)

    assert census() == 0
    torch.cuda.synchronize()
    assert int(out[-1]) == 0 and int(out[0]) == 15 and int(out[:100].sum()) == 15      # one particle on one layer
    assert census(n=-1) == hip.GNN_ERR_BADARG and census(n_events=0) == hip.GNN_ERR_BADARG
    assert census(L=0) == hip.GNN_ERR_BADARG and census(L=4097) == hip.GNN_ERR_UNSUPPORTED
    assert census(rp=None) == hip.GNN_ERR_BADARG and census(tp=None) == hip.GNN_ERR_BADARG
    assert census(sp=None) == hip.GNN_ERR_BADARG
    assert census(wb=64) == hip.GNN_ERR_WORKSPACE
    assert lib.gnn_layer_census_workspace_bytes(-1, 1, 10) == 0
    assert 0 < lib.gnn_layer_census_workspace_bytes(0, 1, 10) < lib.gnn_layer_census_workspace_bytes(10000, 1, 10)
    torch.cuda.synchronize()


# ---- the layer census -------------------------------------------------------------------------------------------------
def census_both(cols, **kw):
    host = count_layer_transitions(cols.r, cols.layer, cols.particle_id, **kw)
    dev = count_layer_transitions(*(torch.from_numpy(np.ascontiguousarray(c)).to(DEV)
                                    for c in (cols.r, cols.layer, cols.particle_id)), **kw)
    assert dev.is_cuda and dev.dtype == torch.int64 and dev.shape == host.shape
    np.testing.assert_array_equal(dev.cpu().numpy(), host.numpy())
    return host


@pytest.mark.parametrize("name", CENSUS_CASES)
def test_census_device_reproduces_reference(hip, name):
    cols, _, _, _, census = load_case(name)
    host = census_both(cols, event_ptr=cols.event_ptr, n_layers=10)
    np.testing.assert_array_equal(host.numpy(), census)


def test_census_device_equals_spec(hip):
    cols = synth.barrel_event(300, 300, n_events=3, seed=14)
    # noise ids -1, -2, ... are in all three events (not to be joined); give some noise a common id to skip, give
    # two tracks ties in r, and let one track's id appear in two events
    pid = cols.particle_id.copy()
    pid[(pid < 0) & (pid % 3 == 0)] = 0
    r = cols.r.copy()
    for p in (5, 1_000_007):
        rows = np.flatnonzero(pid == p)
        r[rows[:4]] = r[rows[0]]
    pid[pid == 2_000_009] = 9
    cols = cols._replace(particle_id=pid, r=r)
    with_noise = census_both(cols, event_ptr=cols.event_ptr)
    skipped = census_both(cols, event_ptr=cols.event_ptr, skip_particle_id=0)
    assert int(with_noise.sum()) > int(skipped.sum()) > 3 * 300 * 9 - 1
    joined = census_both(cols)                                              # one event: ids join across the old events
    assert int(joined.sum()) > int(with_noise.sum())
    d = on_dev(cols)
    a, b = (count_layer_transitions(d.r, d.layer, d.particle_id, event_ptr=cols.event_ptr) for _ in range(2))
    assert torch.equal(a, b)


def test_census_many_layers_and_tiny_inputs(hip):
    rng = np.random.default_rng(55)
    n = 5000
    cols = synth.HitColumns(rng.uniform(1, 1000, n).astype(np.float32), None, None,
                            rng.integers(0, 70, n).astype(np.int32), rng.integers(0, 400, n).astype(np.int64),
                            np.array([0, 1200, 1200, n], np.int64))
    census_both(cols, event_ptr=cols.event_ptr)                             # 70 layers: the global-atomics kernel
    small = cols._replace(layer=(cols.layer % 64).astype(np.int32))
    census_both(small, event_ptr=cols.event_ptr, n_layers=64)               # the LDS table at its largest
    for k in (0, 1, 2):
        one = synth.HitColumns(cols.r[:k], None, None, small.layer[:k], np.zeros(k, np.int64), None)
        census_both(one, n_layers=3 if k == 0 else 64)
