"""The cut study and the layer census on the host: the numpy specifications against the reference-made fixtures
(tests/golden/cut_study, tools/gen_cut_study_golden.py), the kept-count identity with the graph builder's own
reference-made fixtures, the API's contracts and refusals, and the C ABI's new entry points; no GPU."""
import glob
import json
import os
import re

import numpy as np
import pytest
import torch

from gnn_fpga_amd import SegmentCutStudy, _lib, count_layer_transitions, study_segment_cuts, synth
from test_graph_build_host import CASES as GB_CASES, load_case as load_gb_case

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = os.path.join(REPO, "tests", "golden", "cut_study")
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(CS, "*.npz")))
CENSUS_CASES = [c for c in CASES if "census" in np.load(os.path.join(CS, c + ".npz")).files]
NAMES = ("gnn_cut_study_workspace_bytes", "gnn_cut_study", "gnn_layer_census_workspace_bytes", "gnn_layer_census")
ADJACENT = np.stack([np.arange(9), np.arange(1, 10)], axis=1)
SLOPE_EDGES = [1e-4, 5e-4, 1e-3, 5e-3]
Z0_EDGES = [50.0, 200.0, 800.0]


def load_case(name):
    f = np.load(os.path.join(CS, name + ".npz"))
    cols = synth.HitColumns(f["r"], f["phi"], f["z"], f["layer"], f["particle_id"], f["event_ptr"])
    kw = dict(event_ptr=cols.event_ptr, phi_slope_edges=f["phi_slope_edges"], z0_edges=f["z0_edges"])
    return cols, f["layer_pairs"], kw, f["counts"], (f["census"] if "census" in f.files else None)


def study(cols, pairs, **kw):
    return study_segment_cuts(cols.r, cols.phi, cols.z, cols.layer, pairs, cols.particle_id, **kw)


def gb_edges(kw):
    """Edges that contain a graph_build fixture's cuts (as float32), among others."""
    psm, pso, z0m = (np.float32(kw[k]) for k in ("phi_slope_max", "phi_slope_outer_max", "z0_max"))
    se = np.unique(np.concatenate([np.array([1e-4, 3e-3, 0.05], np.float32), [psm, pso]]))
    ze = np.unique(np.concatenate([np.array([20.0, 1000.0], np.float32), [z0m]]))
    return se, ze


def gb_study_args(name):
    cols, pairs, kw, graphs = load_gb_case(name)
    se, ze = gb_edges(kw)
    skw = dict(event_ptr=cols.event_ptr, n_phi_sectors=kw["n_phi_sectors"], phi_slope_edges=se, z0_edges=ze)
    cuts = (kw["phi_slope_max"], kw["z0_max"], kw["phi_slope_outer_max"])
    return cols, pairs, skw, cuts, graphs


# ---- the reference-made fixtures -------------------------------------------------------------------------------------
def test_fixture_set():
    assert set(CASES) >= {"notebook", "dr_zero", "phi_wrap", "missing_layer", "two_events", "inf_edge"}
    assert len(CENSUS_CASES) >= 4
    assert sum(os.path.getsize(os.path.join(CS, c + ".npz")) for c in CASES) < 200e3
    with open(os.path.join(CS, "reference_time.json")) as fh:
        rec = json.load(fh)
    assert rec["hits"] == 10000 and rec["study_seconds"] > 0 and rec["census_seconds"] > 0


@pytest.mark.parametrize("name", CASES)
def test_spec_reproduces_reference_counts(name):
    cols, pairs, kw, counts, _ = load_case(name)
    s = study(cols, pairs, **kw)
    assert s.counts.dtype == torch.int64 and tuple(s.counts.shape) == counts.shape
    np.testing.assert_array_equal(s.counts.numpy(), counts)            # element for element
    assert s.phi_slope_edges.dtype == np.float32 and s.z0_edges.dtype == np.float32


def test_fixtures_cover_their_edge_cases():
    c = {n: load_case(n) for n in CASES}
    assert c["dr_zero"][3][:2, :, -1, -1].sum() > 0                   # dr = 0 pairs: the last bin of both axes
    assert c["dr_zero"][3][1, 1].sum() > 0                            # the (l, l) pair pairs a hit with itself: true
    assert np.isinf(c["inf_edge"][2]["phi_slope_edges"][-1]) and c["inf_edge"][3][:, :, -1, -1].sum() > 0
    assert c["inf_edge"][3][:, :, -1, :-1].sum() == 0                 # inf or NaN in one quantity is in both
    assert c["missing_layer"][3][3:5].sum() == 0 and c["missing_layer"][3][2].sum() > 0
    assert c["two_events"][0].event_ptr.shape[0] == 3
    np.testing.assert_array_equal(c["two_events"][3][0], c["two_events"][3][2])     # a repeated pair: its own row
    pi32 = np.float32(np.pi)
    assert np.any(c["phi_wrap"][0].phi == pi32) and np.any(c["phi_wrap"][0].phi == -pi32)


@pytest.mark.parametrize("name", CENSUS_CASES)
def test_census_reproduces_reference(name):
    cols, _, _, _, census = load_case(name)
    t = count_layer_transitions(cols.r, cols.layer, cols.particle_id, event_ptr=cols.event_ptr, n_layers=10)
    assert t.dtype == torch.int64
    np.testing.assert_array_equal(t.numpy(), census)


# ---- the kept-count identity with the graph builder's fixtures ----------------------------------------------------------
@pytest.mark.parametrize("name", GB_CASES)
def test_kept_equals_reference_segments(name):
    cols, pairs, skw, cuts, graphs = gb_study_args(name)
    s = study(cols, pairs, **skw)
    kept = s.kept(*cuts)
    assert tuple(kept.shape) == (len(pairs), 2) and kept.dtype == torch.int64
    n_seg = sum(g["y"].shape[0] for g in graphs)
    n_true = int(sum(g["y"].sum() for g in graphs))
    assert int(kept.sum()) == n_seg and int(kept[:, 1].sum()) == n_true
    if name == "default_2k":
        assert (n_seg, n_true) == (3315, 1552)
    if name == "all_pairs_inf":
        assert (n_seg, n_true) == (1431, 108) and np.isinf(s.phi_slope_edges[-1])
    assert s.purity(*cuts) == n_true / n_seg
    assert s.efficiency(*cuts) == n_true / int(s.counts[:, 1].sum())


# ---- API contracts ----------------------------------------------------------------------------------------------------
def n_pairs_expected(cols, pairs, S=1):
    edges = np.linspace(-np.pi, np.pi, S + 1)
    total = 0
    for e in range(cols.event_ptr.shape[0] - 1):
        sl = slice(cols.event_ptr[e], cols.event_ptr[e + 1])
        ph, lay = cols.phi[sl].astype(np.float64), cols.layer[sl]
        for s in range(S):
            m = (ph > edges[s]) & (ph < edges[s + 1])
            total += sum(int((lay[m] == a).sum()) * int((lay[m] == b).sum()) for a, b in pairs)
    return total


def test_counts_sum_marginals_and_kept():
    cols = synth.barrel_event(60, 30, n_events=2, seed=41)
    s = study(cols, ADJACENT, event_ptr=cols.event_ptr, n_phi_sectors=4, phi_slope_edges=SLOPE_EDGES,
              z0_edges=Z0_EDGES)
    assert tuple(s.counts.shape) == (9, 2, 5, 4)
    assert int(s.counts.sum()) == n_pairs_expected(cols, ADJACENT, 4)
    ms, mz = s.marginals()
    assert tuple(ms.shape) == (9, 2, 5) and tuple(mz.shape) == (9, 2, 4)
    assert torch.equal(ms.sum(-1), mz.sum(-1)) and torch.equal(ms.sum(-1), s.counts.sum((2, 3)))
    # kept: bins 0 .. k by 0 .. kz with edges[k] == cut; inner pairs (l1 < 5) take phi_slope_max
    k = s.kept(1e-3, 200.0, 5e-4)
    want = torch.stack([s.counts[p, :, :(3 if p < 5 else 2), :2].sum((1, 2)) for p in range(9)])
    assert torch.equal(k, want)
    assert torch.equal(s.kept(1e-3, 200.0), s.kept(1e-3, 200.0, 1e-3))
    np.testing.assert_array_equal(s.layer_pairs, ADJACENT)
    np.testing.assert_array_equal(s.phi_slope_edges, np.asarray(SLOPE_EDGES, np.float32))


def test_purity_and_efficiency_nan_without_pairs():
    cols = synth.barrel_event(5, 0, seed=42)
    s = study(cols, [[0, 1]], phi_slope_edges=[1e-12, 1.0], z0_edges=[1e-12, 1.0])
    assert int(s.kept(1e-12, 1e-12).sum()) == 0 and np.isnan(s.purity(1e-12, 1e-12))
    assert s.efficiency(1e-12, 1e-12) == 0.0
    none = study(cols, [], phi_slope_edges=[1.0], z0_edges=[1.0])
    assert tuple(none.counts.shape) == (0, 2, 2, 2) and np.isnan(none.efficiency(1.0, 1.0))


def test_additivity_over_events():
    cols = synth.barrel_event(50, 20, n_events=2, seed=43)
    kw = dict(n_phi_sectors=2, phi_slope_edges=SLOPE_EDGES, z0_edges=Z0_EDGES)
    both = study(cols, ADJACENT, event_ptr=cols.event_ptr, **kw)
    m = int(cols.event_ptr[1])
    a = study(synth.HitColumns(*(c[:m] for c in cols[:5]), None), ADJACENT, **kw)
    b = study(synth.HitColumns(*(c[m:] for c in cols[:5]), None), ADJACENT, **kw)
    total = a + b
    assert isinstance(total, SegmentCutStudy) and torch.equal(total.counts, both.counts)
    assert int(a.counts.sum()) > 0 and int(b.counts.sum()) > 0


def test_torch_cpu_inputs_take_the_specification():
    cols = synth.barrel_event(30, 10, seed=44)
    t = [torch.from_numpy(c) for c in cols[:5]]
    a = study_segment_cuts(t[0], t[1], t[2], t[3], ADJACENT, t[4], phi_slope_edges=torch.tensor(SLOPE_EDGES),
                           z0_edges=Z0_EDGES)
    b = study(cols, ADJACENT, phi_slope_edges=SLOPE_EDGES, z0_edges=Z0_EDGES)
    assert torch.equal(a.counts, b.counts) and not a.counts.is_cuda


def test_refusals():
    cols = synth.barrel_event(10, 2, seed=45)
    ok = dict(phi_slope_edges=SLOPE_EDGES, z0_edges=Z0_EDGES)
    with pytest.raises(ValueError, match="float64"):
        study_segment_cuts(cols.r.astype(np.float64), cols.phi, cols.z, cols.layer, [[0, 1]], cols.particle_id, **ok)
    with pytest.raises(ValueError, match="particle_id is required"):
        study_segment_cuts(cols.r, cols.phi, cols.z, cols.layer, [[0, 1]], None, **ok)
    with pytest.raises(ValueError, match="entries"):
        study_segment_cuts(cols.r, cols.phi, cols.z, cols.layer, [[0, 1]], cols.particle_id[:3], **ok)
    with pytest.raises(ValueError, match="strictly increasing"):
        study(cols, [[0, 1]], phi_slope_edges=[1e-3, 1e-4], z0_edges=Z0_EDGES)
    with pytest.raises(ValueError, match="strictly increasing"):       # equal once rounded to float32
        study(cols, [[0, 1]], phi_slope_edges=[1.0, 1.0 + 1e-12], z0_edges=Z0_EDGES)
    with pytest.raises(ValueError, match="NaN"):
        study(cols, [[0, 1]], phi_slope_edges=SLOPE_EDGES, z0_edges=[1.0, float("nan")])
    with pytest.raises(ValueError, match="one-dimensional"):
        study(cols, [[0, 1]], phi_slope_edges=[[1.0, 2.0]], z0_edges=Z0_EDGES)
    with pytest.raises(ValueError, match="one-dimensional"):
        study(cols, [[0, 1]], phi_slope_edges=[], z0_edges=Z0_EDGES)
    with pytest.raises(ValueError, match="at most 4096"):
        study(cols, [[0, 1]], phi_slope_edges=np.arange(1, 64), z0_edges=np.arange(1, 66))      # 64 x 66 cells
    assert tuple(study(cols, [[0, 1]], phi_slope_edges=np.arange(1, 64),
                       z0_edges=np.arange(1, 64)).counts.shape) == (1, 2, 64, 64)               # 4096 exactly
    with pytest.raises(ValueError, match="negative"):
        study(cols, [[0, -1]], **ok)
    with pytest.raises(ValueError, match="n_phi_sectors"):
        study(cols, [[0, 1]], n_phi_sectors=0, **ok)
    s = study(cols, [[0, 1]], **ok)
    with pytest.raises(ValueError, match="not one of the edges"):
        s.kept(2e-3, 200.0)
    with pytest.raises(ValueError, match="not one of the edges"):
        s.kept(1e-3, 200.0, 7e-4)
    with pytest.raises(ValueError, match="not one of the edges"):
        s.purity(1e-3, 100.0)
    with pytest.raises(ValueError, match="equal edges"):
        s + study(cols, [[0, 1]], phi_slope_edges=SLOPE_EDGES[:-1], z0_edges=Z0_EDGES)
    with pytest.raises(ValueError, match="equal edges"):
        s + study(cols, [[1, 2]], **ok)
    with pytest.raises(TypeError):
        s + 1


# ---- the layer census ---------------------------------------------------------------------------------------------------
def test_census_tie_in_r_takes_row_order():
    # one particle, three hits at r = 5: rows 1, 3, 4 in that order, between r = 1 (row 2) and r = 9 (row 0)
    r = np.array([9, 5, 1, 5, 5], np.float32)
    layer = np.array([4, 1, 0, 3, 2], np.int32)
    pid = np.full(5, 7, np.int64)
    t = count_layer_transitions(r, layer, pid).numpy()
    want = np.zeros((5, 5), np.int64)
    for a, b in ((0, 1), (1, 3), (3, 2), (2, 4)):
        want[a, b] = 1
    np.testing.assert_array_equal(t, want)
    # -0.0 and +0.0 are one radius
    t = count_layer_transitions(np.array([0.0, -0.0], np.float32), np.array([1, 0], np.int32), pid[:2]).numpy()
    assert t[1, 0] == 1 and t.sum() == 1


def test_census_events_skip_and_sizes():
    r = np.array([1, 2, 3, 1, 2, 1, 2], np.float32)
    layer = np.array([0, 1, 2, 0, 1, 0, 2], np.int32)
    pid = np.array([5, 5, 5, 0, 0, 5, 5], np.int64)
    one = count_layer_transitions(r, layer, pid).numpy()                 # particle 5: r 1, 1, 2, 2, 3 in row order
    assert one[0, 0] == 1 and one[0, 1] == 2 and one[1, 2] == 1 and one[2, 2] == 1 and one.sum() == 5
    two = count_layer_transitions(r, layer, pid, event_ptr=[0, 5, 7]).numpy()      # particle 5 is in both events
    want = np.zeros((3, 3), np.int64)
    want[0, 1], want[1, 2], want[0, 2] = 2, 1, 1
    np.testing.assert_array_equal(two, want)
    skip = count_layer_transitions(r, layer, pid, event_ptr=[0, 5, 7], skip_particle_id=0).numpy()
    want[0, 1] = 1
    np.testing.assert_array_equal(skip, want)
    assert tuple(count_layer_transitions(r, layer, pid, n_layers=6).shape) == (6, 6)
    assert int(count_layer_transitions(r[:0], layer[:0], pid[:0]).sum()) == 0
    cols = synth.barrel_event(40, 25, n_events=3, seed=46)
    t = count_layer_transitions(cols.r, cols.layer, cols.particle_id, event_ptr=cols.event_ptr)
    assert tuple(t.shape) == (10, 10) and int(t.sum()) == 3 * 40 * 9     # a track crosses ten layers; noise is alone


def test_census_refusals():
    r = np.array([1, np.nan, 3], np.float32)
    layer = np.array([0, 1, 2], np.int32)
    pid = np.zeros(3, np.int64)
    with pytest.raises(ValueError, match="NaN"):
        count_layer_transitions(r, layer, pid)
    r[1] = 2
    with pytest.raises(ValueError, match="float32"):
        count_layer_transitions(r.astype(np.float64), layer, pid)
    with pytest.raises(ValueError, match="entries"):
        count_layer_transitions(r, layer[:2], pid)
    with pytest.raises(ValueError, match="negative"):
        count_layer_transitions(r, np.array([0, -1, 2], np.int32), pid)
    with pytest.raises(ValueError, match="layer outside"):
        count_layer_transitions(r, layer, pid, n_layers=2)
    with pytest.raises(ValueError, match="event_ptr"):
        count_layer_transitions(r, layer, pid, event_ptr=[0, 2])
    with pytest.raises(ValueError, match="n_layers"):
        count_layer_transitions(r, layer, pid, n_layers=0)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    with open(os.path.join(REPO, "include", "gnn_hip.h")) as fh:
        hdr = fh.read()
    lib = _lib.load()
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, hdr) and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert "GNN_ABI_VERSION 7" in hdr and _lib.GNN_ABI_VERSION == 7 and lib.gnn_abi_version() == 7
    doc = hdr.split("all-pair histograms and a layer census")[1].split("gnn_layer_census(")[0]
    for cite in ("GraphConstructionDev.ipynb cell 20", "GraphConstructionDev_mu200.ipynb cell 18",
                 "gnn/graph.py:57-62", "cells 16-17 and 37-41"):
        assert cite in doc, cite


def test_cut_study_workspace_bytes_without_a_gpu():
    lib = _lib.load()
    pairs = np.array([[0, 1], [1, 2]], np.int32)
    ws = lambda n=1000, E=1, p=pairs, P=2, L=10, S=1, NS=4, NZ=3: \
        lib.gnn_cut_study_workspace_bytes(n, E, p.ctypes.data, P, L, S, NS, NZ)  # noqa: E731
    assert 0 < ws(n=0) < ws() < ws(n=100000)
    assert ws(NS=63, NZ=63) > 0                                            # 4096 cells
    assert ws(NS=63, NZ=64) == 0 and "4096" in lib.gnn_last_error().decode()
    assert ws(NS=0) == 0 and ws(NZ=0) == 0 and "edge" in lib.gnn_last_error().decode()
    assert ws(n=-1) == 0 and ws(E=0) == 0 and ws(S=0) == 0
    assert ws(p=np.array([[0, 10], [1, 2]], np.int32)) == 0
    assert ws(n=2 ** 25) == 0 and "2^25" in lib.gnn_last_error().decode()
