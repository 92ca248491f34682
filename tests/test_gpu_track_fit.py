"""The track fit's kernel (csrc/track_fit.hip) against the specification (gnn-fpga_amd/tracks.py fit_tracks_numpy):
moments, params, n_hits and status equal bit for bit, NaN equal to NaN.  No tolerance anywhere: the kernel restates
the specification operation for operation in float64 without contraction, and fp64 + - * / and sqrt round on gfx950
as they do in numpy."""
import numpy as np
import pytest
import torch

from gnn_fpga_amd import HitGraphBatch, TrackFit, build_tracks, select_hits, synth
from gnn_fpga_amd.model import SegmentClassifier
from poisoned_alloc import poison
from track_fit_cases import (KEYS, STATUS_CASES, assert_fit_equal, barrel_xyz, lengths_case, listed_tracks,
                             spec_of_tracks, three_hit_tracks)
from tracks_cases import BARREL, barrel_batch, path_graph

pytestmark = pytest.mark.gpu
MODES = ("components", "best")


@pytest.fixture(scope="module")
def dev(hip):
    return torch.device("cuda", torch.cuda.current_device())


def run_case(case, dev, dtype=np.float64):
    """The kernel on hand-listed tracks + its comparison with the specification on the same (cast) columns."""
    ptr, hits, x, y, z, max_hits, want = case
    cols = [v.astype(dtype) for v in (x, y, z)]
    tracks = listed_tracks(ptr, hits, x.size, dev)
    fit = tracks.fit(*cols, max_hits=max_hits)
    assert isinstance(fit, TrackFit) and all(getattr(fit, k).is_cuda for k in KEYS)
    assert fit.moments.shape == (len(ptr) - 1, 13) and fit.params.shape == (len(ptr) - 1, 8)
    spec = spec_of_tracks(tracks, *cols, max_hits=max_hits)
    assert_fit_equal(fit, spec)
    if want is not None and dtype == np.float64:
        assert fit.status.tolist() == want
    return fit, spec


@pytest.mark.parametrize("name", sorted(STATUS_CASES))
def test_status_cases(name, dev):
    run_case(STATUS_CASES[name], dev)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_every_length_from_1_to_40(dtype, dev):
    fit, spec = run_case(lengths_case(), dev, dtype)
    assert fit.n_hits.tolist() == list(range(1, 41))
    assert fit.status.tolist() == [1, 1] + [0] * 30 + [2] * 8


@pytest.mark.parametrize("n_tracks", [0, 1, 255, 256, 257])
def test_track_counts_across_the_block_size(n_tracks, dev):
    fit, spec = run_case(three_hit_tracks(n_tracks), dev)
    assert fit.status.shape == (n_tracks,) and not fit.status.any()


@pytest.fixture(scope="module")
def barrel(dev):
    return {row: barrel_batch(row, dev) for row in BARREL}


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("row", sorted(BARREL))
def test_barrel_recipe(row, mode, dtype, barrel, dev):
    batch, scores, pid = barrel[row]
    tracks = build_tracks(batch, scores, 0.5, mode, 3)
    cols = [torch.from_numpy(v).to(dev, dtype) for v in barrel_xyz(row, batch)]
    fit = tracks.fit(*cols)
    assert len(tracks) == BARREL[row][1][mode][1] and fit.params.is_cuda
    assert_fit_equal(fit, spec_of_tracks(tracks, *cols))
    if mode == "best":
        assert not fit.status.any()
    elif dtype == torch.float64:                        # the cut of the issue's table, on the device
        sel = tracks.match(pid).select(fit.good(0.05, 2.0))
        assert sel.is_cuda and sel.tolist()[:2] == {(40, 40, 2, 1, 3): [8, 8], (300, 300, 2, 2, 4): [4, 4]}[row]


def test_hit_ids_in_permuted_order(dev):
    """One path of 1200 hits numbered in a seeded permuted order, cut into short chains: a track's list is in
    ascending hit id, which is not the order along the path, and its hits lie all over the coordinate columns."""
    g, scores = path_graph(1200, "permuted", seed=41)
    rng = np.random.default_rng(42)
    scores = np.where(rng.random(scores.size) < 0.2, np.float32(0.1), scores)
    batch = HitGraphBatch.from_graphs([g]).to(dev)
    tracks = build_tracks(batch, torch.from_numpy(scores).to(dev), 0.5, "components", 1)
    x, y, z = (rng.normal(0.0, 300.0, size=1200) for _ in range(3))
    fit = tracks.fit(x, y, z, max_hits=8)
    assert_fit_equal(fit, spec_of_tracks(tracks, x, y, z, max_hits=8))
    n = fit.n_hits.cpu().numpy()
    assert len(tracks) > 150 and n.min() == 1 and n.max() > 8 and (fit.status == 0).sum() > 50
    ids = tracks.track_hits.cpu().numpy()
    assert (np.diff(ids) != 1).mean() > 0.9             # the lists do not run along the columns


def test_two_runs_and_poisoned_allocations_give_the_same_bits(barrel, dev):
    batch, scores, pid = barrel[(300, 300, 2, 2, 4)]
    tracks = build_tracks(batch, scores, 0.5, "best", 3)
    cols = [torch.from_numpy(v).to(dev) for v in barrel_xyz((300, 300, 2, 2, 4), batch)]
    len(tracks), tracks.track_hits                       # the lists are filled before anything is poisoned

    def call():
        fit = tracks.fit(*cols)
        return [getattr(fit, k).clone().reshape(-1).view(torch.uint8) for k in KEYS]
    plain, again = call(), call()
    assert all(torch.equal(a, b) for a, b in zip(plain, again))
    for case in (lengths_case(), STATUS_CASES["mixed"]):
        ptr, hits, x, y, z, max_hits, _ = case
        listed = listed_tracks(ptr, hits, x.size, dev)
        first = listed.fit(x, y, z, max_hits)
        for pattern in ("ff", "one"):
            with poison(pattern) as p:
                got = listed.fit(x, y, z, max_hits)
                assert len(p.records) == 4               # moments, params, n_fit, status - allocated in _lib only
                damaged = p.guards_intact()
                clone = {k: getattr(got, k).clone() for k in KEYS}
            assert damaged == [], (pattern, damaged)
            assert_fit_equal(clone, {k: getattr(first, k).cpu().numpy() for k in KEYS}, pattern)
    for pattern in ("ff", "one"):
        with poison(pattern) as p:
            got = call()
            damaged = p.guards_intact()
        assert damaged == [] and all(torch.equal(a, b) for a, b in zip(plain, got)), pattern


@pytest.mark.parametrize("mode", MODES)
def test_the_whole_chain_on_the_device(mode, dev):
    ev = synth.trackml_events(2, 60, 60, seed=6)
    up = lambda table: {k: v if k == "event_ptr" else torch.from_numpy(v).to(dev)      # noqa: E731
                        for k, v in table.items()}
    hits = up(ev["hits"])
    sel = select_hits(hits, up(ev["truth"]), up(ev["particles"]))
    batch = sel.build_graphs(n_phi_sectors=2, phi_slope_max=0.002, z0_max=400.0)
    torch.manual_seed(0)
    model = SegmentClassifier(3, 8, 3).to(dev).eval()
    with torch.no_grad():
        scores = model(batch)
    tracks = build_tracks(batch, scores, float(scores.median()), mode, 3)
    row = sel.row[batch.hit_index]                      # batch hit -> selected hit -> row of the raw hit table
    x, y, z = (hits[k][row] for k in ("x", "y", "z"))
    assert x.is_cuda and x.dtype == torch.float32 and x.shape == (batch.n_hits,)
    fit = tracks.fit(x, y, z)
    assert len(tracks) > 0 and fit.params.is_cuda
    assert_fit_equal(fit, spec_of_tracks(tracks, x, y, z))
    if mode == "best":                                  # simple paths: short enough to be fitted
        assert (fit.status == 0).any()
    m = tracks.match(sel.particle_id[batch.hit_index])
    after = m.select(fit.good(0.05, 2.0))
    assert after.is_cuda and int(after[0]) <= int(m.counts[0]) and int(after[2]) == int(m.counts[2])
