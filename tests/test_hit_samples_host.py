"""The hit-sample builder's specification (gnn-fpga_amd/hit_samples.py) against the reference's own sample
preparation (tests/golden/hit_samples, written by tools/gen_hit_samples_golden.py running cells 5 and 9-15 of
gnn/MPNN_HitClassifier.ipynb), its dense layout, input validation and the C ABI's new entry points; no GPU."""
import glob
import json
import os
import re

import numpy as np
import pytest
import torch

from gnn_fpga_amd import _lib, build_hit_samples, synth
from gnn_fpga_amd.hit_samples import build_hit_samples_numpy, segment_pattern

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hit_samples")
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, "*.npz")))
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(case):
    return dict(np.load(os.path.join(GOLD, case + ".npz")))


def _build(f, **kw):
    args = dict(n_det_layers=int(f["n_det_layers"]), n_layer_hits=int(f["n_layer_hits"]),
                n_seed_layers=int(f["n_seed_layers"]))
    args.update(kw)
    return build_hit_samples(f["r"], f["phi"], f["z"], f["layer"], f["particle_id"], f["event_ptr"], **args)


def test_fixtures_cover_the_cases():
    assert set(CASES) >= {"duplicates", "missing_layers", "event_fails_count", "absent_layer", "shared_noise",
                          "phi_edges", "k8_seed2", "k3_seed0", "notebook"}
    for c in CASES:
        f = _load(c)
        assert int(f["min_gap_ulps"]) > 0, "%s has an exact tie at a selection boundary" % c
        assert json.loads(str(f["dtypes"])) == {"d": "float32", "deta": "float32", "dphi": "float32",
                                                "features": "float64", "lay_eta": "float32", "trk_eta": "float64"}


@pytest.mark.parametrize("case", CASES)
def test_specification_equals_the_reference(case):
    f = _load(case)
    s = _build(f)
    X, Ri, Ro, y = s.dense()
    assert np.array_equal(s.keys.numpy(), f["sig_keys"])                       # the sample set and order
    assert np.array_equal(X.view(np.uint32), f["full_X"].view(np.uint32))     # candidate order and features
    assert np.array_equal(y, f["full_y"])
    assert np.array_equal(Ri, f["full_Ri"]) and np.array_equal(Ro, f["full_Ro"])


def test_fixture_traps_are_present():
    """The cases pin what they are named for."""
    dup = _load("duplicates")
    assert dup["r"].shape[0] > len(np.unique(np.stack([np.repeat(np.arange(len(dup["event_ptr"]) - 1),
                                                                 np.diff(dup["event_ptr"])),
                                                       dup["particle_id"], dup["layer"]]), axis=1))
    ev = _load("event_fails_count")
    s = _build(ev)
    assert 1 not in set(s.keys[:, 0].tolist())                                 # event 1 fails its layer count
    sn = _load("shared_noise")
    assert 0 in set(_build(sn).keys[:, 1].tolist())                            # noise id 0 on all layers: a track
    pe = _load("phi_edges")
    assert np.abs(pe["phi"]).max() > 3.12


def test_hit_index_and_labels_are_consistent():
    f = _load("notebook")
    s = _build(f)
    hi = s.hit_index.numpy()
    L, K = s.n_det_layers, s.n_layer_hits
    assert np.array_equal(f["layer"][hi], np.tile(np.repeat(np.arange(L), K), len(s)))
    assert np.array_equal(s.y.numpy(), (f["particle_id"][hi] == np.repeat(s.keys[:, 1].numpy(), L * K)))
    assert np.array_equal(s.batch.X[:, 0].numpy(), (f["r"][hi].astype(np.float64) / 1000.0).astype(np.float32))


def test_dense_layout_and_segments_match_synth():
    ref = synth.hit_classifier_samples(1)
    src, dst = segment_pattern(10, 5)
    assert np.array_equal(src, ref.src) and np.array_equal(dst, ref.dst)
    s = _build(_load("notebook"))
    X, Ri, Ro, y = s.dense()
    assert X.shape == (len(s), 50, 4) and Ri.shape == Ro.shape == (len(s), 50, 225) and y.dtype == np.uint8
    assert np.array_equal(Ri[0], ref.Ri[0]) and np.array_equal(Ro[0], ref.Ro[0])
    b = s.batch
    assert b.n_graphs == len(s) and np.array_equal(b.hit_ptr, np.arange(len(s) + 1) * 50)
    assert np.array_equal(b.src.numpy()[225:450], ref.src + 50)
    bj, yj = s.batch_of(3, 4)
    assert bj.n_graphs == 4 and torch.equal(bj.X, b.X[150:350]) and torch.equal(yj, s.y[150:350])
    assert torch.equal(bj.src, b.src[:4 * 225]) and torch.equal(bj.dst, b.dst[:4 * 225])


def test_ties_go_to_the_earlier_row():
    """Two hits at the same (r, phi, z) on each layer tie on d: the earlier row comes first."""
    r = np.array([30, 30, 30, 60, 60, 60], np.float32)
    phi = np.array([0.1, 0.2, 0.2, 0.1, 0.3, 0.3], np.float32)
    z = np.zeros(6, np.float32)
    layer = np.array([0, 0, 0, 1, 1, 1], np.int32)
    pid = np.array([7, 1, 2, 7, 3, 4], np.int64)
    s = build_hit_samples(r, phi, z, layer, pid, n_det_layers=2, n_layer_hits=2, n_seed_layers=1)
    assert s.keys.tolist() == [[0, 7]] and s.hit_index.tolist() == [0, 1, 3, 4]
    s = build_hit_samples(r[::-1].copy(), phi[::-1].copy(), z, layer[::-1].copy(), pid[::-1].copy(), n_det_layers=2,
                          n_layer_hits=2, n_seed_layers=1)
    assert s.hit_index.tolist() == [5, 3, 2, 0]


def test_zero_samples_and_empty_input():
    f = _load("notebook")
    s = _build(f, n_det_layers=11)                 # no track crosses 11 layers
    assert len(s) == 0 and s.batch.n_hits == 0 and s.dense()[0].shape == (0, 55, 4)
    e = build_hit_samples(np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.float32),
                          np.zeros(0, np.int32), np.zeros(0, np.int64))
    assert len(e) == 0 and e.keys.shape == (0, 2)


def test_input_validation():
    f = _load("absent_layer")
    r, phi, z, lay, pid, ep = (f[k] for k in ("r", "phi", "z", "layer", "particle_id", "event_ptr"))
    with pytest.raises(ValueError, match="float64"):
        build_hit_samples(r.astype(np.float64), phi, z, lay, pid, ep)
    with pytest.raises(ValueError):
        build_hit_samples(r, phi[:-1], z, lay, pid, ep)
    with pytest.raises(ValueError, match="particle_id"):
        build_hit_samples(r, phi, z, lay, None, ep)
    with pytest.raises(ValueError, match="event_ptr"):
        build_hit_samples(r, phi, z, lay, pid, ep[::-1].copy())
    for kw in ({"n_layer_hits": 17}, {"n_det_layers": 65}, {"n_layer_hits": 0}, {"n_seed_layers": -1},
               {"feature_scale": (1.0, 0.0, 1.0)}, {"feature_scale": (1.0, 2.0)}):
        with pytest.raises(ValueError):
            build_hit_samples(r, phi, z, lay, pid, ep, **kw)
    bad = lay.copy()
    bad[3] = 10
    with pytest.raises(ValueError, match="layer outside"):
        build_hit_samples(r, phi, z, bad, pid, ep)
    for col in ("r", "phi", "z"):
        c = {"r": r.copy(), "phi": phi.copy(), "z": z.copy()}
        c[col][5] = np.nan
        with pytest.raises(ValueError, match="non-finite"):
            build_hit_samples(c["r"], c["phi"], c["z"], lay, pid, ep)
    s = build_hit_samples(torch.from_numpy(r), torch.from_numpy(phi), torch.from_numpy(z), torch.from_numpy(lay),
                          torch.from_numpy(pid), ep)
    assert s.batch.X.device.type == "cpu"


def test_new_symbols_are_declared_bound_and_exported():
    with open(os.path.join(REPO, "include", "gnn_hip.h")) as fh:
        hdr = fh.read()
    names = ("gnn_hit_samples_workspace_bytes", "gnn_hit_samples_sizes", "gnn_hit_samples_fill")
    for n in names:
        assert re.search(r"\b%s\(" % n, hdr) and n in _lib.SIGNATURES
    assert "GNN_ABI_VERSION 7" in hdr
    lib = _lib.load()
    for n in names:
        assert hasattr(lib, n)
    assert lib.gnn_hit_samples_workspace_bytes(100, 1, 65, 5) == 0
    assert "n_det_layers" in lib.gnn_last_error().decode()
    assert lib.gnn_hit_samples_workspace_bytes(100, 1, 10, 17) == 0
    assert lib.gnn_hit_samples_sizes(None, None, None, None, None, 10, None, 1, 10, 17, None, 0, None,
                                     None) == _lib.GNN_ERR_BADARG
    flagged = _lib.GnnHitSamplesSizes(n_samples=1, n_hits=50, n_segments=225, status=8)
    assert lib.gnn_hit_samples_fill(None, None, None, None, 100, 1, 10, 5, 3, 1.0, 1.0, 1.0, flagged, None, 0,
                                    *([None] * 7)) == _lib.GNN_ERR_BADARG
    assert "flagged" in lib.gnn_last_error().decode()


def test_new_kernels_have_no_scratch():
    path = os.path.join(REPO, "build", "hit_samples.remarks")
    if not os.path.exists(path):
        pytest.fail("build/hit_samples.remarks is missing: build the library first")
    with open(path) as fh:
        text = fh.read()
    blocks = re.split(r"remark: Function Name: ", text)[1:]
    ours = [b for b in blocks if "k_hs_" in b.split()[0]]
    assert len(ours) >= 16 + 14
    for b in ours:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, b.split()[0]


def test_numpy_entry_point_matches():
    f = _load("k8_seed2")
    a = _build(f)
    b = build_hit_samples_numpy(f["r"], f["phi"], f["z"], f["layer"], f["particle_id"], f["event_ptr"], 10, 8, 2,
                                (1000.0, np.pi, 1000.0))
    assert torch.equal(a.batch.X, b.batch.X) and torch.equal(a.hit_index, b.hit_index)
