"""The hit-sample builder on the GPU (csrc/hit_samples.hip): exactly the reference's samples on its fixtures
(tests/golden/hit_samples), the specification (gnn-fpga_amd/hit_samples.py) on seeded inputs up to detector scale
with only near-tie swaps allowed, reproducibility, empty inputs, status errors, a grid past 65 535 samples, and
the samples feeding a NodeClassifier end to end."""
import glob
import os

import numpy as np
import pytest
import torch

import nodeclf_fp64 as ref64
from gnn_fpga_amd import HitGraphBatch, build_hit_samples, evaluate, synth
from gnn_fpga_amd.hit_samples import calc_dphi32, eta32, eta64
from gnn_fpga_amd.loss import BCELoss
from gnn_fpga_amd.model import NodeClassifier

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "hit_samples")
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, "*.npz")))
DEV = torch.device("cuda:0")
COLS = ("r", "phi", "z", "layer", "particle_id")
# the last word of each float32 function (atan2, tan, log) may differ by up to this many ulps between the device's
# and numpy's implementations (each documents at most 4; 2 x 4)
FN_ULPS = 8


def _dev(cols):
    return [torch.from_numpy(np.ascontiguousarray(c)).to(DEV) for c in cols]


def _both(cols, ep, **kw):
    host = build_hit_samples(*cols, event_ptr=ep, **kw)
    dev = build_hit_samples(*_dev(cols), event_ptr=ep, **kw)
    return host, dev


def _ulp(x):
    x = np.abs(np.asarray(x, np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def _bound(r, z, teta, d):
    """|d_device - d_spec| bound per candidate: the eta error of the float32 chain from each function's error
    (atan2: FN_ULPS ulp of theta / sin(theta); tan: FN_ULPS * 2^-23 relative, i.e. absolute in log; log: FN_ULPS ulp
    of eta), one ulp of the rounded float64 track eta, and the roundings of deta and d."""
    th = np.arctan2(r.astype(np.float64), z.astype(np.float64))
    e = eta32(r, z)
    b_eta = FN_ULPS * _ulp(np.arctan2(r, z)) / np.sin(th) + FN_ULPS * 2.0 ** -23 + FN_ULPS * _ulp(e)
    return b_eta + _ulp(teta) + _ulp(e - teta) + 2 * _ulp(d)


def _compare(cols, ep, host, dev, L, K):
    """Exact except for near-tie swaps; returns the number of swapped (sample, layer) lists."""
    r, phi, z, layer, pid = cols
    assert torch.equal(dev.keys.cpu(), host.keys)
    hd, hh = dev.hit_index.cpu().numpy(), host.hit_index.numpy()
    swaps = 0
    if not np.array_equal(hd, hh):
        bd, bh = hd.reshape(-1, K), hh.reshape(-1, K)
        for q in np.flatnonzero(np.any(bd != bh, axis=1)):
            s, l = divmod(int(q), L)
            trow = hh[(s * L + l) * K]                        # not necessarily the track hit: recompute it
            rows_s = hh[s * L * K:(s + 1) * L * K]
            t = [i for i in rows_s if layer[i] == l and pid[i] == host.keys[s, 1].item()]
            trow = t[0] if t else trow
            teta = np.float32(eta64(r[trow], z[trow]))

            def dist(h):
                de = eta32(r[h], z[h]) - teta
                dp = calc_dphi32(phi[trow], phi[h])
                return np.sqrt(de * de + dp * dp)
            dd, dh = dist(bd[q]), dist(bh[q])
            assert len(set(bd[q].tolist())) == K and np.all(layer[bd[q]] == l)
            tol = _bound(r[bd[q]], z[bd[q]], teta, dd) + _bound(r[bh[q]], z[bh[q]], teta, dh)
            assert np.all(np.abs(dd.astype(np.float64) - dh) <= tol), (q, dd, dh, tol)
            swaps += 1
    # every value follows from hit_index exactly
    same = np.repeat(np.all(hd.reshape(-1, K) == hh.reshape(-1, K), axis=1), K)
    Xd, Xh = dev.batch.X.cpu().numpy(), host.batch.X.numpy()
    assert np.array_equal(Xd[same].view(np.uint32), Xh[same].view(np.uint32))
    assert np.array_equal(dev.y.cpu().numpy(), (pid[hd] == np.repeat(host.keys[:, 1].numpy(), L * K)).astype(np.float32))
    assert np.array_equal(Xd[:, 0], (r[hd].astype(np.float64) / 1000.0).astype(np.float32))
    assert torch.equal(dev.batch.src.cpu(), host.batch.src) and torch.equal(dev.batch.dst.cpu(), host.batch.dst)
    assert np.array_equal(dev.batch.hit_ptr, host.batch.hit_ptr) and np.array_equal(dev.batch.seg_ptr,
                                                                                     host.batch.seg_ptr)
    return swaps


@pytest.mark.parametrize("case", CASES)
def test_device_equals_the_reference(hip, case):
    f = dict(np.load(os.path.join(GOLD, case + ".npz")))
    cols = [f[k] for k in COLS]
    kw = dict(n_det_layers=int(f["n_det_layers"]), n_layer_hits=int(f["n_layer_hits"]),
              n_seed_layers=int(f["n_seed_layers"]))
    s = build_hit_samples(*_dev(cols), event_ptr=f["event_ptr"], **kw)
    assert s.batch.X.is_cuda and s.y.is_cuda and s.keys.is_cuda
    X, Ri, Ro, y = s.dense()
    assert np.array_equal(s.keys.cpu().numpy(), f["sig_keys"])
    assert np.array_equal(X.view(np.uint32), f["full_X"].view(np.uint32))
    assert np.array_equal(y, f["full_y"])
    assert np.array_equal(Ri, f["full_Ri"]) and np.array_equal(Ro, f["full_Ro"])


SPEC_CASES = [(20, 50, 1, 0), (30, 0, 1, 1), (50, 200, 2, 2), (100, 500, 1, 3), (100, 1000, 3, 4),
              (200, 2000, 2, 5), (300, 300, 4, 6), (500, 5000, 1, 7), (500, 1000, 2, 8), (1000, 10000, 1, 9),
              (1000, 10000, 3, 10), (1000, 2000, 2, 11), (64, 64, 8, 12), (65, 300, 2, 13), (10, 20, 16, 14),
              (800, 8000, 2, 15), (150, 3000, 3, 16), (1000, 0, 2, 17), (400, 4000, 3, 18), (1000, 10000, 4, 19)]


@pytest.mark.parametrize("n_tracks,n_noise,n_events,seed", SPEC_CASES)
def test_device_equals_the_specification(hip, n_tracks, n_noise, n_events, seed):
    ev = synth.barrel_event(n_tracks, n_noise, n_events=n_events, seed=100 + seed)
    cols = [ev.r, ev.phi, ev.z, ev.layer, ev.particle_id]
    K = (5, 3, 8, 16)[seed % 4]
    host, dev = _both(cols, ev.event_ptr, n_layer_hits=K, n_seed_layers=seed % 4)
    assert len(host) > 0
    swaps = _compare(cols, ev.event_ptr, host, dev, 10, K)
    print("barrel_event(%d, %d, %d events): %d samples, %d near-tie swaps" % (n_tracks, n_noise, n_events,
                                                                               len(host), swaps))


def test_two_builds_are_identical(hip):
    ev = synth.barrel_event(1000, 10000, n_events=2, seed=3)
    cols = _dev([ev.r, ev.phi, ev.z, ev.layer, ev.particle_id])
    a = build_hit_samples(*cols, event_ptr=ev.event_ptr)
    b = build_hit_samples(*cols, event_ptr=ev.event_ptr)
    for u, v in ((a.batch.X, b.batch.X), (a.y, b.y), (a.hit_index, b.hit_index), (a.keys, b.keys),
                 (a.batch.src, b.batch.src), (a.batch.dst, b.batch.dst)):
        assert torch.equal(u, v)


def test_empty_input_and_zero_samples(hip):
    e = build_hit_samples(*_dev([np.zeros(0, np.float32)] * 3 + [np.zeros(0, np.int32), np.zeros(0, np.int64)]))
    assert len(e) == 0 and e.keys.shape == (0, 2) and e.batch.n_hits == 0
    ev = synth.barrel_event(3, 0, n_events=2, seed=1)            # 3 hits per layer: every event fails the count
    s = build_hit_samples(*_dev([ev.r, ev.phi, ev.z, ev.layer, ev.particle_id]), event_ptr=ev.event_ptr)
    assert len(s) == 0 and s.y.numel() == 0


def test_status_errors_raise(hip):
    ev = synth.barrel_event(20, 30, n_events=2, seed=2)
    base = [ev.r, ev.phi, ev.z, ev.layer, ev.particle_id]
    lay = ev.layer.copy()
    lay[7] = 10
    with pytest.raises(ValueError, match="layer outside"):
        build_hit_samples(*_dev(base[:3] + [lay, base[4]]), event_ptr=ev.event_ptr)
    for c in range(3):
        bad = [x.copy() for x in base]
        bad[c][11] = np.inf if c else np.nan
        with pytest.raises(ValueError, match="non-finite"):
            build_hit_samples(*_dev(bad), event_ptr=ev.event_ptr)
    with pytest.raises(ValueError, match="event_ptr"):
        build_hit_samples(*_dev(base), event_ptr=ev.event_ptr[::-1].copy())
    s = build_hit_samples(*_dev(base), event_ptr=ev.event_ptr)      # the device is fine afterwards
    assert len(s) == 40


def test_more_than_65535_samples(hip):
    ev = synth.barrel_event(1000, 0, n_events=70, seed=21)
    cols = [ev.r, ev.phi, ev.z, ev.layer, ev.particle_id]
    host, dev = _both(cols, ev.event_ptr)
    assert len(host) == 70000
    _compare(cols, ev.event_ptr, host, dev, 10, 5)


def test_node_classifier_end_to_end(hip):
    f = dict(np.load(os.path.join(GOLD, "notebook.npz")))
    cols = [f[k] for k in COLS]
    s = build_hit_samples(*_dev(cols), event_ptr=f["event_ptr"])
    fx = ref64.fixture(os.path.join(HERE, "golden", "node_classifier", "d8_t1_b4.npz"))
    D, T = int(fx["hidden_dim"]), int(fx["n_iters"])
    m = NodeClassifier(input_dim=4, hidden_dim=D, n_iters=T)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in fx["params"].items()})
    m = m.to(DEV).eval()
    n = len(s)
    ref_batch = HitGraphBatch(f["full_X"].reshape(-1, 4), s.batch.src.cpu().numpy(), s.batch.dst.cpu().numpy(),
                              hit_ptr=s.batch.hit_ptr, seg_ptr=s.batch.seg_ptr).to(DEV)
    with torch.no_grad():
        ref = m(ref_batch)
        got = m(s.batch)
    assert got.shape == ref.shape == (n * 50,)
    assert torch.equal(got, ref)
    m.train()
    opt = torch.optim.Adam(m.parameters())
    b, y = s.batch_of(0, 16)
    opt.zero_grad()
    loss = BCELoss()(m(b), y)
    loss.backward()
    opt.step()
    assert torch.isfinite(loss)

    def gen():
        for j in range(0, n, 32):
            yield s.batch_of(j, 32)
    met = evaluate(m, gen(), (n + 31) // 32, thresholds=(0.5,))
    status, counts, _ = met._views()
    assert int(status.item()) == 0 and int(counts.cpu().numpy()[0].sum()) == n * 50
