"""The bf16 matrix-core forward (GNN_FLAG_BF16_MLP, model.mlp_bf16: hidden_dim 32 / 64) against a bf16-faithful fp64
reference: oracle/bf16_torch.py, the same forward with every product and sum in fp64 but rounded to bf16 at exactly
the points where the kernels round.

tests/test_gpu_parity.py and tests/test_gpu_stress.py hold this route to the fp32 oracle at TOL_BF16 = 2e-3, which is
the size of the bf16 effect itself (measured max 6e-4): a kernel that truncated instead of rounding, left X
unrounded or kept a record in the wrong precision would still pass there.  Against its own emulation the route is
held to what fp32 accumulation moves (a value that lands next to a bf16 rounding midpoint may round the other way):

  max |GPU - emulation| <= B_max and mean |GPU - emulation| <= B_mean of the case (BF16_BOUNDS), and
  mean |GPU - emulation| <= MEAN_SHARE[T] x mean |GPU - fp64 forward| (the emulation explains most of the bf16 error).

Every case runs both wide kernels - k_iter_w (round barriers, GNN_WIDE_LOCKSTEP=1) and k_iter_wx (sweep waves +
matrix-core waves, GNN_WIDE_ROLES=1) - and the default choice; each must show k_pack16 (the bf16 route ran; its input
kernel k_input4_bf is launched under the name k_input4) and the three must agree bit for bit.  Weights: default
initialisation (the exp-product bound is far below 60: GNN_FLAG_EXP_PRODUCT on) and the same with
model.exp_product = False (the exact-tanh records: k_pack16(xp = 0), k_input4_bf<XP = false>, k_iter_w<.., false>).

GNN_TEST_RECORD=<file> receives every comparison's numbers (tests/test_gpu_fp64_reference.py's format).
"""
import numpy as np
import pytest
import torch

import fp64_graphs
from gnn_fpga_amd import HitGraphBatch
from oracle import bf16_torch, index_torch
from oracle.dense_torch import KEYS

pytestmark = pytest.mark.gpu

# mean |GPU - emulation| / mean |GPU - fp64 forward| by n_iters.  0.2 holds up to T = 2 (worst measured 0.157); deeper
# networks carry more of the fp32 noise forward (a flipped rounding in iteration 1 moves every later one): measured
# worst 0.323 at T = 3, 0.531 at mu200's T = 6, where the CPU floor (fp32 alone) is 3.43e-5 = the GPU's own 3.43e-5
MEAN_SHARE = {1: 0.2, 2: 0.2, 3: 0.4, 6: 0.65}

SHAPES = ((2, 32), (3, 32), (3, 64))
FAMILIES = ("c3x4", "hubs", "ragged", "superhub")
# (family, F, D, T, exp-product on, masked)
CASES = ([(f, F, D, T, xp, False) for f in FAMILIES for F, D in SHAPES for T in (1, 2, 3) for xp in (True, False)] +
         [("mu200", 3, 64, 6, xp, False) for xp in (True, False)] +
         [("c3x4", 3, 64, 2, True, True)])
WHY = {"c3x4": "40 k hits (k_iter_wx by default), 1 % padded segments scattered",
       "hubs": "in- and out-degrees 1 ... 4097, 50 isolated hits",
       "ragged": "a 1-hit self-loop, graphs below one slice, an all-padded graph, 200 small graphs",
       "superhub": "a 70 000-segment hit: the torch plan builder",
       "mu200": "the mu200 notebook's (3, 64, 6) at 500 k segments"}

# {case: (B_max, B_mean, (max, mean) |GPU - emulation| measured on MI355X with GNN_TEST_RECORD)}.  Each bound lies
# above the measured error and is at most 2.5 x it and at most 2.5 x the bf16 floor: the worst max / mean of
# |fp32-accumulated emulation - fp64-accumulated emulation| over five segment orders, which
# tests/test_oracle_bf16_host.py recomputes on the CPU and checks against every entry here.
BF16_BOUNDS = {
    ('c3x4', 2, 32, 1, True, False): (0.00026, 7e-07, (0.00014, 3.89e-07)),  # floor 0.00014, 3.98e-07
    ('c3x4', 2, 32, 1, False, False): (0.00025, 7.3e-07, (0.000134, 4.01e-07)),  # floor 0.000137, 4.19e-07
    ('c3x4', 2, 32, 2, True, False): (0.00036, 6.6e-06, (0.000197, 3.62e-06)),  # floor 0.000197, 4.15e-06
    ('c3x4', 2, 32, 2, False, False): (0.00035, 6e-06, (0.000194, 3.33e-06)),  # floor 0.00024, 3.88e-06
    ('c3x4', 2, 32, 3, True, False): (0.00036, 2.5e-05, (0.000203, 1.4e-05)),  # floor 0.000199, 1.37e-05
    ('c3x4', 2, 32, 3, False, False): (0.0004, 2.4e-05, (0.000219, 1.35e-05)),  # floor 0.000245, 1.32e-05
    ('c3x4', 3, 32, 1, True, False): (0.00023, 5.5e-07, (0.000123, 3.04e-07)),  # floor 0.000151, 3.14e-07
    ('c3x4', 3, 32, 1, False, False): (0.00023, 4.9e-07, (0.000127, 2.68e-07)),  # floor 0.000127, 2.71e-07
    ('c3x4', 3, 32, 2, True, False): (0.00036, 7.4e-06, (0.000197, 4.07e-06)),  # floor 0.000197, 4.64e-06
    ('c3x4', 3, 32, 2, False, False): (0.00035, 7.7e-06, (0.000193, 4.24e-06)),  # floor 0.000193, 4.58e-06
    ('c3x4', 3, 32, 3, True, False): (0.00038, 3.8e-05, (0.000209, 2.09e-05)),  # floor 0.000213, 2.13e-05
    ('c3x4', 3, 32, 3, False, False): (0.0004, 3.7e-05, (0.000219, 2.02e-05)),  # floor 0.000235, 2.05e-05
    ('c3x4', 3, 64, 1, True, False): (0.00023, 1.3e-06, (0.000132, 6.86e-07)),  # floor 0.000123, 8.01e-07
    ('c3x4', 3, 64, 1, False, False): (0.00018, 1.3e-06, (9.52e-05, 7.03e-07)),  # floor 0.000124, 8.11e-07
    ('c3x4', 3, 64, 2, True, False): (0.00034, 1.8e-05, (0.000187, 9.47e-06)),  # floor 0.000222, 1.02e-05
    ('c3x4', 3, 64, 2, False, False): (0.00029, 1.7e-05, (0.000156, 9.23e-06)),  # floor 0.000157, 9.82e-06
    ('c3x4', 3, 64, 3, True, False): (0.00034, 4.4e-05, (0.00019, 2.41e-05)),  # floor 0.000184, 2.43e-05
    ('c3x4', 3, 64, 3, False, False): (0.00035, 4.3e-05, (0.00019, 2.38e-05)),  # floor 0.000198, 2.38e-05
    ('hubs', 2, 32, 1, True, False): (0.00017, 4.1e-07, (9.23e-05, 2.26e-07)),  # floor 9.22e-05, 2.45e-07
    ('hubs', 2, 32, 1, False, False): (0.00013, 3.1e-07, (7.14e-05, 1.68e-07)),  # floor 7.7e-05, 1.9e-07
    ('hubs', 2, 32, 2, True, False): (0.0002, 2.1e-06, (0.000107, 1.26e-06)),  # floor 0.000107, 1.16e-06
    ('hubs', 2, 32, 2, False, False): (0.00018, 2e-06, (9.62e-05, 1.13e-06)),  # floor 9.62e-05, 1.06e-06
    ('hubs', 2, 32, 3, True, False): (0.00019, 5.3e-06, (0.000102, 2.92e-06)),  # floor 0.000101, 3.13e-06
    ('hubs', 2, 32, 3, False, False): (0.00028, 8.6e-06, (0.000151, 4.72e-06)),  # floor 0.000151, 4.86e-06
    ('hubs', 3, 32, 1, True, False): (0.00015, 3.6e-07, (7.98e-05, 2.3e-07)),  # floor 7.98e-05, 1.99e-07
    ('hubs', 3, 32, 1, False, False): (0.0002, 3.5e-07, (0.000108, 2.29e-07)),  # floor 0.000108, 1.9e-07
    ('hubs', 3, 32, 2, True, False): (0.00016, 1.5e-06, (8.87e-05, 7.82e-07)),  # floor 8.87e-05, 7.97e-07
    ('hubs', 3, 32, 2, False, False): (0.00017, 1.5e-06, (8.94e-05, 8.07e-07)),  # floor 0.00012, 1.1e-06
    ('hubs', 3, 32, 3, True, False): (0.00021, 6.8e-06, (0.000112, 3.74e-06)),  # floor 0.000112, 3.86e-06
    ('hubs', 3, 32, 3, False, False): (0.00033, 8.1e-06, (0.000181, 4.49e-06)),  # floor 0.000181, 4.63e-06
    ('hubs', 3, 64, 1, True, False): (0.00018, 6e-07, (9.74e-05, 3.33e-07)),  # floor 9.74e-05, 3.35e-07
    ('hubs', 3, 64, 1, False, False): (0.00013, 6.2e-07, (7.21e-05, 3.43e-07)),  # floor 8.19e-05, 3.42e-07
    ('hubs', 3, 64, 2, True, False): (0.00017, 3.7e-06, (9.58e-05, 2.02e-06)),  # floor 9.14e-05, 2.05e-06
    ('hubs', 3, 64, 2, False, False): (0.00015, 3.6e-06, (8.02e-05, 1.95e-06)),  # floor 8.02e-05, 2.03e-06
    ('hubs', 3, 64, 3, True, False): (0.00013, 9.7e-06, (6.84e-05, 5.36e-06)),  # floor 9.46e-05, 7.28e-06
    ('hubs', 3, 64, 3, False, False): (0.00012, 9.4e-06, (7.13e-05, 5.2e-06)),  # floor 6.58e-05, 6.51e-06
    ('ragged', 2, 32, 1, True, False): (0.00022, 5.7e-07, (0.00012, 3.45e-07)),  # floor 0.00012, 3.16e-07
    ('ragged', 2, 32, 1, False, False): (0.00021, 5.3e-07, (0.000116, 3.13e-07)),  # floor 0.000116, 2.92e-07
    ('ragged', 2, 32, 2, True, False): (0.00021, 2.9e-06, (0.000115, 1.56e-06)),  # floor 0.000115, 1.66e-06
    ('ragged', 2, 32, 2, False, False): (0.00026, 2.8e-06, (0.000141, 1.52e-06)),  # floor 0.000149, 1.6e-06
    ('ragged', 2, 32, 3, True, False): (0.00032, 1.1e-05, (0.000173, 5.66e-06)),  # floor 0.000173, 5.76e-06
    ('ragged', 2, 32, 3, False, False): (0.00037, 1.1e-05, (0.000202, 5.67e-06)),  # floor 0.000202, 5.8e-06
    ('ragged', 3, 32, 1, True, False): (0.00013, 4.5e-07, (6.91e-05, 2.59e-07)),  # floor 6.69e-05, 2.45e-07
    ('ragged', 3, 32, 1, False, False): (0.00019, 4.9e-07, (0.000104, 2.71e-07)),  # floor 0.000104, 2.76e-07
    ('ragged', 3, 32, 2, True, False): (0.00019, 2.4e-06, (0.000106, 1.29e-06)),  # floor 0.000106, 1.31e-06
    ('ragged', 3, 32, 2, False, False): (0.00015, 2.1e-06, (9.28e-05, 1.14e-06)),  # floor 8.02e-05, 1.13e-06
    ('ragged', 3, 32, 3, True, False): (0.00025, 1.5e-05, (0.000136, 8.31e-06)),  # floor 0.000153, 8.57e-06
    ('ragged', 3, 32, 3, False, False): (0.00024, 1.5e-05, (0.000132, 8e-06)),  # floor 0.00015, 8.44e-06
    ('ragged', 3, 64, 1, True, False): (0.0002, 9.5e-07, (0.000109, 5.27e-07)),  # floor 0.000112, 5.6e-07
    ('ragged', 3, 64, 1, False, False): (0.00015, 9e-07, (8.01e-05, 4.98e-07)),  # floor 8.01e-05, 5.24e-07
    ('ragged', 3, 64, 2, True, False): (0.00025, 6.6e-06, (0.000136, 3.66e-06)),  # floor 0.000185, 3.69e-06
    ('ragged', 3, 64, 2, False, False): (0.00026, 6.7e-06, (0.00014, 3.73e-06)),  # floor 0.00014, 3.72e-06
    ('ragged', 3, 64, 3, True, False): (0.00037, 1.8e-05, (0.000204, 9.66e-06)),  # floor 0.000204, 9.65e-06
    ('ragged', 3, 64, 3, False, False): (0.00037, 1.7e-05, (0.000205, 9.43e-06)),  # floor 0.000205, 9.61e-06
    ('superhub', 2, 32, 1, True, False): (0.00012, 2.2e-07, (8.27e-05, 1.2e-07)),  # floor 6.49e-05, 1.17e-07
    ('superhub', 2, 32, 1, False, False): (0.00014, 2.4e-07, (7.46e-05, 1.32e-07)),  # floor 7.46e-05, 1.35e-07
    ('superhub', 2, 32, 2, True, False): (0.0002, 7.7e-07, (0.000107, 4.27e-07)),  # floor 0.000107, 4.52e-07
    ('superhub', 2, 32, 2, False, False): (0.00018, 8e-07, (9.52e-05, 4.41e-07)),  # floor 9.52e-05, 4.46e-07
    ('superhub', 2, 32, 3, True, False): (0.0002, 1.7e-06, (0.000109, 9.26e-07)),  # floor 0.000109, 9.23e-07
    ('superhub', 2, 32, 3, False, False): (0.00014, 1.8e-06, (7.6e-05, 9.64e-07)),  # floor 9.27e-05, 9.69e-07
    ('superhub', 3, 32, 1, True, False): (0.00012, 2e-07, (6.18e-05, 1.24e-07)),  # floor 7.09e-05, 1.06e-07
    ('superhub', 3, 32, 1, False, False): (9.5e-05, 1.9e-07, (7.13e-05, 1.3e-07)),  # floor 5.25e-05, 1.03e-07
    ('superhub', 3, 32, 2, True, False): (0.00016, 6.6e-07, (8.66e-05, 3.62e-07)),  # floor 8.66e-05, 3.72e-07
    ('superhub', 3, 32, 2, False, False): (0.00014, 6.1e-07, (7.28e-05, 3.37e-07)),  # floor 7.67e-05, 3.65e-07
    ('superhub', 3, 32, 3, True, False): (0.00019, 2.2e-06, (0.000102, 1.21e-06)),  # floor 0.000103, 1.26e-06
    ('superhub', 3, 32, 3, False, False): (0.00016, 2e-06, (8.99e-05, 1.11e-06)),  # floor 8.5e-05, 1.14e-06
    ('superhub', 3, 64, 1, True, False): (0.00015, 4e-07, (8.13e-05, 2.21e-07)),  # floor 8.13e-05, 2.22e-07
    ('superhub', 3, 64, 1, False, False): (0.00011, 3.9e-07, (6.08e-05, 2.13e-07)),  # floor 6.08e-05, 2.15e-07
    ('superhub', 3, 64, 2, True, False): (0.00015, 1.5e-06, (8.08e-05, 8.04e-07)),  # floor 8.07e-05, 8.23e-07
    ('superhub', 3, 64, 2, False, False): (0.00013, 1.5e-06, (6.98e-05, 7.79e-07)),  # floor 7.52e-05, 8.3e-07
    ('superhub', 3, 64, 3, True, False): (0.00017, 4.6e-06, (9.36e-05, 2.5e-06)),  # floor 9.36e-05, 2.52e-06
    ('superhub', 3, 64, 3, False, False): (0.00019, 4.4e-06, (0.000104, 2.44e-06)),  # floor 0.000101, 2.48e-06
    ('mu200', 3, 64, 6, True, False): (0.00042, 6.2e-05, (0.000231, 3.43e-05)),  # floor 0.000267, 3.43e-05
    ('mu200', 3, 64, 6, False, False): (0.00038, 6.2e-05, (0.000208, 3.41e-05)),  # floor 0.000249, 3.41e-05
    ('c3x4', 3, 64, 2, True, True): (3e-05, 2.8e-07, (1.64e-05, 1.54e-07)),  # floor 1.64e-05, 1.57e-07
}

DEAD_UNITS = 36         # of the masked (3, 64) model's 64: <= 32 live units in every width -> it runs at hidden_dim 32


def case_id(c):
    return "%s-F%d-D%d-T%d-%s%s" % (c[0], c[1], c[2], c[3], "xp" if c[4] else "exact", "-masked" if c[5] else "")


def _masks(F, D, seed):
    """Random masks (density 0.7 / 0.8) with DEAD_UNITS hit features, edge units and node units dead everywhere."""
    g = torch.Generator().manual_seed(seed)
    C = F + D
    dead = torch.randperm(D, generator=g)[:DEAD_UNITS]
    m1 = (torch.rand(D, 2 * C, generator=g) < 0.7).float()
    m2 = (torch.rand(1, D, generator=g) < 0.8).float()
    m3 = (torch.rand(D, 3 * C, generator=g) < 0.7).float()
    m4 = (torch.rand(D, D, generator=g) < 0.8).float()
    for b in range(2):
        m1[:, b * C + dead] = 0.0          # hit feature k read by nobody
    for b in range(3):
        m3[:, b * C + dead] = 0.0
    m2[0, dead] = 0.0                      # edge unit dropped (W2 = 0)
    m4[:, dead] = 0.0                      # node unit dropped (W4 column = 0)
    return dict(masks_e=[m1, m2], masks_n=[m3, m4])


def model(case):
    """The case's CPU SegmentClassifier (default init) and the ten tensors its bf16 forward receives: the effective
    weights, compacted to the width they run at for the masked model (model.compact_dead_units, as
    SegmentClassifier._cached_weights does on the device)."""
    from gnn_fpga_amd.model import SegmentClassifier, compact_dead_units
    fam, F, D, T, xp, masked = case
    seed = 7 * D + 3 * F + T + (500 if masked else 0)
    torch.manual_seed(seed)
    m = SegmentClassifier(input_dim=F, hidden_dim=D, n_iters=T, **(_masks(F, D, seed) if masked else {}))
    m.exp_product = xp
    w = [t.detach().clone() for t in m.effective_weights()]
    if masked:
        w, D_run, _ = compact_dead_units(w, F, D, [d for d in (4, 8, 16, 32, 64) if d < D])
        assert D_run == 32, D_run
    return m, w


def _record(what, err, scale):
    import os
    rec = os.environ.get("GNN_TEST_RECORD")
    if rec:
        with open(rec, "a") as f:
            f.write("%s\t%.3e\t%.3e\t%.3e\n" % (what, err, scale, err / scale if scale else 0.0))


def _batch(fam):
    return HitGraphBatch(fam.X, fam.src, fam.dst, y=fam.y, hit_ptr=fam.hit_ptr, seg_ptr=fam.seg_ptr).cuda()


class _Refs:
    """fp64 emulations and fp64 forwards per (case, perturbation), kept for the module."""

    def __init__(self):
        self.emu, self.exact = {}, {}

    def emulation(self, case, weights, perturb=None):
        key = (case, perturb)
        if key not in self.emu:
            fam = fp64_graphs.family(case[0], case[1])
            self.emu[key] = bf16_torch.segment_classifier(fam.X, fam.src, fam.dst, weights, case[3], case[4],
                                                          perturb=perturb).numpy()
        return self.emu[key]

    def forward(self, case, weights):
        if case not in self.exact:
            fam = fp64_graphs.family(case[0], case[1])
            p = {k: w.double() for k, w in zip(KEYS, weights)}
            self.exact[case] = index_torch.segment_classifier(fam.X, fam.src, fam.dst, p, case[3]).numpy()
        return self.exact[case]


@pytest.fixture(scope="module")
def refs():
    return _Refs()


def run_bf16(hip, m, b, kernel, monkeypatch):
    """Scores of the bf16 route on `kernel` ("k_iter_w", "k_iter_wx" or None = the default choice) and the names of
    the kernels that ran."""
    monkeypatch.delenv("GNN_WIDE_LOCKSTEP", raising=False)
    monkeypatch.delenv("GNN_WIDE_ROLES", raising=False)
    if kernel == "k_iter_w":
        monkeypatch.setenv("GNN_WIDE_LOCKSTEP", "1")
    elif kernel == "k_iter_wx":
        monkeypatch.setenv("GNN_WIDE_ROLES", "1")
    with torch.no_grad(), hip.profile(512) as prof:
        e = m(b)
        torch.cuda.synchronize()
    monkeypatch.delenv("GNN_WIDE_LOCKSTEP", raising=False)
    monkeypatch.delenv("GNN_WIDE_ROLES", raising=False)
    return e.cpu().numpy().astype(np.float64), {k for k, _ in prof.records}


def gpu_scores(hip, case, monkeypatch):
    """The case on the GPU: scores (default kernel choice), after asserting the route, the exp-product decision,
    the weights the kernels received and that k_iter_w, k_iter_wx and the default agree bit for bit."""
    fam_name, F, D, T, xp, masked = case
    fam = fp64_graphs.family(fam_name, F)
    m, w = model(case)
    m = m.cuda().eval()
    m.use_plan, m.use_events, m.mlp_bf16 = True, False, True
    b = _batch(fam)
    out = {}
    for kernel in ("k_iter_w", "k_iter_wx", None):
        out[kernel], names = run_bf16(hip, m, b, kernel, monkeypatch)
        assert "k_pack16" in names, (case, kernel, sorted(names))
        ran = {"k_iter_w", "k_iter_wx"} & names
        if kernel is not None:
            assert ran == {kernel}, (case, kernel, sorted(names))
        else:
            assert ran == {"k_iter_wx" if b.plan.n_pad >= 32768 else "k_iter_w"}, (case, b.plan.n_pad, sorted(names))
    assert np.array_equal(out["k_iter_w"], out["k_iter_wx"]) and np.array_equal(out["k_iter_w"], out[None]), case
    if xp:                                  # the bound check passed: 2^P 2^Q records
        assert m._xp_cache is not None and m._xp_cache[1] == hip.GNN_FLAG_EXP_PRODUCT, (case, m._xp_cache)
    else:                                   # exp_product = False: no decision taken, the flag stays off
        assert m._xp_cache is None, (case, m._xp_cache)
    kw = m._cached_weights()[0]
    assert len(kw) == len(w) and all(torch.equal(a.cpu(), c) for a, c in zip(kw, w)), case
    if masked:
        info = m.pruned_info()
        assert info is not None and info["hidden_dim"] == 32 and b.plan.hidden_dim == 32, info
    else:
        assert m.pruned_info() is None and b.plan.hidden_dim == D
    if fam_name == "superhub":
        from gnn_fpga_amd.plan_device import DeviceSellPlan
        assert isinstance(b.plan, DeviceSellPlan)
    return out[None], w


def criterion(err, case):
    """(max, mean) of |err| against the case's bounds: (passes, ratio = the larger of max / B_max, mean / B_mean)."""
    B_max, B_mean, _ = BF16_BOUNDS[case]
    mx, mn = float(np.abs(err).max()), float(np.abs(err).mean())
    ratio = max(mx / B_max, mn / B_mean)
    return mx <= B_max and mn <= B_mean, ratio


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_bf16_route_against_its_emulation(hip, refs, case, monkeypatch):
    """The case's scores on the bf16 route against oracle.bf16_torch in fp64: within the case's bounds, and the
    emulation explains most of the distance to the fp64 forward (MEAN_SHARE)."""
    e, w = gpu_scores(hip, case, monkeypatch)
    emu = refs.emulation(case, w)
    ref = refs.forward(case, w)
    err, dev = e - emu, e - ref
    tag = "bf16 %s (%s)" % (case_id(case), WHY[case[0]])
    _record(tag + " |GPU - emulation| max", float(np.abs(err).max()), 1.0)
    _record(tag + " |GPU - emulation| mean", float(np.abs(err).mean()), 1.0)
    _record(tag + " |GPU - fp64 forward| max", float(np.abs(dev).max()), 1.0)
    _record(tag + " |GPU - fp64 forward| mean", float(np.abs(dev).mean()), 1.0)
    assert case in BF16_BOUNDS, case
    ok, ratio = criterion(err, case)
    assert ok, (case, ratio, float(np.abs(err).max()), float(np.abs(err).mean()), BF16_BOUNDS[case])
    share = float(np.abs(err).mean()) / float(np.abs(dev).mean())
    assert share <= MEAN_SHARE[case[3]], (case, share)


@pytest.mark.parametrize("F,D", [(2, 32), (3, 64)])
def test_bf16_declined_without_iterations(hip, F, D):
    """n_iters = 0 with mlp_bf16: the route needs an iteration (choose_route), so the fp32 path runs - same bits, no
    k_pack16."""
    from gnn_fpga_amd.model import SegmentClassifier
    torch.manual_seed(D)
    m = SegmentClassifier(input_dim=F, hidden_dim=D, n_iters=0).cuda().eval()
    m.use_plan, m.use_events = True, False
    b = _batch(fp64_graphs.c3x4(F))
    with torch.no_grad():
        e32 = m(b)
        m.mlp_bf16 = True
        with hip.profile(64) as prof:
            e16 = m(b)
            torch.cuda.synchronize()
    assert "k_pack16" not in {k for k, _ in prof.records}
    assert torch.equal(e32, e16)


# every perturbation of oracle.bf16_torch, each rejected.  Ratio measured on MI355X (xp / exact): trunc 15.8 / 15.9,
# x_unrounded 2.55 / 2.68, q_unrounded 2.54 / 2.68, records_fp32 2.47 / 2.58, exp2_after_round 2.32 / -,
# scale_after_round 2.75 / 2.81, u_rounded 2.39 / 2.50, final_rounded 7.30 / 2.08; the true emulation 0.55 / 0.54
PERTURBED = bf16_torch.PERTURBATIONS


@pytest.mark.parametrize("xp", [True, False], ids=["xp", "exact"])
def test_criterion_sees_a_misplaced_rounding(hip, refs, xp, monkeypatch):
    """The bounds can see a rounding done wrong: the GPU scores of c3x4 (3, 64, 2) fail the case's criterion against
    the emulation with each perturbation of oracle.bf16_torch.PERTURBATIONS (exp2_after_round: exp-product mode
    only) and pass it against the true emulation.  The ratio (the larger of max / B_max and mean / B_mean) of every
    perturbation is recorded."""
    case = ("c3x4", 3, 64, 2, xp, False)
    e, w = gpu_scores(hip, case, monkeypatch)
    errs = {p: e - refs.emulation(case, w, p) for p in (None,) + PERTURBED if p != "exp2_after_round" or xp}
    for p, err in errs.items():
        _record("discrimination %s: %s, max" % (case_id(case), p), float(np.abs(err).max()), 1.0)
        _record("discrimination %s: %s, mean" % (case_id(case), p), float(np.abs(err).mean()), 1.0)
    ok, ratio = criterion(errs[None], case)
    _record("discrimination %s: the true emulation, ratio" % case_id(case), ratio, 1.0)
    assert ok, ratio
    for perturb in PERTURBED:
        if perturb in errs:
            ok, ratio = criterion(errs[perturb], case)
            _record("discrimination %s: %s, ratio" % (case_id(case), perturb), ratio, 1.0)
            assert not ok, (perturb, ratio)
