"""oracle/bf16_torch.py on the CPU: its rounding is the kernels' bf16_rne, with rounding="none" it is the reference's
forward (oracle.index_torch), with rounding="rne" it really rounds, and the bounds of tests/test_gpu_bf16_reference.py
(BF16_BOUNDS) are backed by the bf16 floor recomputed here: the fp32-accumulated emulation over five segment orders
against the fp64-accumulated one, as tests/test_fp32_limit_host.py backs FP32_LIMIT."""
import numpy as np
import pytest
import torch

import fp64_graphs
import test_gpu_bf16_reference as g
from oracle import bf16_torch, index_torch
from oracle.dense_torch import KEYS
from test_gpu_parity import TOL_BF16


bf16_rne_bits = bf16_torch.bf16_rne_bits      # sell_pipeline.hip bf16_rne, integer for integer (NaN case included)


def _torch_bits(u):
    f = torch.from_numpy(np.asarray(u, np.uint32).view(np.float32).copy())
    r = bf16_torch.bf16_round(f)
    return (r.numpy().view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def test_rounding_is_the_kernels_bf16_rne():
    """10^6 random fp32 bit patterns (NaNs excluded here: torch gives every NaN one bit pattern, bf16_rne keeps the
    sign - tests/test_nonfinite_host.py pins the NaN case) plus constructed ties, +-0, subnormals and the largest
    finite values."""
    rng = np.random.default_rng(0)
    u = rng.integers(0, 1 << 32, 1_000_000, dtype=np.uint64).astype(np.uint32)
    u = u[~np.isnan(u.view(np.float32))]
    hi = rng.integers(0, 1 << 15, 4096, dtype=np.uint64).astype(np.uint32) << np.uint32(16)    # sign 0, any exponent
    hi = hi[((hi >> np.uint32(23)) & np.uint32(0xFF)) != 0xFF]
    ties = np.concatenate([hi | 0x8000, (hi | 0x10000) | 0x8000, hi | 0x7FFF, hi | 0x8001])     # even / odd bit 16
    ties = np.concatenate([ties, ties | np.uint32(1 << 31)])
    special = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00008000, 0x00018000, 0x007FFFFF,
                        0x807FFFFF, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0x7F7E8000,
                        0x7F800000, 0xFF800000, 0x3F808000, 0x3F818000], np.uint32)
    for what, bits in (("random", u), ("ties", ties), ("special", special)):
        assert np.array_equal(_torch_bits(bits), bf16_rne_bits(bits)), what
    # a few by hand: ties go to the even neighbour, 0x7F7F8000 (max bf16 + half an ulp) overflows to +inf
    assert list(bf16_rne_bits([0x3F808000, 0x3F818000, 0x7F7F8000, 0x00008000])) == [0x3F80, 0x3F82, 0x7F80, 0x0000]
    # truncation (the "trunc" perturbation) drops the low half
    f = torch.from_numpy(np.array([0x3F81FFFF], np.uint32).view(np.float32))
    assert int(bf16_torch.bf16_round(f, "trunc").numpy().view(np.uint32)[0]) == 0x3F810000


def _weights(F, D, T, seed):
    from gnn_fpga_amd.model import SegmentClassifier
    torch.manual_seed(seed)
    return [t.detach().clone() for t in SegmentClassifier(input_dim=F, hidden_dim=D, n_iters=T).effective_weights()]


@pytest.mark.parametrize("xp", [True, False], ids=["xp", "exact"])
@pytest.mark.parametrize("F,D,T", [(2, 32, 2), (3, 32, 3), (3, 64, 2)])
@pytest.mark.parametrize("fam_name", ["c3x4", "hubs", "ragged"])
def test_unrounded_emulation_is_the_reference(fam_name, F, D, T, xp):
    """rounding="none": the record form (P / R / Q / S / U, edge scores from P_src + Q_dst or 2^P 2^Q, node sums
    over R / S, the NULL rows of the padded segments) is the reference's algebra: index_torch in fp64 at 1e-12.
    rounding="rne" lies within TOL_BF16 of it and more than 1e-6 away (it really rounds)."""
    fam = fp64_graphs.family(fam_name, F)
    w = _weights(F, D, T, 90 + D + T)
    ref = index_torch.segment_classifier(fam.X, fam.src, fam.dst, {k: t.double() for k, t in zip(KEYS, w)}, T).numpy()
    none = bf16_torch.segment_classifier(fam.X, fam.src, fam.dst, w, T, xp, rounding="none").numpy()
    assert np.abs(none - ref).max() < 1e-12
    rne = bf16_torch.segment_classifier(fam.X, fam.src, fam.dst, w, T, xp).numpy()
    d = float(np.abs(rne - ref).max())
    assert 1e-6 < d < TOL_BF16, d


def _orders(E, dst):
    return {"caller": np.arange(E), "by_dst": np.argsort(dst, kind="stable"),
            **{"random%d" % s: np.random.default_rng(s).permutation(E) for s in range(3)}}


def bf16_floor(case):
    """(worst max, worst mean) of |fp32-accumulated emulation - fp64-accumulated emulation| over five segment orders."""
    fam = fp64_graphs.family(case[0], case[1])
    _, w = g.model(case)
    ref = bf16_torch.segment_classifier(fam.X, fam.src, fam.dst, w, case[3], case[4]).numpy()
    mx = mn = 0.0
    for o in _orders(fam.src.shape[0], fam.dst).values():
        e = bf16_torch.segment_classifier(fam.X, fam.src, fam.dst, w, case[3], case[4], accum="fp32", order=o).numpy()
        mx, mn = max(mx, float(np.abs(e - ref).max())), max(mn, float(np.abs(e - ref).mean()))
    return mx, mn


def test_every_gpu_case_has_a_bound():
    assert sorted(g.BF16_BOUNDS, key=str) == sorted(g.CASES, key=str)


@pytest.mark.parametrize("case", g.CASES, ids=g.case_id)
def test_bf16_bounds_are_backed_by_the_floor(case):
    """B_max / B_mean of the case: above the GPU error measured, at most 2.5 x it and at most 2.5 x the floor."""
    B_max, B_mean, gpu = g.BF16_BOUNDS[case]
    fmax, fmean = bf16_floor(case)
    assert gpu[0] < B_max <= 2.5 * min(gpu[0], fmax) * 1.0001, (B_max, gpu, fmax)
    assert gpu[1] < B_mean <= 2.5 * min(gpu[1], fmean) * 1.0001, (B_mean, gpu, fmean)
