"""The kernels on batches past the 4 GiB record-table and 2^31-element marks, against fp64 references.

A wrapped or truncated offset does not fault: it reads a valid row of another hit.  Every batch here is built by
tests/big_graphs.py from copies of a pool of distinct odd-sized graphs in a seeded random order, and EVERY copy's
scores are compared with its own pool graph's reference (index_c in fp64; oracle.bf16_torch for the bf16 route).
The worst copy is reported with the plan rows it occupies.

  wide guard     choose_route (csrc/sell_pipeline.hip) picks the wide kernels (k_iter_w / k_iter_wx, 32-bit byte offsets
                 off a wave-uniform base) only while (n_pad + 2) * D * B < 2^32, B = 4 (bf16) or 8 (exact fp32).
                 Each shape runs once with n_pad within 1 MiB of rows below the guard and once within 1 MiB above
                 it, and asserts from the kernel names which route ran on each side.
  per-module     gnn_kernels.hip's H [N, ldh] past 2^31 elements (use_plan = False)
  training       H_all [(T + 1), N, ldh] past 2^31 elements on the caller's order and on the twin

Each case prints n_pad, the bytes of its largest table and its worst error; GNN_TEST_RECORD=<file> receives the
errors (tests/test_gpu_fp64_reference.py's format).
"""
import functools
import os

import numpy as np
import pytest
import torch

import big_graphs
from golden_util import GRAD_REL, assert_grad_close
from gnn_fpga_amd import HitGraphBatch, _lib
from oracle import bf16_torch, index_c, index_torch
from test_gpu_bf16_reference import BF16_BOUNDS

pytestmark = pytest.mark.gpu

TOL = 1e-5
LOSS_TOL = 1e-6


def _record(what, err, scale=1.0):
    rec = os.environ.get("GNN_TEST_RECORD")
    if rec:
        with open(rec, "a") as f:
            f.write("%s\t%.3e\t%.3e\t%.3e\n" % (what, err, scale, err / scale if scale else 0.0))


def _free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()


def _peaks():
    import resource
    return "device peak %.1f GB, host peak RSS %.1f GB" % (torch.cuda.max_memory_allocated() / 1e9,
                                                         resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1e6)


def _model(F, D, T, seed):
    from gnn_fpga_amd.model import SegmentClassifier
    torch.manual_seed(seed)
    m = SegmentClassifier(input_dim=F, hidden_dim=D, n_iters=T)
    params = {k: v.detach().double().clone() for k, v in m.state_dict().items()}
    return m, params


def _batch(t):
    return HitGraphBatch(t.X, t.src, t.dst, y=t.y, hit_ptr=t.hit_ptr, seg_ptr=t.seg_ptr).cuda()


def _plan_rows(b):
    """caller's hit id -> plan row (device int64)."""
    perm = b.plan.perm.to(torch.int64)
    new = torch.nonzero(perm >= 0).reshape(-1)
    rank = torch.empty(b.n_hits, dtype=torch.int64, device=perm.device)
    rank[perm[new]] = new
    return rank


def compare_copies(e, t, refs, rows=None):
    """|e - reference| of every copy of t against refs[pool graph] (fp64).  Returns (worst error, mean error,
    description of the worst copy: its index, pool graph, hits and the last plan row it occupies)."""
    assert bool(torch.isfinite(e).all()), "non-finite scores"
    sp = torch.from_numpy(t.seg_ptr).to(e.device)
    worst, worst_k, total, count = -1.0, -1, 0.0, 0
    for p in np.unique(t.copies):
        ks = np.flatnonzero(t.copies == p)
        ref = torch.from_numpy(np.asarray(refs[p], np.float64)).to(e.device)
        E_p = ref.shape[0]
        ar = torch.arange(E_p, device=e.device)
        for c0 in range(0, ks.shape[0], 64):
            kk = torch.from_numpy(ks[c0:c0 + 64]).to(e.device)
            idx = sp[kk][:, None] + ar[None, :]
            d = (e[idx].double() - ref[None, :]).abs()
            total += float(d.sum())
            count += d.numel()
            per = d.amax(dim=1)
            j = int(per.argmax())
            if float(per[j]) > worst:
                worst, worst_k = float(per[j]), int(ks[c0 + j])
    assert count == e.shape[0], (count, e.shape[0])
    h0, h1 = int(t.hit_ptr[worst_k]), int(t.hit_ptr[worst_k + 1])
    where = "copy %d of %d (pool graph %d, hits %d-%d" % (worst_k, len(t.copies), t.copies[worst_k], h0, h1 - 1)
    if rows is not None:
        where += ", plan rows up to %d" % int(rows[h0:h1].max())
    return worst, total / max(count, 1), where + ")"


class _Refs:
    def __init__(self):
        self.f64, self.emu = {}, {}

    def fp64(self, graphs, key, params, T):
        if key not in self.f64:
            p = {k: v.numpy() for k, v in params.items()}
            self.f64[key] = [index_c.segment_classifier(g.X, g.src, g.dst, p, T, f64=True).astype(np.float64)
                             for g in graphs]
        return self.f64[key]

    def bf16(self, graphs, key, weights, T, xp):
        if key not in self.emu:
            self.emu[key] = [bf16_torch.segment_classifier(g.X, g.src, g.dst, weights, T, xp).numpy()
                             for g in graphs]
        return self.emu[key]


@pytest.fixture(scope="module")
def refs():
    return _Refs()


@functools.lru_cache(maxsize=1)
def wide_batch(F, D, B, side):
    lo, hi = big_graphs.window(D, B, side)
    return big_graphs.tiled(F, _lib.plan_limits(F, D), lo, hi, "hi" if side == "below" else "lo")


def _run(hip, m, b, env=()):
    for k in ("GNN_WIDE_LOCKSTEP", "GNN_WIDE_ROLES"):
        os.environ.pop(k, None)
    try:
        for k in env:
            os.environ[k] = "1"
        with torch.no_grad(), hip.profile(512) as prof:
            e = m(b)
            torch.cuda.synchronize()
    finally:
        for k in env:
            os.environ.pop(k, None)
    return e, {k for k, _ in prof.records}


# (F, D, T, records): the wide shapes of the issue's table
WIDE = [(3, 64, 2, "exact"), (3, 32, 2, "exact"), (2, 16, 2, "exact"), (3, 64, 2, "bf16"), (3, 32, 2, "bf16")]


@pytest.mark.parametrize("side", ["below", "above"])
@pytest.mark.parametrize("case", WIDE, ids=lambda c: "F%d-D%d-T%d-%s" % c)
def test_wide_guard(hip, refs, case, side):
    """Below the 4 GiB guard the wide kernels run (k_pack32 / k_pack16 + k_iter_wx) and read the last rows under
    4 GiB right; above it the general fp32 k_iter runs (for a bf16 model too: no k_pack16, scores at TOL against
    fp64).  Every copy's scores against its pool graph's reference."""
    F, D, T, rec = case
    B = big_graphs.RECORD_BYTES[rec]
    lo, hi = big_graphs.window(D, B, side)
    t = wide_batch(F, D, B, side)
    m, params = _model(F, D, T, 300 + D + F)
    m = m.cuda().eval()
    m.use_plan, m.use_events, m.mlp_bf16 = True, False, rec == "bf16"
    b = _batch(t)
    e, names = _run(hip, m, b)
    n_pad = int(b.plan.n_pad)
    assert lo <= n_pad <= hi and n_pad == t.n_pad, (lo, n_pad, hi, t.n_pad)
    assert big_graphs.guard_ok(n_pad, D, B) == (side == "below")
    wide = {k for k in names if k.startswith("k_iter_w")}
    if side == "below":
        assert {"k_pack16" if rec == "bf16" else "k_pack32", "k_iter_wx"} <= names, sorted(names)
        assert wide == {"k_iter_wx"} and "k_iter" not in names, sorted(names)
    else:
        assert "k_iter" in names and not wide, sorted(names)
        assert "k_pack16" not in names and "k_pack32" not in names, sorted(names)
    rows = _plan_rows(b)
    xp = m._xp_cache[1] != 0
    if rec == "bf16" and side == "below":
        emu = refs.bf16(t.graphs, (case, side), [w.detach().cpu() for w in m.effective_weights()], T, xp)
        worst, mean, where = compare_copies(e, t, emu, rows)
        B_max, B_mean, _ = BF16_BOUNDS[("c3x4", F, D, T, xp, False)]
        bound = "bf16 emulation: max %.1e, mean %.1e" % (B_max, B_mean)
        ok = worst <= B_max and mean <= B_mean
    else:
        ref = refs.fp64(t.graphs, (case, side), params, T)
        worst, mean, where = compare_copies(e, t, ref, rows)
        bound = "fp64 at TOL"
        ok = worst < TOL
    table = (n_pad + 2) * D * B if side == "below" else (n_pad + 65) * 2 * D * 4
    tag = "index width %s %s: n_pad %d, record table %d bytes, kernels %s" % (
        "F%d-D%d-T%d-%s" % case, side, n_pad, table, sorted(k for k in names if k.startswith(("k_iter", "k_pack"))))
    print("\n%s; worst %.3e mean %.3e (%s) at %s; %s" % (tag, worst, mean, bound, where, _peaks()))
    _record(tag + " worst", worst)
    _record(tag + " mean", mean)
    assert ok, (tag, worst, mean, bound, where)
    if case == (3, 64, 2, "exact") and side == "below":
        # the lockstep twin: k_iter_w (round barriers) on the same batch, bit for bit the k_iter_wx result
        e2, names2 = _run(hip, m, b, env=("GNN_WIDE_LOCKSTEP",))
        assert {k for k in names2 if k.startswith("k_iter_w")} == {"k_iter_w"} and "k_pack32" in names2, sorted(names2)
        assert torch.equal(e, e2), float((e - e2).abs().max())
        print("lockstep twin (k_iter_w): bit-identical to k_iter_wx at n_pad %d" % n_pad)
    del e, b, m, rows
    _free()


def test_per_module_route_past_2_31_elements(hip, refs):
    """use_plan = False at (3, 64, 1) with N * ldh > 2^31: gnn_kernels.hip's H [N, ldh] (and PQ [N, 2D],
    M [N, 2 ldh] before it) past 2^31 elements, every copy against fp64."""
    F, D, T = 3, 64, 1
    ldh = _lib.h_stride(F, D)
    t = big_graphs.by_hits(F, (1 << 31) // ldh + 1)
    N = t.X.shape[0]
    assert N * ldh > 1 << 31
    m, params = _model(F, D, T, 310)
    m = m.cuda().eval()
    m.use_plan, m.use_events = False, False
    b = _batch(t)
    e, names = _run(hip, m, b)
    assert b.plan is None and not any(k.startswith("k_iter") for k in names), sorted(names)
    assert "k_node_walkW" in names and "k_node_mlpW" in names, sorted(names)
    worst, mean, where = compare_copies(e, t, refs.fp64(t.graphs, "modules", params, T))
    tag = "index width per-module F3-D64-T1: N %d, H %d elements (%d bytes), M %d elements" % (
        N, N * ldh, N * ldh * 4, N * 2 * ldh)
    print("\n%s; worst %.3e mean %.3e at %s; %s" % (tag, worst, mean, where, _peaks()))
    _record(tag + " worst", worst)
    assert worst < TOL, (tag, worst, where)
    del e, b, m
    _free()


@pytest.mark.parametrize("route", ["pass", "twin_pp"])
def test_training_past_2_31_elements_of_H_all(hip, route, monkeypatch):
    """A training step at (3, 64, 3) on identical copies of ONE odd-sized graph with (T + 1) * N * ldh > 2^31: the
    summed loss and every gradient are K x the single copy's fp64 ones (index_torch autograd), every copy's scores
    match the single-copy reference."""
    from gnn_fpga_amd.loss import BCELoss
    F, D, T = 3, 64, 3
    ldh = _lib.h_stride(F, D)
    g = big_graphs.pool(F)[0]
    t = big_graphs.repeated(g, (1 << 31) // ((T + 1) * ldh) + 1)
    K, N = len(t.copies), t.X.shape[0]
    assert (T + 1) * N * ldh > 1 << 31 and g.X.shape[0] % 2 == 1
    m, params = _model(F, D, T, 320)
    m = m.cuda().train()
    m.use_events = False
    m.level_order_training = route == "twin_pp"
    if route == "twin_pp":
        monkeypatch.setenv("GNN_NO_FUSED_TRAIN", "1")
    b = _batch(t)
    y = b.y.cuda()
    m.zero_grad()
    with hip.profile(2048) as prof:
        out = m(b)
        loss = BCELoss(reduction="sum")(out, y)
        loss.backward()
        torch.cuda.synchronize()
    names = {k for k, _ in prof.records}
    twin = getattr(b, "_twin", None)
    assert "k_seg_bwdW" in names and "k_edge_tw" not in names and "k_event_bwd" not in names, sorted(names)
    if route == "pass":
        assert twin is None
    else:
        assert twin is not None and twin is not b
    # fp64, one copy
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    e_ref = index_torch.segment_classifier(g.X, g.src, g.dst, p, T)
    l_ref = torch.nn.BCELoss(reduction="sum")(e_ref, torch.from_numpy(g.y).double())
    l_ref.backward()
    tag = "index width training F3-D64-T3 %s: %d copies, N %d, H_all %d elements" % (route, K, N, (T + 1) * N * ldh)
    worst, mean, where = compare_copies(out.detach(), t, [e_ref.detach().numpy()])
    print("\n%s; scores worst %.3e mean %.3e at %s; %s" % (tag, worst, mean, where, _peaks()))
    _record(tag + " scores", worst)
    assert worst < TOL, (tag, worst, where)
    err = abs(loss.item() - K * l_ref.item())
    _record(tag + " loss", err, K * abs(l_ref.item()))
    assert err < LOSS_TOL * max(1.0, K * abs(l_ref.item())), (tag, loss.item(), K * l_ref.item())
    for k, q in m.named_parameters():
        assert_grad_close(q.grad, K * p[k].grad, tag + " " + k, rel=GRAD_REL)
    del out, loss, b, m, y
    _free()

