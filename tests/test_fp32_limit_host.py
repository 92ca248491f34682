"""Backs the case-specific bounds of tests/test_gpu_fp64_reference.py (FP32_LIMIT) with numbers anyone can recompute
on a CPU: the fp32 oracle (oracle.index_torch in float32) of each listed case, run over five orders of the same
segments, against the fp64 reference.  Every bound must be at most 2.5 x the worst of those fp32 errors (the case
sits at the limit of fp32, not beyond it) and at most 2.5 x the GPU error it was measured from, and above that GPU
error."""
import numpy as np
import pytest
import torch

import fp64_graphs
import test_gpu_fp64_reference as g
from oracle import index_torch
from oracle.dense_torch import KEYS


def _orders(fam):
    E = fam.src.shape[0]
    return {"caller": np.arange(E), "by_dst": np.argsort(fam.dst, kind="stable"),
            **{"random%d" % s: np.random.default_rng(s).permutation(E) for s in range(3)}}


def fp32_worst(case):
    """(worst |score error|, worst gradient error / max|fp64| beyond GRAD_ABS) of the fp32 oracle over the orders."""
    from golden_util import GRAD_ABS
    fam_name, F, D, T, loss, masked, seed = case[:7]
    fam = fp64_graphs.family(fam_name, F)
    e64, _, g64 = g._Refs().training(case)
    _, params, masks = g._model(F, D, T, seed, masked)
    m32 = None if masks is None else {k: v.float() for k, v in masks.items()}
    ws = wg = 0.0
    for o in _orders(fam).values():
        p = {k: v.float().clone().requires_grad_(True) for k, v in params.items()}
        e = index_torch.segment_classifier(fam.X, fam.src[o], fam.dst[o], p, T, m32)
        g._loss_fn(loss, dev=False)(e, torch.from_numpy(fam.y[o])).backward()
        ws = max(ws, float(np.abs(e.detach().double().numpy() - e64[o]).max()))
        for k in KEYS:
            if p[k].grad is not None:
                err = float(np.abs(p[k].grad.double().numpy() - g64[k]).max())
                wg = max(wg, max(0.0, err - GRAD_ABS) / float(np.abs(g64[k]).max()))
    return ws, wg


_CASES = {tuple(c[:4]): c for c in g.TRAIN_CASES}


@pytest.mark.parametrize("case4", sorted({k[0] for k in g.FP32_LIMIT}))
def test_fp32_limit_bounds_are_backed_by_the_fp32_oracle(case4):
    ws, wg = fp32_worst(_CASES[case4])
    for (c, route), (tol, rel, gpu) in g.FP32_LIMIT.items():
        if c != case4:
            continue
        assert gpu is not None
        if tol is not None:
            assert gpu[0] < tol <= 2.5 * min(gpu[0], ws) * 1.0001, (route, tol, gpu, ws)
        if rel is not None:
            assert gpu[1] < rel <= 2.5 * min(gpu[1], wg) * 1.0001, (route, rel, gpu, wg)


@pytest.mark.parametrize("D,order", sorted(g.SUBMODULE_FP32_LIMIT))
def test_submodule_fp32_limit_bounds_are_backed_by_the_fp32_oracle(D, order):
    """grad e of the node network on the hubs graph: the fp32 oracle over the orders against fp64."""
    from golden_util import GRAD_ABS
    F = 3
    fam = fp64_graphs.hubs(F)
    _, params, _ = g._model(F, D, 1, 30 + D)
    H0, e0, wE, wN = g.submodule_inputs(fam, F + D, D)

    def grad_e(dtype, o):
        p = {k: v.to(dtype) for k, v in params.items()}
        er = e0[o].to(dtype).requires_grad_(True)
        (index_torch.node_network(H0.to(dtype), er, fam.src[o], fam.dst[o], p) * wN.to(dtype)).sum().backward()
        out = torch.empty(er.shape[0], dtype=torch.float64)
        out[torch.from_numpy(o)] = er.grad.double()
        return out.numpy()

    ref = grad_e(torch.float64, np.arange(fam.src.shape[0]))
    worst = max(max(0.0, float(np.abs(grad_e(torch.float32, o) - ref).max()) - GRAD_ABS) / float(np.abs(ref).max())
                for o in _orders(fam).values())
    for what, (rel, gpu) in g.SUBMODULE_FP32_LIMIT[(D, order)].items():
        assert gpu < rel <= 2.5 * min(gpu, worst) * 1.0001, (what, rel, gpu, worst)
