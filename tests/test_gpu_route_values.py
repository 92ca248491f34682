"""The values behind every route case, against float64 on the CPU (tests/route_cases.py).

tests/test_gpu_backward_route.py and tests/test_gpu_plan_route.py assert which kernels a case launches and that two
runs give the same bits; a launcher that hands a kernel the wrong row (H(u-2) for H(u-1)), the wrong `first` flag or
the wrong gradient buffer launches the same names and is just as reproducible.  Here every case is also computed:

  backward   the 19 recorded cases and the shape matrix - every supported shape at T = 2 with and without the kept
             hidden layers and at T = 0, every one-launch shape, the seeded head without k_fin_hit - run once under
             their switch inside _lib.profile, with a seeded positive upstream gradient of order 1 that is NOT BCE's
             (the public entry points take any).  Kernel names against `kernels_of` (and the JSON where recorded),
             every returned tensor against autograd through oracle.index_torch / nodeclf_fp64 in float64 with
             golden_util.assert_grad_close at the unchanged GRAD_REL / GRAD_ABS.  The per-module cases' references run
             on the GPU forward's kept H_0, e_0 cast to float64.  tests/test_route_values_host.py shows on the CPU that
             the absolute floor plays no part, that float32 itself meets the bound and that the bound sees one segment
  into=      a quad case, a wide case and the one-launch case add into ten seeded tensors of order 1: prefill + fp64
             gradient, bound relative to max|prefill + gradient|
  forward    the 18 fused-forward cases under their switch: names as the replay test asserts them, scores against
             oracle.index_c in float64 at TOL = 1e-5 (the training case's returned scores too).  The two bf16 cases
             get TOL_BF16 = 2e-3, the project's bound for that route against fp32 / fp64; their tight pin (a bf16-faithful
             fp64 reference) stays in tests/test_gpu_bf16_reference.py

GNN_TEST_RECORD=<file> receives every comparison's worst error and max|reference|.  Measured on MI355X: the largest
error / max|reference| over the 731 gradient comparisons is 4.7e-7 (GRAD_REL: 5e-6; float32 CPU oracle: 6.6e-7), the
largest score error 1.5e-7 on the fp32 cases and 3.1e-4 on the bf16 ones.  No case has a bound of its own.
"""
import os

import numpy as np
import pytest
import torch

import route_cases as rc
from golden_util import assert_grad_close
from oracle import index_c

pytestmark = pytest.mark.gpu

TOL = 1e-5          # edge scores, as in test_gpu_parity / test_gpu_fp64_reference
TOL_BF16 = 2e-3     # bf16 records and matrix-core operands (GNN_FLAG_BF16_MLP), as in test_gpu_parity

BWD_CASES = rc.backward_cases()


def _record(what, err, scale):
    rec = os.environ.get("GNN_TEST_RECORD")
    if rec:
        with open(rec, "a") as f:
            f.write("%s\t%.3e\t%.3e\t%.3e\n" % (what, err, scale, err / scale if scale else 0.0))


def _set_switch(monkeypatch, switches, name):
    for k in switches:
        monkeypatch.delenv(k, raising=False)
    if name:
        monkeypatch.setenv(name, "1")


def _device_grad(case, inp):
    """route_cases.upstream on the device, in the layout the entry point reads."""
    go = rc.upstream(case).cuda()
    if case["kind"] == "node":                      # rows of H_all's stride, the first D columns used
        full = torch.zeros_like(inp.H_all[1])
        full[:, :case["D"]] = go
        return full
    return go


def _run(hip, case, monkeypatch, into=None):
    _set_switch(monkeypatch, rc.bwd.SWITCHES, case["env"])
    inp = rc.bwd.build_inputs(case, head=rc.head(case) if case["kind"] == "nodeclf" else None)
    for a, b in zip(inp.w, rc.host_weights(case)):
        assert torch.equal(a.cpu(), b)              # the reference's weights are the run's
    grad = _device_grad(case, inp)
    with hip.profile(64) as prof:
        got = rc.bwd.run_inputs(inp, grad=grad, into=into)
        torch.cuda.synchronize()
    names = [k for k, _ in prof.records]
    assert names == rc.kernels_of(case), case["name"]
    if case["name"] in rc.RECORDED_BWD:
        assert names == rc.RECORDED_BWD[case["name"]]
    return inp, got


@pytest.mark.parametrize("case", BWD_CASES, ids=[rc.case_id(c) for c in BWD_CASES])
def test_backward_values_against_fp64(hip, case, monkeypatch):
    inp, got = _run(hip, case, monkeypatch)
    C = case["F"] + case["D"]
    if case["kind"] in ("edge", "node"):
        ref = rc.reference(case, H0=inp.H_all[0][:, :C].double().cpu(), e0=inp.e_all[0].double().cpu())
        got = [got[0][:, :C]] + list(got[1:])
    else:
        ref = rc.REFS.backward(case)
    names = rc.tensor_names(case)
    assert len(got) == len(ref) == len(names)
    for g, r, n in zip(got, ref, names):
        assert tuple(g.shape) == tuple(r.shape), (case["name"], n)
        assert_grad_close(g, r, "route values %s %s" % (case["name"], n))


@pytest.mark.parametrize("name", rc.INTO_CASES, ids=[n.replace(" ", "_") for n in rc.INTO_CASES])
def test_backward_adds_into_the_callers_tensors(hip, name, monkeypatch):
    case = rc.case_named(name)
    pre = rc.prefill(case)
    into = [t.cuda().clone() for t in pre]
    _, got = _run(hip, case, monkeypatch, into=into)
    ref = rc.REFS.backward(case)
    assert len(got) == 10
    for g, t, p, r, n in zip(got, into, pre, ref, rc.tensor_names(case)):
        assert g.data_ptr() == t.data_ptr()         # the caller's own tensors come back
        assert_grad_close(g, p.double().numpy() + r, "route values into= %s %s" % (name, n))


# ---- the fused forward --------------------------------------------------------------------------------------------
_fwd_refs = {}


def _forward_reference(inp):
    """index_c in float64 on the case's unpadded batch; one per (batch, shape, T), left unchanged."""
    from gnn_fpga_amd import HitGraphBatch
    case = inp.case
    key = (case["big"], case["F"], case["D"], case["T"])
    params = {k: w.cpu().numpy() for k, w in zip(rc.KEYS, inp.weights)}
    if key not in _fwd_refs:
        b = HitGraphBatch.from_graphs(inp.graphs)
        e = index_c.segment_classifier(b.X.numpy(), b.src.numpy(), b.dst.numpy(), params, case["T"], f64=True)
        _fwd_refs[key] = (params, e.astype(np.float64))
    kept, e = _fwd_refs[key]
    assert all(np.array_equal(kept[k], params[k]) for k in rc.KEYS)      # same seed, same weights
    return e


@pytest.mark.parametrize("case", rc.fwd.CASES, ids=[rc.case_id(c) for c in rc.fwd.CASES])
def test_forward_values_against_fp64(hip, case, monkeypatch):
    _set_switch(monkeypatch, rc.fwd.SWITCHES, None)
    inp = rc.fwd.build_inputs(case)
    names, first, _ = rc.fwd.run_inputs(inp)
    assert names == rc.RECORDED_FWD[case["name"]]
    _set_switch(monkeypatch, rc.fwd.SWITCHES, case["env"])
    route = hip.plan_route(inp.plan, case["F"], case["D"], case["T"], flags=inp.flags, training=case["train"])
    assert names == rc.plan_kernels_of(route, case["T"], inp.plan.n_pad, inp.plan.n_segments, case["train"]), route
    ref = _forward_reference(inp)
    got = first.double().cpu().numpy()
    assert got.shape == ref.shape
    err = float(np.abs(got - ref).max())
    _record("route values forward %s" % case["name"], err, float(np.abs(ref).max()))
    assert err < (TOL_BF16 if case["bf16"] else TOL), (case["name"], err)
