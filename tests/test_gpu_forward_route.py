"""The kernels the per-pass forward launches, case by case (tools/record_forward_routes.py: the smallest batches on
either side of the 2048-hit edge, both classifiers, inference and training, the trace rows, the per-module entry points
and the one-launch forward): the names `_lib.profile` reports must equal those recorded in
tests/data/forward_routes.json - written by that tool at the commit before the route decision was gathered into
choose_fwd_route (csrc/gnn_kernels.hip) - and must be the sequence `_kernels_of` derives from the entry point, the
shape, the iteration count, the hit count, the head, the trace rows and the switch; two runs of a case give the same
bits, the traced scores are the last trace row's, and the scores are the references' within the bounds of
test_gpu_parity.py and test_gpu_node_classifier.py.  The switch is flipped inside this one process: read_fwd_switches
reads it once per library call.  `_kernels_of` lives in tests/route_cases.py."""
import functools

import numpy as np
import pytest
import torch

import nodeclf_fp64
from oracle import index_c, index_torch
from oracle.dense_torch import KEYS
from route_cases import RECORDED_PASS as RECORDED, fwd_pass as recorder, pass_kernels_of as _kernels_of

TOL = 1e-5          # tests/test_gpu_parity.py: edge scores against the CPU reference
TOL_H = 2e-5        # tests/test_gpu_parity.py: hit features of the sub-modules
TOL_Y = 1e-5        # tests/test_gpu_node_classifier.py: hit scores against float64


def test_the_cases_are_the_recorded_ones():
    assert [c["name"] for c in recorder.CASES] == list(RECORDED)


def test_the_derived_kernels_are_the_recorded_ones():
    for case in recorder.CASES:
        assert _kernels_of(case) == RECORDED[case["name"]], case["name"]


@functools.lru_cache(maxsize=None)
def _reference(head, F, D, T, size):
    """Scores of the case's model on its batch, computed once per (classifier, shape, T, batch) and left unchanged:
    the C oracle's segment scores over the valid segments, or float64 hit scores."""
    case = dict(F=F, D=D, T=T, size=size)
    b = recorder.batch_host(case)
    X, src, dst = b.X.numpy(), b.src.numpy(), b.dst.numpy()
    w, Wo, bo = recorder.host_weights(case)
    if head:
        params = dict(zip(nodeclf_fp64.KEYS, [t.numpy() for t in w] + [Wo.numpy(), bo.numpy()]))
        return nodeclf_fp64.forward(X, src, dst, params, T)[0]
    valid = src >= 0
    return index_c.segment_classifier(X, src[valid], dst[valid], dict(zip(KEYS, [t.numpy() for t in w])), T)


def _check_module(case, out):
    """A per-module entry point against oracle.index_torch in float64 on the tensors the call was given."""
    F, D, kind = case["F"], case["D"], case["kind"]
    C = F + D
    inp = recorder.build_inputs(case)
    b = inp.b
    src, dst = b.src.cpu().numpy(), b.dst.cpu().numpy()
    p = {k: t.double().cpu() for k, t in zip(KEYS, inp.w)}
    got = out.double().cpu()
    with torch.no_grad():
        if kind == "input":
            trace = {}
            index_torch.segment_classifier(b.X.cpu().numpy(), src, dst, p, 0, trace=trace)
            assert (got[:, :C] - trace["H"][0]).abs().max().item() < TOL_H
            assert not got[:, C:].any()
        elif kind == "edge":
            ref = index_torch.edge_network(inp.H.double().cpu()[:, :C], src, dst, p)
            assert (got - ref).abs().max().item() < TOL
        else:
            H = inp.H.double().cpu()
            ref = index_torch.node_network(H[:, :C], inp.e.double().cpu(), src, dst, p)
            assert (got[:, :D] - ref).abs().max().item() < TOL_H
            assert torch.equal(got[:, D:C], H[:, D:C]) and not got[:, C:].any()


@pytest.mark.gpu
@pytest.mark.parametrize("case", recorder.CASES, ids=[c["name"].replace(" ", "_") for c in recorder.CASES])
def test_launched_kernels_are_the_recorded_and_the_derived_ones(hip, case, monkeypatch):
    for k in recorder.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if case["env"]:
        monkeypatch.setenv(case["env"], "1")
    names, first, second = recorder.run_case(case)
    assert names == RECORDED[case["name"]]
    assert names == _kernels_of(case)
    assert len(first) == len(second) >= 1
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    kind, T = case["kind"], case["T"]
    if case["trace"] and kind == "segclf":
        assert torch.equal(first[0], first[1][T])             # the final-score copy: not a kernel, so no name shows it
    if kind in ("input", "edge", "node"):
        return _check_module(case, first[0])
    head = kind in ("nodeclf", "nodeclf_train")
    ref = _reference(head, case["F"], case["D"], T, case["size"])
    if head:
        y = first[-1] if kind == "nodeclf_train" else first[0]
        assert np.abs(y.cpu().numpy() - ref).max() < TOL_Y
    else:
        e = first[0][T] if kind in ("train", "events_train") else first[0]
        valid = recorder.batch_host(case).src.numpy() >= 0
        assert np.abs(e.cpu().numpy()[valid] - ref).max() < TOL
