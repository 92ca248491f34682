"""The kernels the backward launches, case by case (tools/record_backward_routes.py: the smallest batches that reach
each branch of the route decision, the per-module entry points, the one-launch backward and k_edge_bwd's grid clamp):
the names `_lib.profile` reports must equal those recorded in tests/data/backward_routes.json - written by that tool at
the commit before the route decision was gathered into choose_bwd_route (csrc/backward.hip) - and must be the
sequence `_kernels_of` derives from the shape, the iteration count, the kept hidden layers, the head and the switch;
two runs of a case give the same bits.  The switches are flipped inside this one process: read_bwd_switches reads
them once per library call.  `_kernels_of` lives in tests/route_cases.py; what the launched kernels compute is checked
case by case against float64 in tests/test_gpu_route_values.py."""
import pytest
import torch

from route_cases import RECORDED_BWD as RECORDED, bwd as recorder, kernels_of as _kernels_of


def test_the_cases_are_the_recorded_ones():
    assert [c["name"] for c in recorder.CASES] == list(RECORDED)


def test_the_derived_kernels_are_the_recorded_ones():
    for case in recorder.CASES:
        assert _kernels_of(case) == RECORDED[case["name"]], case["name"]


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
    assert len(first) == len(second) >= 5
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert float(first[0].abs().max()) > 0
