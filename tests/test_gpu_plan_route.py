"""The kernels the fused forward launches, case by case (tools/record_plan_routes.py: the smallest batches that reach
each branch of the route decision): the names `_lib.profile` reports must equal those recorded in
tests/data/plan_routes.json - written by that tool at the commit before the route decision was gathered into
choose_route (csrc/sell_pipeline.hip) - and must be what `_lib.plan_route` says for the case; two runs of a case give
the same bits.  `_kernels_of` lives in tests/route_cases.py (plan_kernels_of); the scores the launched kernels give are
checked case by case against float64 in tests/test_gpu_route_values.py."""
import pytest
import torch

from route_cases import RECORDED_FWD as RECORDED, fwd as recorder, plan_kernels_of as _kernels_of


def test_the_cases_are_the_recorded_ones():
    assert [c["name"] for c in recorder.CASES] == list(RECORDED)


@pytest.mark.gpu
@pytest.mark.parametrize("case", recorder.CASES, ids=[c["name"].replace(" ", "_") for c in recorder.CASES])
def test_launched_kernels_are_the_recorded_and_the_decided_ones(hip, case, monkeypatch):
    for k in recorder.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    names, first, second, plan, flags = recorder.run_case(case)
    assert names == RECORDED[case["name"]]
    assert torch.equal(first, second)
    if case["env"]:
        monkeypatch.setenv(case["env"], "1")
    route = hip.plan_route(plan, case["F"], case["D"], case["T"], flags=flags, training=case["train"])
    assert names == _kernels_of(route, case["T"], plan.n_pad, plan.n_segments, case["train"]), route
    if case["big"]:
        assert plan.n_pad >= 32768
    elif case["D"] >= 16:
        assert plan.n_pad < 32768
