"""The kernels the fused forward launches, case by case (tools/record_plan_routes.py: the smallest batches that reach
each branch of the route decision): the names `_lib.profile` reports must equal those recorded in
tests/data/plan_routes.json - written by that tool at the commit before the route decision was gathered into
choose_route (csrc/sell_pipeline.hip) - and must be what `_lib.plan_route` says for the case; two runs of a case give
the same bits."""
import importlib.util
import json
import os

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_plan_routes", os.path.join(REPO, "tools", "record_plan_routes.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)

with open(os.path.join(REPO, "tests", "data", "plan_routes.json")) as _f:
    RECORDED = json.load(_f)


def _kernels_of(route, n_iters, n_pad, n_segments, training):
    """The launches of a route, in order, under the names the profiler gives them."""
    names = ["k_pack16"] if route["records"] == "bf16" else []
    names += ["k_pack"] if route["pack"] else []
    names += ["k_pack32"] if route["records"] == "exact" else []
    if n_pad > 0:
        names += ["k_input4"] if route["input"] else []              # (k_input4_bf / k_input4_x: profiled as k_input4)
        names += [route["family"]] * n_iters
    names += ["k_edge"] if n_segments > 0 else []                    # (k_edge_w: profiled as k_edge)
    names += ["k_edge_tw"] if training and n_segments > 0 else []
    return names


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
