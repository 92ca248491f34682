"""The kernels the backward launches, case by case (tools/record_backward_routes.py: the smallest batches that reach
each branch of the route decision, the per-module entry points, the one-launch backward and k_edge_bwd's grid clamp):
the names `_lib.profile` reports must equal those recorded in tests/data/backward_routes.json - written by that tool at
the commit before the route decision was gathered into choose_bwd_route (csrc/backward.hip) - and must be the
sequence `_kernels_of` derives from the shape, the iteration count, the kept hidden layers, the head and the switch;
two runs of a case give the same bits.  The switches are flipped inside this one process: read_bwd_switches reads
them once per library call."""
import importlib.util
import json
import os

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_backward_routes",
                                               os.path.join(REPO, "tools", "record_backward_routes.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)

with open(os.path.join(REPO, "tests", "data", "backward_routes.json")) as _f:
    RECORDED = json.load(_f)

EDGE_PASS = ["kb_pq", "k_edge_bwd", "k_pq_bwd"]
WIDE = ["k_hit_bwdW", "k_seg_bwdW", "k_seg_finW"]
FOLD = ["k_grad_fold", "k_grad_fold"]


def _kernels_of(case):
    """The launches of a case with hits and segments, in order, under the names the profiler gives them."""
    D, T, q, env, kind = case["D"], case["T"], case["q"] and case["T"] > 0, case["env"], case["kind"]
    if kind == "edge":
        return EDGE_PASS + FOLD
    if kind == "node":
        return ["k_node_bwd", "k_agg_bwd_n", "k_seg_grad"] + FOLD
    if kind == "events":
        return ["k_event_bwd"] + FOLD
    wide = D >= 32 and q and env != "GNN_BWD_WIDE_PER_PASS"
    if kind == "nodeclf":
        names = ["k_head_bwd", "k_head_fold", "k_head_fold"]
    elif wide:
        names = WIDE + ["k_edge_bwd"]                # the wide final pass; k_edge_bwd for the padded segments only
    else:
        names = list(EDGE_PASS)
    if D <= 16 and q:
        fused = env != "GNN_BWD_NO_FIN_HIT"
        for u in range(T, 0, -1):
            names += ["k_hit_bwd4"] if u == T or not fused else []
            names += ["k_seg_bwd4", "k_fin_hit" if u > 1 and fused else "k_seg_fin"]
    elif D <= 16:
        names += ["kb_prs", "k_hit_bwd", "k_seg_bwd"] * T
    elif wide:
        names += WIDE * T
    else:
        names += (["k_node_bwd", "k_agg_bwd_n"] + EDGE_PASS) * T
    return names + ["k_input_bwd"] + FOLD


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
