"""The kernels one plan build launches, case by case (tools/record_plan_build_launches.py: both forms of stage 1, both
list forms of the graph-local one, both level kernels of the global one, the FAST_MISS retry, the debug copies): the
names `_lib.profile` reports must equal those recorded in tests/data/plan_build_launches.json - written by that tool at
the commit before the builder's host side was gathered into a form decision and one launcher per stage
(csrc/plan_build.hip, plan_hip.py).  What the launched kernels build is compared array for array with the numpy
specification in tests/test_plan_hip.py."""
import importlib.util
import json
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location("record_plan_build_launches",
                                                  os.path.join(REPO, "tools", "record_plan_build_launches.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


recorder = _recorder()
with open(recorder.OUT) as f:
    RECORDED = json.load(f)

# what each case must show, beyond equal lists: (graph_local, list_mode, names that occur, names that do not)
SHOWS = {
    "layered graph-local": (True, 1, ["pb_graph_levels", "pb_graph_lists"], ["pb_degrees"]),
    "layered graph-local GNN_PLAN_SCATTER_LISTS": (True, 0, ["pb_graph_levels", "pb_sort_lists"], ["pb_degrees"]),
    "layered global": (False, 0, ["pb_levels_small"], ["pb_level_sweep", "pb_graph_levels"]),
    "shuffled global": (False, 0, ["pb_level_sweep", "pb_widen"], ["pb_levels_small", "pb_graph_levels"]),
    "cyclic default": (False, 0, ["pb_graph_levels", "pb_degrees"], []),
    "layered graph-local debug": (True, 1, ["pb_graph_levels"], ["pb_degrees"]),
}


def test_the_cases_are_the_recorded_ones():
    assert [c["name"] for c in recorder.CASES] == list(RECORDED) == list(SHOWS)


def test_the_record_shows_what_each_case_is_there_for():
    for name, (_, _, present, absent) in SHOWS.items():
        assert all(k in RECORDED[name] for k in present), name
        assert not any(k in RECORDED[name] for k in absent), name
    # FAST_MISS: the graph-local attempt runs to its sizes, then the global build follows in the same record
    cyc = RECORDED["cyclic default"]
    assert cyc.count("pb_sizes") == 2 and cyc.index("pb_graph_levels") < cyc.index("pb_sizes") < cyc.index("pb_degrees")
    # the three copies debug=True adds to the fill
    plain, dbg = RECORDED["layered graph-local"], RECORDED["layered graph-local debug"]
    assert dbg == plain + ["pb_copy_i32"] * 3


@pytest.mark.gpu
@pytest.mark.parametrize("case", recorder.CASES, ids=[c["name"].replace(" ", "_") for c in recorder.CASES])
def test_launched_kernels_are_the_recorded_ones(hip, case, monkeypatch):
    for k in recorder.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    names, plan = recorder.run_case(case)
    assert names == RECORDED[case["name"]]
    local, list_mode = SHOWS[case["name"]][:2]
    assert (plan.graph_local, plan.list_mode) == (local, list_mode)
