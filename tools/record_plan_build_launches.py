"""Which kernels one plan build (HipSellPlan: csrc/plan_build.hip through plan_hip.py) launches, case by case: the
batches of tests/test_plan_hip.py (case_batch) that reach both forms of stage 1, both list forms of the graph-local
one, both level kernels of the global one, the FAST_MISS retry and the debug copies of the fill.

    python tools/record_plan_build_launches.py            # writes tests/data/plan_build_launches.json

The JSON holds, per case, the ordered kernel names `_lib.profile` reports for one build after one warm-up build.  It is
recorded at the commit BEFORE a change to the host side of the builder; tests/test_gpu_plan_build_launches.py replays
the cases (`run_case`) on the current build.  Names cannot tell pb_graph_lists<true> from <false>, nor the LDS size of
pb_graph_levels' 4-byte keys from the 8-byte ones: what those arms compute is compared array for array in
tests/test_plan_hip.py (mu200_size, many_muon, c3)."""
import argparse
import contextlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(REPO, "tests", "data", "plan_build_launches.json")

SWITCHES = ("GNN_PLAN_GRAPH_LOCAL", "GNN_PLAN_SCATTER_LISTS")


def _case(name, batch, graph_local=None, env=None, debug=False):
    return dict(name=name, batch=batch, graph_local=graph_local, env=env, debug=debug)


CASES = [
    _case("layered graph-local", "layered", graph_local=True),
    _case("layered graph-local GNN_PLAN_SCATTER_LISTS", "layered", graph_local=True, env="GNN_PLAN_SCATTER_LISTS"),
    _case("layered global", "layered", graph_local=False),
    _case("shuffled global", "shuffled", graph_local=False),
    _case("cyclic default", "cyclic"),
    _case("layered graph-local debug", "layered", graph_local=True, debug=True),
]


@contextlib.contextmanager
def _switch(name):
    """The builder's switches off, except `name`; the caller's environment comes back afterwards."""
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    if name:
        os.environ[name] = "1"
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def run_case(case):
    """Builds the case's plan twice (the first build is the warm-up: one-time attribute calls are not launches).
    Returns (kernel names of the second build, the plan)."""
    import torch
    from gnn_fpga_amd import _lib
    from gnn_fpga_amd.plan_hip import HipSellPlan
    from test_plan_hip import case_batch
    b, F, D, lim_over = case_batch(case["batch"])
    lim = _lib.plan_limits(F, D)
    lim.update(lim_over)
    b = b.cuda()
    with _switch(case["env"]):
        HipSellPlan(b, lim, debug=case["debug"], graph_local=case["graph_local"])
        with _lib.profile(512) as prof:
            plan = HipSellPlan(b, lim, debug=case["debug"], graph_local=case["graph_local"])
    torch.cuda.synchronize()
    return [k for k, _ in prof.records], plan


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    launches = {}
    for case in CASES:
        names, plan = run_case(case)
        launches[case["name"]] = names
        print("%-44s local=%d lists=%d  %s" % (case["name"], plan.graph_local, plan.list_mode, " ".join(names)), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(launches, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
