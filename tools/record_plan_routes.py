"""Which kernels the fused forward launches for a planned batch, case by case: the smallest batches that reach every
branch of the route decision (choose_route in csrc/sell_pipeline.hip).

    python tools/record_plan_routes.py            # writes tests/data/plan_routes.json
    python tools/record_plan_routes.py --hash     # also prints a SHA-256 of each case's score bytes

The JSON holds, per case, the ordered kernel names `_lib.profile` reports.  It is recorded at the commit BEFORE a
change to the host side of the pipeline; tests/test_gpu_plan_route.py replays the cases (`run_case`) on the current
build.  The hashes are for comparing two builds on one machine and are not kept: kernel work may change them.
What the cases compute is checked by tests/test_gpu_route_values.py, which takes a case's inputs from `build_inputs`,
runs it through `run_inputs` and compares the scores with float64."""
import argparse
import contextlib
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "tests", "data", "plan_routes.json")

SWITCHES = ("GNN_NO_ITER2", "GNN_NO_FUSE_FIRST", "GNN_NO_WIDE_EXACT", "GNN_WIDE_LOCKSTEP", "GNN_WIDE_ROLES")


def _case(name, F, D, T=3, env=None, xp=True, bf16=False, limits=None, big=False, train=False):
    return dict(name=name, F=F, D=D, T=T, env=env, xp=xp, bf16=bf16, limits=limits, big=big, train=train)


CASES = [
    _case("3x8", 3, 8),
    _case("3x8 GNN_NO_ITER2", 3, 8, env="GNN_NO_ITER2"),
    _case("3x8 GNN_NO_FUSE_FIRST", 3, 8, env="GNN_NO_FUSE_FIRST"),
    _case("3x8 one iteration", 3, 8, T=1),
    _case("3x8 no iteration", 3, 8, T=0),
    _case("3x8 plain exp", 3, 8, xp=False),
    _case("3x8 iter_records 0", 3, 8, limits={"iter_records": 0}),
    _case("2x8", 2, 8),
    _case("11x16", 11, 16),
    _case("3x16", 3, 16),
    _case("3x16 GNN_NO_WIDE_EXACT", 3, 16, env="GNN_NO_WIDE_EXACT"),
    _case("3x16 GNN_WIDE_ROLES", 3, 16, env="GNN_WIDE_ROLES"),
    _case("3x16 over 32768 padded hits", 3, 16, big=True),
    _case("3x32", 3, 32),
    _case("3x32 bf16", 3, 32, bf16=True),
    _case("3x64", 3, 64),
    _case("3x64 bf16", 3, 64, bf16=True),
    _case("3x8 training", 3, 8, train=True),
]


@contextlib.contextmanager
def _switch(name):
    """The route switches off, except `name`; the caller's environment comes back afterwards."""
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


def build_inputs(case):
    """The case's inputs on the device, as a namespace: the `graphs` it is made of (host), `batch`, `weights` (the
    model's ten effective tensors), `plan`, `flags`, and `twin` (the level-ordered batch: the training case only)."""
    import types

    import torch
    from gnn_fpga_amd import HitGraphBatch, _lib, synth
    from gnn_fpga_amd.model import SegmentClassifier
    F, D, T = case["F"], case["D"], case["T"]
    torch.manual_seed(3 * D + T)
    if case["big"]:
        graphs = [synth.layered_graph(33000, 200000, F, seed=70)]
    else:
        graphs = [synth.layered_graph(900, 6000, F, seed=70 + i) for i in range(3)]
        graphs.append(synth.layered_graph(5, 4, F, n_layers=2, seed=9))
    model = SegmentClassifier(input_dim=F, hidden_dim=D, n_iters=T).cuda().eval()
    weights = [t.detach().contiguous() for t in model.effective_weights()]
    batch = HitGraphBatch.from_graphs(graphs).cuda()
    plan = batch.build_plan(D, case["limits"])
    flags, twin = 0, None
    if case["train"]:
        twin = batch.level_ordered(D)
        assert twin._fused is plan
    else:
        if case["xp"]:
            assert _lib.exp_product_bound(weights, F, D, plan.x_absmax) <= 60.0
            flags |= _lib.GNN_FLAG_EXP_PRODUCT
        if case["bf16"]:
            flags |= _lib.GNN_FLAG_BF16_MLP
    return types.SimpleNamespace(case=case, graphs=graphs, batch=batch, weights=weights, plan=plan, flags=flags, twin=twin)


def run_inputs(inp):
    """The case's forward twice on `inp` (build_inputs), under the case's switch.  Returns (kernel names of the first
    run, scores of the first run, scores of the second), the scores in the caller's segment order."""
    import torch
    from gnn_fpga_amd import _lib
    case = inp.case
    F, D, T = case["F"], case["D"], case["T"]
    if case["train"]:
        run = lambda: _lib.segclf_forward_train_fused(inp.twin, inp.weights, F, D, T)[3]
    else:
        run = lambda: _lib.segclf_forward_plan(inp.plan, inp.weights, F, D, T, flags=inp.flags)
    with _switch(case["env"]):
        run()                                   # (a batch's one-time work - plan struct, counts - is not a launch)
        with _lib.profile(64) as prof:
            first = run().clone()
        second = run().clone()
    torch.cuda.synchronize()
    return [k for k, _ in prof.records], first, second


def run_case(case):
    """Runs the case's forward twice.  Returns (kernel names of the first run, scores of the first run, scores of
    the second, plan, flags)."""
    inp = build_inputs(case)
    names, first, second = run_inputs(inp)
    return names, first, second, inp.plan, inp.flags


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--hash", action="store_true", help="print a SHA-256 of every case's score bytes")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    routes = {}
    for case in CASES:
        names, first, _, _, _ = run_case(case)
        routes[case["name"]] = names
        line = "%-30s %s" % (case["name"], " ".join(names))
        if args.hash:
            line = "%s  %s" % (hashlib.sha256(first.cpu().numpy().tobytes()).hexdigest(), line)
        print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(routes, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
