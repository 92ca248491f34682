"""Which kernels the backward launches, case by case: the smallest batches that reach every branch of the route
decision (choose_bwd_route in csrc/backward.hip), the per-module entry points, the one-launch backward, and the one
size at which a launcher's arithmetic differs (k_edge_bwd's grid clamp at 1024 workgroups).

    python tools/record_backward_routes.py                 # writes tests/data/backward_routes.json
    python tools/record_backward_routes.py --hash          # also prints a SHA-256 of each case's gradient bytes
    python tools/record_backward_routes.py --case NAME     # that case alone; its entry of the JSON is replaced

The JSON holds, per case, the ordered kernel names `_lib.profile` reports for the backward call.  It is recorded at
the commit BEFORE a change to the host side of the backward; tests/test_gpu_backward_route.py replays the cases
(`run_case`) on the current build.  A library that reads GNN_BWD_NO_FIN_HIT once per process (every commit before
read_bwd_switches) cannot have that switch flipped between cases: there, record the whole list first and then the
GNN_BWD_NO_FIN_HIT case again in a process of its own with `--case`, which sets the variable before the first
backward.  The hashes are for comparing two builds on one machine and are not kept: kernel work may change them.
What the cases compute is checked by tests/test_gpu_route_values.py, which takes a case's inputs from `build_inputs`
and runs it through `run_inputs` under an upstream gradient of its own, against float64."""
import argparse
import contextlib
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "tests", "data", "backward_routes.json")

SWITCHES = ("GNN_BWD_WIDE_PER_PASS", "GNN_BWD_NO_FIN_HIT")


def _case(name, F, D, T, q=True, env=None, kind="segclf"):
    return dict(name=name, F=F, D=D, T=T, q=q, env=env, kind=kind)


CASES = [
    _case("3x8 T=3 Q", 3, 8, 3),
    _case("3x8 T=3 Q GNN_BWD_NO_FIN_HIT", 3, 8, 3, env="GNN_BWD_NO_FIN_HIT"),
    _case("3x8 T=1 Q", 3, 8, 1),
    _case("3x8 T=0", 3, 8, 0),
    _case("3x8 T=2 no Q", 3, 8, 2, q=False),
    _case("11x16 T=2 Q", 11, 16, 2),
    _case("3x32 T=2 Q", 3, 32, 2),
    _case("3x32 T=2 Q GNN_BWD_WIDE_PER_PASS", 3, 32, 2, env="GNN_BWD_WIDE_PER_PASS"),
    _case("3x32 T=2 no Q", 3, 32, 2, q=False),
    _case("3x32 T=0 Q", 3, 32, 0),
    _case("3x64 T=1 Q", 3, 64, 1),
    _case("nodeclf 3x8 T=2 Q", 3, 8, 2, kind="nodeclf"),
    _case("nodeclf 3x8 T=2 no Q", 3, 8, 2, q=False, kind="nodeclf"),
    _case("nodeclf 3x64 T=2 Q", 3, 64, 2, kind="nodeclf"),
    _case("nodeclf 3x64 T=2 no Q", 3, 64, 2, q=False, kind="nodeclf"),
    _case("edge_bwd 3x8", 3, 8, 1, kind="edge"),
    _case("node_bwd 3x8", 3, 8, 1, kind="node"),
    _case("one launch 3x8 T=2", 3, 8, 2, kind="events"),
    _case("3x8 T=1 Q over 262144 segments", 3, 8, 1, kind="big"),
]


@contextlib.contextmanager
def switch(name):
    """The backward's switches off, except `name`; the caller's environment comes back afterwards."""
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


def batch_host(case):
    """The case's batch on the host, every 13th segment padded (src = dst = -1)."""
    from gnn_fpga_amd import HitGraphBatch, synth
    F = case["F"]
    if case["kind"] == "events":
        graphs = [synth.layered_graph(40, 150, F, n_layers=5, seed=80 + i) for i in range(3)]
    elif case["kind"] == "big":
        graphs = [synth.layered_graph(30000, 270000, F, seed=90)]
    else:
        graphs = [synth.layered_graph(900, 6000, F, seed=70), synth.layered_graph(9, 11, F, n_layers=3, seed=71)]
    b = HitGraphBatch.from_graphs(graphs)
    src, dst = b.src.numpy().copy(), b.dst.numpy().copy()
    src[7::13] = -1
    dst[7::13] = -1
    return HitGraphBatch(b.X.numpy(), src, dst, hit_ptr=b.hit_ptr, seg_ptr=b.seg_ptr)


def host_weights(case):
    """The case's ten weight tensors on the host, state_dict order: SegmentClassifier's default init from the case's
    seed (which also seeds the device generator the head and the default upstream gradients are drawn from)."""
    import torch
    from gnn_fpga_amd.model import SegmentClassifier
    torch.manual_seed(5 * case["D"] + case["T"])
    model = SegmentClassifier(input_dim=case["F"], hidden_dim=case["D"], n_iters=case["T"])
    return [t.detach().contiguous() for t in model.state_dict().values()]


def build_inputs(case, head=None):
    """The case's inputs on the device, as a namespace: batch `b`, weights `w`, the head (`Wo`, `bo`: nodeclf only;
    `head` = (Wo, bo) replaces the seeded one), the event layout `lay` (events only), the kept forward tensors
    `e_all`, `H_all`, `Q_all` (and `y`: nodeclf), and `grad`, the default upstream gradient: randn / count."""
    import types

    import torch
    from gnn_fpga_amd import _lib
    F, D, T, kind = case["F"], case["D"], case["T"], case["kind"]
    w = [t.cuda() for t in host_weights(case)]
    b = batch_host(case).cuda()
    N, E = b.n_hits, b.n_segments
    inp = types.SimpleNamespace(case=case, b=b, w=w, Wo=None, bo=None, lay=None, y=None, Q_all=None)
    if kind == "nodeclf":
        inp.Wo, inp.bo = 0.3 * torch.randn(1, F + D, device="cuda"), torch.randn(1, device="cuda")
        if head is not None:
            inp.Wo, inp.bo = (t.to("cuda", torch.float32) for t in head)
        inp.e_all, inp.H_all, inp.Q_all, inp.y = _lib.nodeclf_forward_train(b, w, inp.Wo, inp.bo, F, D, T, keep_q=case["q"])
        inp.grad = torch.randn(N, device="cuda") / N
    elif kind == "events":
        inp.lay = b.event_layout()
        assert inp.lay is not None and _lib.events_backward_supported(F, D, inp.lay.max_hits, inp.lay.max_segments)
        inp.e_all, inp.H_all, _ = _lib.segclf_forward_train(b, w, F, D, T, layout=inp.lay)
        inp.grad = torch.randn(E, device="cuda") / E
    else:
        inp.e_all, inp.H_all, Q_all = _lib.segclf_forward_train(b, w, F, D, T)
        inp.Q_all = Q_all if case["q"] else None
        inp.grad = torch.randn(E, device="cuda") / E
        if kind == "node":
            inp.grad = torch.randn_like(inp.H_all[1]) / N
    return inp


def run_inputs(inp, grad=None, into=None):
    """One backward of the case on `inp` (build_inputs), with the environment as the caller left it.  `grad`: the
    upstream gradient instead of the default one - of e_T [E] (segclf, big, events), of e [E] (edge), of H' (node:
    rows of H_all's stride, the first D columns used), of y [N] (nodeclf).  `into` (segclf, big, events): ten
    tensors the gradients are added into.  Returns the gradient tensors: the ten weights' (segclf, big, events; and
    gWo, gbo after them: nodeclf), gH and gW1, gb1, gW2, gb2 (edge), gH, ge and gW3, gb3, gW4, gb4 (node)."""
    from gnn_fpga_amd import _lib
    case, b, w = inp.case, inp.b, inp.w
    F, D, T, kind = case["F"], case["D"], case["T"], case["kind"]
    go = inp.grad if grad is None else grad
    e_all, H_all = inp.e_all, inp.H_all
    assert into is None or kind in ("segclf", "big", "events")
    if kind == "nodeclf":
        grads, gWo, gbo = _lib.nodeclf_backward(b, w, inp.Wo, inp.bo, F, D, T, e_all, H_all, inp.y, go, Q_all=inp.Q_all)
        return list(grads) + [gWo, gbo]
    if kind == "events":
        return list(_lib.segclf_backward_events(b, inp.lay, w, F, D, T, e_all, H_all, go, into=into))
    if kind == "edge":
        gH, grads = _lib.edge_bwd(H_all[0], b, w, F, D, e_all[0], go)
        return [gH] + list(grads)
    if kind == "node":
        gH, ge, grads = _lib.node_bwd(H_all[0], e_all[0], H_all[1], b, w, F, D, go)
        return [gH, ge] + list(grads)
    return list(_lib.segclf_backward(b, w, F, D, T, e_all, H_all, go, into=into, Q_all=inp.Q_all))


def run_case(case):
    """Runs the case's backward twice on one saved forward, with the environment as the caller left it.  Returns
    (kernel names of the first run, gradient tensors of the first run, of the second)."""
    import torch
    from gnn_fpga_amd import _lib
    inp = build_inputs(case)
    with _lib.profile(64) as prof:
        first = [t.clone() for t in run_inputs(inp)]
    second = [t.clone() for t in run_inputs(inp)]
    torch.cuda.synchronize()
    return [k for k, _ in prof.records], first, second


def gradient_hash(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--hash", action="store_true", help="print a SHA-256 of every case's gradient bytes")
    ap.add_argument("--case", help="run this case alone and replace its entry of the JSON")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    routes = {}
    if args.case:
        with open(args.out) as f:
            routes = json.load(f)
    cases = [c for c in CASES if args.case in (None, c["name"])]
    if not cases:
        ap.error("no case named %r" % args.case)
    for case in cases:
        with switch(case["env"]):
            names, first, _ = run_case(case)
        routes[case["name"]] = names
        line = "%-36s %s" % (case["name"], " ".join(names))
        if args.hash:
            line = "%s  %s" % (gradient_hash(first), line)
        print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(routes, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
