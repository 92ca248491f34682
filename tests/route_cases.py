"""The route cases of tools/record_backward_routes.py, tools/record_plan_routes.py and tools/record_forward_routes.py with
what a value check needs (test infrastructure, not product; shared by test_gpu_backward_route.py, test_gpu_plan_route.py,
test_gpu_forward_route.py, test_gpu_route_values.py and test_route_values_host.py):

  the kernels    `kernels_of` / `plan_kernels_of` / `pass_kernels_of`: the launches of a case, derived from its shape,
                 iteration count, kept hidden layers, head and switch; `route_of`: what choose_bwd_route
                 (csrc/backward.hip) returns for it, restated
  the matrix     `matrix_cases()`: beyond the 19 recorded backward cases, every shape the library supports at T = 2
                 with the kept hidden layers, T = 2 without them and T = 0 on the per-pass entry point, every shape
                 the one-launch backward accepts at T = 2, and the seeded head without k_fin_hit - on the recorder's
                 batch (900 + 9 hits, 6011 segments, every 13th padded: ragged lists, hits without segments, a graph
                 below one slice).  They are not in the JSON: their kernel names come from `kernels_of` alone
  the gradients  `upstream`: seeded, positive, 0.5 + U[0, 1) per element (times UPSTREAM_SCALE) and NOT divided by the
                 element count, drawn on the CPU generator so that the reference and the GPU run share the values.
                 With randn / E the largest entry of a gradient tensor is 2e-6 ... 4e-5 and golden_util.GRAD_ABS is up
                 to 5e-3 of it; with this one every tensor's largest entry is >= MIN_SCALE (test_route_values_host.py)
                 and the absolute floor is below 4 % of GRAD_REL * scale
  the truth      `reference`: float64 on the CPU - autograd through oracle.index_torch (segclf, big, events; edge and
                 node on given H_0, e_0) or tests/nodeclf_fp64.py (nodeclf) of sum(upstream * output); `dtype` and
                 `order` give the float32 oracle over other segment orders, `drop` the reference without one segment
"""
import functools
import importlib.util
import json
import os

import numpy as np
import torch

import nodeclf_fp64
from oracle import index_torch
from oracle.dense_torch import KEYS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _json(name):
    with open(os.path.join(REPO, "tests", "data", name)) as f:
        return json.load(f)


bwd = _tool("record_backward_routes")
fwd = _tool("record_plan_routes")
fwd_pass = _tool("record_forward_routes")
RECORDED_BWD = _json("backward_routes.json")
RECORDED_FWD = _json("plan_routes.json")
RECORDED_PASS = _json("forward_routes.json")

MIN_SCALE = 0.05        # every gradient tensor's max|fp64 reference| under `upstream`, unless it is identically zero
# The events batch has 450 segments against the others' 6011: a thirteenth of the terms in every sum.  Unscaled, the
# fp64 reference's smallest max|gradient| over its shapes is 0.016 ((11, 4): the input bias); times 16 (a power of
# two: exact in float32) the reference alone meets MIN_SCALE there as it does everywhere else
UPSTREAM_SCALE = {"events": 16.0}

# ---- the kernels of a case ----------------------------------------------------------------------------------------
EDGE_PASS = ["kb_pq", "k_edge_bwd", "k_pq_bwd"]
WIDE = ["k_hit_bwdW", "k_seg_bwdW", "k_seg_finW"]
FOLD = ["k_grad_fold", "k_grad_fold"]


def kernels_of(case):
    """The launches of a backward case with hits and segments, in order, under the names the profiler gives them."""
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


def route_triple(D, T, q, head, env):
    """(BwdStart, BwdIter, fuse_fin_hit) as choose_bwd_route returns them.  `q`: the caller passes kept hidden layers
    (the binding drops an empty Q_all: at T = 0 there are none); `head`: the NodeClassifier's, which has no grad_out."""
    q = q and T > 0
    if D <= 16:
        it = "quad" if q else "one_lane"
    else:
        it = "wide" if q and env != "GNN_BWD_WIDE_PER_PASS" else "per_pass"
    start = "seeded_head" if head else "wide_final_pass" if it == "wide" and T > 0 else "edge_pass"
    return start, it, it == "quad" and env != "GNN_BWD_NO_FIN_HIT"


def route_of(case):
    """The case's route triple; None for the entry points that do not go through choose_bwd_route."""
    if case["kind"] not in ("segclf", "big", "nodeclf"):
        return None
    return route_triple(case["D"], case["T"], case["q"], case["kind"] == "nodeclf", case["env"])


def reachable_routes():
    """Every triple choose_bwd_route can return, from its inputs: D <= 16 or D >= 32 (no shape lies between), T = 0 or
    not, kept hidden layers or not, head or not, each switch."""
    return {route_triple(D, T, q, head, env) for D in (16, 32) for T in (0, 2) for q in (False, True)
            for head in (False, True) for env in (None,) + tuple(bwd.SWITCHES)}


def plan_kernels_of(route, n_iters, n_pad, n_segments, training):
    """The launches of a fused-forward route (_lib.plan_route), in order, under the names the profiler gives them."""
    names = ["k_pack16"] if route["records"] == "bf16" else []
    names += ["k_pack"] if route["pack"] else []
    names += ["k_pack32"] if route["records"] == "exact" else []
    if n_pad > 0:
        names += ["k_input4"] if route["input"] else []              # (k_input4_bf / k_input4_x: profiled as k_input4)
        names += [route["family"]] * n_iters
    names += ["k_edge"] if n_segments > 0 else []                    # (k_edge_w: profiled as k_edge)
    names += ["k_edge_tw"] if training and n_segments > 0 else []
    return names


NODE_WIDE_MIN_HITS = 2048     # kNodeWideMinHits (csrc/gnn_kernels.hip)


def pass_kernels_of(case):
    """The launches of a per-pass forward case with hits and segments, in order, under the names the profiler gives
    them: choose_fwd_route (csrc/gnn_kernels.hip) restated from the entry point, hidden_dim, iteration count, total
    hits, head, trace rows and switch."""
    kind, D, T = case["kind"], case["D"], case["T"]
    if kind in ("events", "events_train"):
        return ["k_event"]
    if kind in ("input", "edge", "node"):             # the module entry points: one lane per item at every size
        return {"input": ["k_input"], "edge": ["k_pq", "k_edge"], "node": ["k_node"]}[kind]
    n_hits = fwd_pass.SIZES[case["size"]][0] + 9
    head = kind in ("nodeclf", "nodeclf_train")
    wide = D >= 32 and case["env"] != "GNN_NODE_ONE_LANE"
    wide_node = wide and (head or n_hits >= NODE_WIDE_MIN_HITS)
    wide_input = wide and n_hits >= NODE_WIDE_MIN_HITS and not (head and T == 0)
    names = ["k_input"] + (["k_pq_mlpW"] if wide_input else [])
    for t in range(T + 1):
        names += ["k_unpad"] if case["trace"] else []
        if t == T and head:                           # the last node pass scored the hits: no final edge pass
            break
        names += ["k_edge"]
        if t < T:
            names += ["k_node_walkW", "k_node_mlpW"] if wide_node else ["k_node"]
    return names


# ---- the cases ----------------------------------------------------------------------------------------------------
HIDDEN_DIMS = (4, 8, 16, 32, 64)
INPUT_DIMS = range(1, 17)


def supported_shapes():
    """Every (F, D) in 1 <= F <= 16, D in HIDDEN_DIMS the library has kernels for (asked, not listed)."""
    from gnn_fpga_amd import _lib
    return [(F, D) for F in INPUT_DIMS for D in HIDDEN_DIMS if _lib.shape_supported(F, D)]


def event_shapes():
    """The shapes the one-launch backward accepts on the recorder's events batch."""
    from gnn_fpga_amd import _lib
    out = []
    for F, D in supported_shapes():
        b = host_batch(bwd._case("", F, D, 2, kind="events"))
        max_hits, max_segments = int(np.diff(b.hit_ptr).max()), int(np.diff(b.seg_ptr).max())
        if _lib.events_backward_supported(F, D, max_hits, max_segments):
            out.append((F, D))
    return out


def _what(c):
    return c["kind"], c["F"], c["D"], c["T"], bool(c["q"] and c["T"] > 0), c["env"]


@functools.lru_cache(maxsize=None)
def matrix_cases():
    """The shape matrix, less the cases the recorder already has (same entry point, shape, T, kept layers, no switch)."""
    cases = []
    for F, D in supported_shapes():
        cases.append(bwd._case("matrix %dx%d T=2 Q" % (F, D), F, D, 2))
        cases.append(bwd._case("matrix %dx%d T=2 no Q" % (F, D), F, D, 2, q=False))
        cases.append(bwd._case("matrix %dx%d T=0" % (F, D), F, D, 0, q=False))
    for F, D in event_shapes():
        cases.append(bwd._case("matrix one launch %dx%d T=2" % (F, D), F, D, 2, kind="events"))
    # the one triple no recorded case returns: the seeded head on the quad iterations without k_fin_hit
    cases.append(bwd._case("matrix nodeclf 3x8 T=2 Q GNN_BWD_NO_FIN_HIT", 3, 8, 2, env="GNN_BWD_NO_FIN_HIT", kind="nodeclf"))
    recorded = {_what(c) for c in bwd.CASES}
    return tuple(c for c in cases if _what(c) not in recorded)


def backward_cases():
    return list(bwd.CASES) + list(matrix_cases())


def case_id(case):
    return case["name"].replace(" ", "_")


# one quad case, one wide case and the one-launch case: the backward adds into ten caller-owned tensors
INTO_CASES = ["3x8 T=3 Q", "3x32 T=2 Q", "one launch 3x8 T=2"]


def case_named(name):
    return next(c for c in backward_cases() if c["name"] == name)


# ---- seeded inputs on the host ------------------------------------------------------------------------------------
def _batch_kind(case):
    return case["kind"] if case["kind"] in ("events", "big") else "default"


@functools.lru_cache(maxsize=None)
def _host_batch(kind, F):
    return bwd.batch_host(dict(kind=kind, F=F))


def host_batch(case):
    """The case's batch on the host (the recorder's): X, src, dst as its tensors."""
    return _host_batch(_batch_kind(case), case["F"])


@functools.lru_cache(maxsize=None)
def _host_weights(F, D, T):
    return tuple(bwd.host_weights(dict(F=F, D=D, T=T)))


def host_weights(case):
    return list(_host_weights(case["F"], case["D"], case["T"]))


def _seed(case, salt):
    return 100003 * salt + 1009 * case["F"] + 17 * case["D"] + case["T"]


def head(case):
    """The NodeClassifier's output network (Wo [1, C], bo [1]), float32 on the host: drawn like the recorder's, but on
    the CPU generator."""
    g = torch.Generator().manual_seed(_seed(case, 1))
    C = case["F"] + case["D"]
    return 0.3 * torch.randn(1, C, generator=g), torch.randn(1, generator=g)


def upstream(case):
    """The upstream gradient, float32 on the host: UPSTREAM_SCALE * (0.5 + U[0, 1)) per element of e_T (segclf, big, events), e (edge),
    the first D columns of H' (node) or y (nodeclf)."""
    b = host_batch(case)
    shape = {"edge": (b.n_segments,), "node": (b.n_hits, case["D"]), "nodeclf": (b.n_hits,)}.get(case["kind"], (b.n_segments,))
    g = torch.Generator().manual_seed(_seed(case, 2))
    return UPSTREAM_SCALE.get(case["kind"], 1.0) * (0.5 + torch.rand(shape, generator=g))


def prefill(case):
    """Seeded values of order 1 for the ten tensors an `into=` backward adds into (float32, host)."""
    g = torch.Generator().manual_seed(_seed(case, 3))
    return [torch.randn(w.shape, generator=g) for w in host_weights(case)]


def host_forward(case):
    """(H_0 [N, C], e_0 [E]) of the case's model in float64 on the host: the per-module cases' inputs where no GPU
    forward is at hand."""
    b = host_batch(case)
    p = {k: w.double() for k, w in zip(KEYS, host_weights(case))}
    trace = {}
    with torch.no_grad():
        index_torch.segment_classifier(b.X.numpy(), b.src.numpy(), b.dst.numpy(), p, case["T"], trace=trace)
    return trace["H"][0], trace["e"][0]


# ---- the references -----------------------------------------------------------------------------------------------
def _np(t, shape=None):
    return np.zeros(shape) if t is None else t.detach().double().numpy()


def reference(case, dtype=torch.float64, order=None, drop=None, H0=None, e0=None):
    """The tensors recorder.run_inputs returns for the case under `upstream`, as float64 arrays computed in `dtype` on
    the CPU (gH of the per-module cases as [N, C]).  `order`: a permutation of the segments the sums are taken in
    (per-segment results come back in the caller's order); `drop`: one segment left out (segclf, big, events);
    `H0`, `e0`: the forward's kept hit features [N, C] and scores [E] the edge / node case runs on (default: the
    float64 host forward's)."""
    kind, T = case["kind"], case["T"]
    b = host_batch(case)
    X, src, dst = b.X.numpy(), b.src.numpy().astype(np.int64), b.dst.numpy().astype(np.int64)
    go = upstream(case)
    E = src.shape[0]
    o = np.arange(E) if order is None else np.asarray(order)
    if drop is not None:
        assert kind in ("segclf", "big", "events")
        o = o[o != drop]
    assert o.shape[0] == E - (drop is not None)
    ot = torch.from_numpy(o)
    src, dst = src[o], dst[o]
    w = host_weights(case)
    if kind == "nodeclf":
        Wo, bo = head(case)
        params = dict(zip(nodeclf_fp64.KEYS, [t.numpy() for t in w] + [Wo.numpy(), bo.numpy()]))
        grads = nodeclf_fp64.upstream_step(X, src, dst, params, T, go.numpy(), dtype=dtype)
        return [grads[k] for k in nodeclf_fp64.KEYS]
    p = {k: t.to(dtype).clone().requires_grad_(True) for k, t in zip(KEYS, w)}
    if kind in ("edge", "node"):
        if H0 is None:
            H0, e0 = host_forward(case)
        H = torch.as_tensor(H0).to(dtype).clone().requires_grad_(True)
        if kind == "edge":
            e = index_torch.edge_network(H, src, dst, p)
            (e * go[ot].to(dtype)).sum().backward()
            return [_np(H.grad)] + [_np(p[k].grad) for k in KEYS[2:6]]
        er = torch.as_tensor(e0).to(dtype)[ot].clone().requires_grad_(True)
        Hn = index_torch.node_network(H, er, src, dst, p)
        (Hn * go.to(dtype)).sum().backward()
        ge = torch.zeros(E, dtype=torch.float64)
        ge[ot] = er.grad.double()
        return [_np(H.grad), ge.numpy()] + [_np(p[k].grad) for k in KEYS[6:10]]
    e = index_torch.segment_classifier(X, src, dst, p, T)
    (e * go[ot].to(dtype)).sum().backward()
    return [_np(p[k].grad, tuple(p[k].shape)) for k in KEYS]


def tensor_names(case):
    """Names of the tensors `reference` returns, for messages and GNN_TEST_RECORD."""
    if case["kind"] == "edge":
        return ["grad H"] + list(KEYS[2:6])
    if case["kind"] == "node":
        return ["grad H", "grad e"] + list(KEYS[6:10])
    if case["kind"] == "nodeclf":
        return list(nodeclf_fp64.KEYS)
    return list(KEYS)


def ref_key(case):
    """Cases with the same key share one reference: the route (kept hidden layers, switch) does not enter."""
    kind = "segclf" if case["kind"] in ("segclf", "big", "events") else case["kind"]
    return _batch_kind(case), kind, case["F"], case["D"], case["T"]


class Refs:
    """float64 references on the host forward's inputs, computed once per key and left unchanged."""

    def __init__(self):
        self._bwd = {}

    def backward(self, case):
        key = ref_key(case)
        if key not in self._bwd:
            self._bwd[key] = reference(case)
        return self._bwd[key]


REFS = Refs()       # one per process: the GPU file and the host file share it


def orders(case, n):
    """`n` segment orders of the case: the caller's, by end hit, then seeded permutations."""
    b = host_batch(case)
    E = b.n_segments
    out = [np.arange(E), np.argsort(b.dst.numpy(), kind="stable")]
    out += [np.random.default_rng(s).permutation(E) for s in range(max(0, n - 2))]
    return out[:n]


def rel_errors(got, ref):
    """Per tensor: max|got - ref| beyond golden_util.GRAD_ABS, over max|ref| (0 where the reference is all zero)."""
    from golden_util import GRAD_ABS
    out = []
    for g, r in zip(got, ref):
        scale = float(np.abs(r).max()) if r.size else 0.0
        err = float(np.abs(np.asarray(g, np.float64) - r).max()) if r.size else 0.0
        out.append(max(0.0, err - GRAD_ABS) / scale if scale else err)
    return out
