"""What the toy MPNN tests share (test infrastructure, not product): synthetic graphs and default-init parameters, the
fp64 reference's own fp32 error, the printing checks against the project's bounds, and the SHAPE MATRIX - every
(input_dim, hidden_dim) pair csrc/iter_events.hip instantiates, with the two batches every shape is run on.

Imported by test_gpu_toy_mpnn.py (size edges), test_toy_mpnn_shapes_host.py (no GPU) and test_gpu_toy_mpnn_shapes.py.
Bounds (tests/toy_mpnn_fp64.py): scores and every stored e_t / H_t within SCORE_BOUND (1e-5 absolute) of fp64; the loss
and every gradient tensor separately within grad_bound(own) = max(4 x the reference's own fp32 error, 5e-6), relative
to the tensor's largest fp64 entry, `own` being `reference_error`'s largest of eight segment orders."""
import functools

import numpy as np
import torch
import torch.nn as nn

import toy_mpnn_fp64 as ref
from gnn_fpga_amd import HitGraphBatch, ToySegmentClassifier, ToySegmentClassifier2, synth


def model_of(params, F, D, T, shared, events=True):
    m = (ToySegmentClassifier2 if shared else ToySegmentClassifier)(F, D, T)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in params.items()})
    m.use_events = events
    return m.cuda()


def train_step(m, inp, y):
    """What the notebook's Estimator does per batch: (scores, loss, {name: grad})."""
    m.train()
    m.zero_grad()
    out = m(inp)
    loss = nn.BCELoss()(out.reshape(-1), y.reshape(-1))
    loss.backward()
    return out.detach().reshape(-1), float(loss.item()), {n: p.grad.detach().cpu().numpy().copy()
                                                           for n, p in m.named_parameters()}


def check_abs(what, got, want):
    err = float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max()) if np.size(want) else 0.0
    print("  %-52s |err| %.3e  bound %.1e" % (what, err, ref.SCORE_BOUND))
    return [] if err <= ref.SCORE_BOUND else ["%s: %.3e > %.1e" % (what, err, ref.SCORE_BOUND)]


def check_rel(what, got, want, ref_err):
    err, b = ref.rel_err(got, want), ref.grad_bound(ref_err)
    print("  %-52s err %.3e  bound %.3e  (reference's own %.3e)" % (what, err, b, float(ref_err)))
    return [] if err <= b else ["%s: %.3e > %.3e" % (what, err, b)]


def random_graph(rng, nh, ns, F, lone=True):
    """nh hits, ns segments between distinct hits (a lower id to a higher one); with `lone` the last hit has none."""
    X = rng.uniform(-1.0, 1.0, size=(nh, F)).astype(np.float32)
    top = nh - 1 if (lone and nh >= 3) else nh
    if top < 2:
        ns = 0
    a = rng.integers(0, max(top - 1, 1), size=ns)
    b = a + 1 + rng.integers(0, np.maximum(top - 1 - a, 1), size=ns) if ns else a
    y = (rng.random(ns) < 0.3).astype(np.float32)
    return synth.HitGraph(X, a.astype(np.int32), np.minimum(b, top - 1).astype(np.int32), y)


def random_params(F, D, T, shared, seed):
    torch.manual_seed(seed)
    m = (ToySegmentClassifier2 if shared else ToySegmentClassifier)(F, D, T)
    return {k: v.detach().numpy().copy() for k, v in m.state_dict().items()}


def reference_error(params, X, src, dst, y, T, r64, orders=8):
    """The reference's own fp32 error on synthetic inputs, per tensor: the restatement run in fp32 on the CPU with the
    segments in `orders` orders (as given, then seeded permutations), the largest distance from the fp64 run.  One
    run is ONE sample of a rounding error, and where a gradient is a cancelling sum the samples spread: the bias of
    edge_networks[0]'s output layer in test_segment_count_edges[32] is a sum of 3 800 terms whose absolute values add
    up to 86 times the sum, and the fp32 restatement's error on it is anywhere from 0.9e-6 to 5.3e-6 over eight
    orders (measured on the CPU alone).  A fixture's ref_err_* is the one sample the reference gave: this stand-in, a
    largest of eight, is WIDER than that one-sample figure, so the synthetic cases are held to a looser bound than the
    fixtures are (never below the project's 5e-6 either way)."""
    own = {}
    for i in range(orders):
        o = np.arange(len(src)) if i == 0 else np.random.default_rng(i).permutation(len(src))
        r32 = ref.run(params, X, src[o], dst[o], y[o], T, dtype=torch.float32)
        own["loss"] = max(own.get("loss", 0.0), ref.rel_err(r32["loss"], r64["loss"]))
        for k in params:
            own[k] = max(own.get(k, 0.0), ref.rel_err(r32["grads"][k], r64["grads"][k]))
    return own


def check_graphs(hip, graphs, F, D, T, want_infer, want_train, shared=False, seed=0):
    """Inference and one training step on `graphs` by the default route, against the fp64 restatement."""
    params = random_params(F, D, T, shared, seed)
    batch = HitGraphBatch.from_graphs(graphs).to("cuda")
    X, src, dst, y = (batch.X.cpu().numpy(), batch.src.cpu().numpy(), batch.dst.cpu().numpy(), batch.y.cpu().numpy())
    r64 = ref.run(params, X, src, dst, y, T)
    own = reference_error(params, X, src, dst, y, T, r64)
    m = model_of(params, F, D, T, shared)
    bad = []
    with torch.no_grad():
        e = m.eval()(batch)
    print("  inference route %s" % m._route.kind)
    assert m._route.kind == want_infer
    bad += check_abs("scores", e.cpu().numpy(), r64["e"][T])
    out, loss, grads = train_step(m, batch, batch.y)
    print("  training route %s" % m._route.kind)
    assert m._route.kind == want_train
    bad += check_abs("training scores", out.cpu().numpy(), r64["e"][T])
    bad += check_rel("loss", loss, r64["loss"], own["loss"])
    for k in params:
        bad += check_rel("grad " + k, grads[k], r64["grads"][k], own[k])
    assert not bad, "\n".join(bad)


# ---- the shape matrix --------------------------------------------------------------------------------------------------
# Every (input_dim, hidden_dim) of IterShapes in csrc/iter_events.hip; test_toy_mpnn_shapes_host.py derives the same set
# from the library and fails when the two differ.
MATRIX = [(2, 4), (2, 8), (2, 16), (2, 32), (3, 4), (3, 8), (3, 16), (3, 32), (4, 8), (4, 16), (4, 32), (11, 4), (11, 8),
          (11, 16)]
MATRIX_T = 2
# (hits, segments) per graph.  ragged: a lone hit in every graph of >= 3 hits, one-hit and two-hit graphs, graphs without
# segments.  padded (from_graphs(pad_segments=True)): 68 padded of 432 segments - below a quarter, so that the
# reference's own fp32 gradient error stays small and the bound with it.
BATCH_SIZES = {"ragged": [(30, 70), (1, 0), (9, 0), (2, 1), (40, 144), (17, 33)],
               "padded": [(40, 144), (35, 120), (30, 100)]}
MATRIX_CAPS = (40, 144)         # the largest graph of either batch: what iter_events_supported is asked


def shape_seed(F, D, kind="ragged"):
    return 1000 * F + 10 * D + (kind == "padded")


def matrix_graphs(F, D, kind):
    rng = np.random.default_rng(shape_seed(F, D, kind))
    return [random_graph(rng, nh, ns, F) for nh, ns in BATCH_SIZES[kind]]


def matrix_batch(F, D, kind):
    """The host batch of one shape: features U(-1, 1), seeded per shape."""
    return HitGraphBatch.from_graphs(matrix_graphs(F, D, kind), pad_segments=kind == "padded")


def host_arrays(batch):
    return tuple(np.asarray(a.cpu() if torch.is_tensor(a) else a) for a in (batch.X, batch.src, batch.dst, batch.y))


@functools.lru_cache(maxsize=None)
def matrix_reference(F, D, shared, kind, T=MATRIX_T):
    """(params, r64, own) of one matrix case: default-init weights seeded per shape, the fp64 run, the reference's own
    fp32 error.  Computed once and shared by every test that needs it; nobody writes into it."""
    params = random_params(F, D, T, shared, shape_seed(F, D))
    X, src, dst, y = host_arrays(matrix_batch(F, D, kind))
    r64 = ref.run(params, X, src, dst, y, T)
    return params, r64, reference_error(params, X, src, dst, y, T, r64)
