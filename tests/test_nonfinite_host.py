"""The non-finite cases of tests/nonfinite_cases.py on the CPU: that every case test_gpu_nonfinite.py asserts exactly
is well posed - the project's restatements agree with each other on where the NaNs are - and the pins the kernels'
fixes are written against (bf16 conversion, BCE reference, the list-form GCN product).

Where the oracles do NOT agree (found here, kept out of the GPU assertions):
  padded segments   oracle.index_torch gathers row 0 for a padded segment and multiplies it by zero: a NaN in hit 0
                    (every weight site ahead of the edge network makes one) turns every padded score into NaN there.
                    oracle.index_c, tests/nodeclf_fp64.py and the kernels read no hit for a padded segment.  The GPU
                    tests take index_torch's mask on the valid segments and index_c's on the padded ones
                    (nonfinite_cases.expected_mask); the valid segments agree in all three, checked below.
  gradients         oracle.index_c has no backward: the NaN masks of the loss and of the ten gradients are held
                    between index_torch in fp64 and in fp32 only (test_training_references_are_all_nan); index_c
                    takes part in the scores' masks.
  BCE gradient      autograd through the clamped logarithms is not NaN at a score outside [0, 1] and is NaN at exactly
                    0 and 1 (test_bce_reference): the gradient reference is nonfinite_cases.bce_grad.
"""
import numpy as np
import pytest
import torch

import gcn_fp64
import nonfinite_cases as nf
import route_cases
from oracle import bf16_torch

SEG_SHAPES = [(3, 8, 3), (3, 32, 2), (3, 64, 2)]        # (F, D, T) of the forward routes on seg_batch


def _weights(F, D, T):
    return route_cases.host_weights(dict(F=F, D=D, T=T))


def _host_plan(b, D):
    from gnn_fpga_amd import _lib
    from gnn_fpga_amd.plan import SellPlan
    return SellPlan(b, _lib.plan_limits(b.n_features, D))


def _seg_cases(F, D, T):
    """(name, X, weights) of every case the forward routes run on seg_batch at this shape."""
    b, w = nf.seg_batch(F), _weights(F, D, T)
    for name, hit in nf.x_sites(b, nf.SEG_GRAPH, _host_plan(b, D)).items():
        yield "X " + name, nf.poisoned_X(b, hit, nf.QNAN), w
        for inf, v in nf.INFS.items():
            yield "X %s %s" % (name, inf), nf.poisoned_X(b, hit, v), w
    for k, t in enumerate(w):
        yield "W %d" % k, b.X.numpy(), w[:k] + [nf.put(t, nf.w_site(t), nf.QNAN)] + w[k + 1:]


def test_the_batch_is_what_the_cases_need():
    b = nf.seg_batch()
    assert (b.n_hits, b.n_segments, b.n_graphs) == (927, 6033, 4)
    assert int((b.src.numpy() < 0).sum()) == len(range(7, 6033, 13))
    sites = nf.x_sites(b, nf.SEG_GRAPH, _host_plan(b, 8))
    assert set(sites) == {"first", "last", "lonely", "tile"} and sites["first"] > 0
    lo, hi = int(b.hit_ptr[nf.SEG_GRAPH]), int(b.hit_ptr[nf.SEG_GRAPH + 1])
    assert all(lo <= h < hi for n, h in sites.items() if n != "lonely") and hi <= sites["lonely"] < int(b.hit_ptr[3])
    assert {"first", "last"} <= set(nf.x_sites(nf.muon_batch(), nf.MUON_GRAPH))
    assert nf.twin_batch().n_hits == 21000


@pytest.mark.parametrize("F,D,T", SEG_SHAPES)
def test_segment_oracles_agree_on_the_masks(F, D, T):
    """index_torch in fp64 and fp32 and index_c (both precisions): one NaN mask on the valid segments; a NaN reaches
    a score, never more than its graph, and the lonely hit none; Inf in X leaves every score finite (tanh(+-inf) =
    +-1) and within 1e-5 of the fp64 value in fp32."""
    b = nf.seg_batch(F)
    valid = b.src.numpy() >= 0
    own = nf.segments_of_graphs(b, [nf.SEG_GRAPH])
    for name, X, w in _seg_cases(F, D, T):
        e64, e32 = nf.scores64(X, b, w, T), nf.scores64(X, b, w, T, torch.float32)
        c64, c32 = nf.scores_c(X, b, w, T, True), nf.scores_c(X, b, w, T, False)
        m = np.isnan(e64)
        for what, other in (("index_torch fp32", e32), ("index_c fp64", c64), ("index_c fp32", c32)):
            assert np.array_equal(np.isnan(other)[valid], m[valid]), (name, what)
        assert not np.isinf(e64).any(), name
        if "inf" in name:
            assert not m.any(), name
            if D >= 32:       # the bf16 route's emulation (oracle.bf16_torch, no exp-product form): no NaN either
                eb = bf16_torch.segment_classifier(X, b.src.numpy(), b.dst.numpy(), w, T, xp=False).numpy()
                assert not np.isnan(eb).any(), name
            assert np.abs(e32 - e64).max() < 1e-5 and np.abs(c32 - e64).max() < 1e-5, name
        elif name.startswith("W"):
            assert m[valid].all(), name                      # a NaN weight: every valid score
        elif name == "X lonely":
            assert not m.any(), name
        else:
            assert m.any() and not m[~own].any(), name
        # the padded segments: index_c reads no hit for them; the two differ only where hit 0 is NaN
        mask, _ = nf.expected_mask(X, b, w, T)
        assert np.array_equal(mask[valid], m[valid]) and np.array_equal(mask[~valid], np.isnan(c64)[~valid]), name
        if not name.startswith("W"):
            assert np.array_equal(mask, m), name


def test_event_oracles_agree_on_the_masks():
    b, (F, D, T) = nf.muon_batch(), (11, 8, 3)
    w = _weights(F, D, T)
    own = nf.segments_of_graphs(b, [nf.MUON_GRAPH])
    cases = [("X " + n, nf.poisoned_X(b, h, nf.QNAN), w) for n, h in nf.x_sites(b, nf.MUON_GRAPH).items()]
    cases += [("W %d" % k, b.X.numpy(), w[:k] + [nf.put(t, nf.w_site(t), nf.QNAN)] + w[k + 1:]) for k, t in enumerate(w)]
    for name, X, wk in cases:
        m = np.isnan(nf.scores64(X, b, wk, T))
        for other in (nf.scores64(X, b, wk, T, torch.float32), nf.scores_c(X, b, wk, T, True), nf.scores_c(X, b, wk, T, False)):
            assert np.array_equal(np.isnan(other), m), name
        assert m.all() if name.startswith("W") else (m.any() and not m[~own].any()), name


TRAIN_CASES = [("seg", 3, 8, 3), ("seg", 3, 32, 2), ("muon", 11, 8, 3), ("twin", 3, 8, 2)]


def train_case(kind, F, D, T, site):
    """(batch, X, weights, labels) of a training case; site: "X" (first hit of the middle graph) or "W" (W3)."""
    b, g = {"seg": (nf.seg_batch(F), nf.SEG_GRAPH), "muon": (nf.muon_batch(), nf.MUON_GRAPH),
            "twin": (nf.twin_batch(), nf.TWIN_GRAPH)}[kind]
    w = _weights(F, D, T)
    X = b.X.numpy()
    if site == "X":
        X = nf.poisoned_X(b, nf.x_sites(b, g)["first"], nf.QNAN)
    else:
        w[6] = nf.put(w[6], nf.w_site(w[6]), nf.QNAN)
    return b, X, w, nf.labels(b.n_segments)


@pytest.mark.parametrize("site", ["X", "W"])
@pytest.mark.parametrize("kind,F,D,T", TRAIN_CASES)
def test_training_references_are_all_nan(kind, F, D, T, site):
    """The loss and every element of all ten gradients are NaN in fp64 and in fp32: no summation order can matter to
    the masks the GPU test compares."""
    b, X, w, y = train_case(kind, F, D, T, site)
    for dtype in (torch.float64, torch.float32):
        loss, grads = nf.train_reference(X, b, w, T, y, dtype)
        assert np.isnan(loss)
        assert all(np.isnan(g).all() for g in grads), [float(np.isnan(g).mean()) for g in grads]


@pytest.mark.parametrize("D", [8, 64])
def test_node_classifier_references(D):
    b, (F, T) = nf.seg_batch(), (3, 2)
    case = dict(F=F, D=D, T=T)
    w12 = _weights(F, D, T) + list(route_cases.head(case))
    y = nf.labels(b.n_hits, 1)
    lo, hi = int(b.hit_ptr[nf.SEG_GRAPH]), int(b.hit_ptr[nf.SEG_GRAPH + 1])
    X = nf.poisoned_X(b, nf.x_sites(b, nf.SEG_GRAPH)["first"], nf.QNAN)
    wp = list(w12)
    wp[6] = nf.put(wp[6], nf.w_site(wp[6]), nf.QNAN)
    for what, Xc, wc in (("X", X, w12), ("W", b.X.numpy(), wp)):
        masks = []
        for dtype in (torch.float64, torch.float32):
            s, loss, grads = nf.nodeclf_reference(Xc, b, wc, T, y, dtype)
            assert np.isnan(loss) and all(np.isnan(g).all() for g in grads), what
            masks.append(np.isnan(s))
        assert np.array_equal(*masks), what
        if what == "X":
            assert masks[0].any() and not masks[0][:lo].any() and not masks[0][hi:].any()
        else:
            assert masks[0].all()


# ---- bf16 conversion ------------------------------------------------------------------------------------------------
def test_bf16_rne_keeps_nan_and_is_torch_everywhere_else():
    """The integer form of sell_pipeline.hip's bf16_rne (oracle.bf16_torch.bf16_rne_bits) against torch.bfloat16 on
    the six poisons, the largest finite value and +-0: a NaN stays a NaN - quiet, sign kept - and nothing else
    becomes one; every other value has torch's bits."""
    bits = np.array(list(nf.NAN_BITS.values()) + [0x7F800000, 0xFF800000, 0x7F7FFFFF, 0x00000000, 0x80000000], np.uint32)
    got = bf16_torch.bf16_rne_bits(bits)
    want = bf16_torch.bf16_round(torch.from_numpy(bits.view(np.float32).copy())).numpy()
    back = (got.astype(np.uint32) << np.uint32(16)).view(np.float32)
    assert np.array_equal(np.isnan(back), np.isnan(want)) and list(np.isnan(want)) == [True] * 4 + [False] * 5
    assert np.array_equal(back.view(np.uint32)[4:], want.view(np.uint32)[4:])
    assert [hex(v) for v in got] == ["0x7fc0", "0x7fc0", "0x7fff", "0xffff", "0x7f80", "0xff80", "0x7f80", "0x0", "0x8000"]


# ---- BCE reference --------------------------------------------------------------------------------------------------
def test_bce_reference():
    nan, inf = float("nan"), float("inf")
    e = torch.tensor([nan, 1.5, -0.1, inf, -inf, 0.3, 0.3, 0.0, 1.0, 0.7], dtype=torch.float64, requires_grad=True)
    y = torch.tensor([1.0, 1.0, 0.0, 1.0, 0.0, nan, 1.0, 0.0, 1.0, 0.0], dtype=torch.float64)
    t = nf.bce_terms(e, y)
    assert list(torch.isnan(t)) == [True] * 6 + [False] * 4
    t.sum().backward()
    g = nf.bce_grad(e.detach(), y)
    assert list(torch.isnan(g)) == [True] * 6 + [False] * 4
    # inside (0, 1) autograd IS the formula; outside [0, 1] it is finite (clamp's backward), at 0 and 1 it is NaN
    assert torch.allclose(e.grad[[6, 9]], g[[6, 9]], rtol=1e-12, atol=0)
    assert torch.isfinite(e.grad[1:5]).all() and torch.isnan(e.grad[7:9]).all()
    assert g[7] == 0.0 and g[8] == 0.0
    # and on the valid range the terms are torch.nn.BCELoss's
    ok = torch.tensor([0.0, 1.0, 0.3, 1e-50, 1.0 - 1e-12], dtype=torch.float64)
    yy = torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0], dtype=torch.float64)
    assert torch.equal(nf.bce_terms(ok, yy), torch.nn.functional.binary_cross_entropy(ok, yy, reduction="none"))


# ---- the list-form GCN product --------------------------------------------------------------------------------------
def _gcn_case(cfg, N=37, B=3):
    import test_gpu_gcn as g
    kind, conv, dims = g.CONFIGS[cfg]
    x, A, y = g.synthetic(N, B)
    torch.manual_seed(7 + cfg)
    return gcn_fp64.DenseGCN(3, dims, kind, conv), x, A, y


@pytest.mark.parametrize("cfg", range(4))
def test_list_product_is_the_dense_one_without_poison(cfg):
    model, x, A, y = _gcn_case(cfg)
    d64, d32 = gcn_fp64.run(model, x, A, y, torch.float64), gcn_fp64.run(model, x, A, y, torch.float32)
    l64 = nf.gcn_list_run(model, x, A, y)
    assert gcn_fp64.rel_err(l64["logits"], d64["logits"]) <= gcn_fp64.bound(gcn_fp64.rel_err(d32["logits"], d64["logits"]))
    assert set(l64["grads"]) == set(d64["grads"])
    for k, g in d64["grads"].items():
        assert gcn_fp64.rel_err(l64["grads"][k], g) <= gcn_fp64.bound(gcn_fp64.rel_err(d32["grads"][k], g)), k


def gcn_case(cfg):
    """(kind, conv, dims, model, x, A, y) of the GPU tests' GCN cases: test_gpu_gcn's synthetic 3 x 37 nodes with one
    node of the middle graph that nothing flows into (row 5 keeps its diagonal alone): it must stay finite."""
    import test_gpu_gcn as g
    model, x, A, y = _gcn_case(cfg)
    A = A.copy()
    A[1, 5, :] = 0
    A[1, 5, 5] = 0.5
    return g.CONFIGS[cfg] + (model, x, A, y)


@pytest.mark.parametrize("cfg", range(4))
def test_list_product_keeps_a_nan_to_what_the_lists_reach(cfg):
    """NaN in one x entry of the middle graph: the dense product makes every logit of that graph NaN (0 * NaN), the
    list product exactly the nodes the lists reach within the layers; fp32 and fp64 agree on the logits' and on every
    gradient's mask; other graphs are clean."""
    _, _, _, model, x, A, y = gcn_case(cfg)
    x = x.copy()
    x[1, 7, 0] = nf.QNAN
    dense = np.isnan(gcn_fp64.run(model, x, A)["logits"])
    runs = [nf.gcn_list_run(model, x, A, y, dt) for dt in (torch.float64, torch.float32)]
    masks = [np.isnan(r["logits"]) for r in runs]
    assert np.array_equal(*masks)
    assert dense[1].all() and not dense[[0, 2]].any()
    assert np.array_equal(masks[0][1], nf.gcn_reach(A, 1, 7, len(model.gc_layers))) and not masks[0][[0, 2]].any()
    assert not masks[0][1, 5] and masks[0][1, 7]
    assert np.isnan(runs[0]["loss"]) and np.isnan(runs[1]["loss"])
    for k, g in runs[0]["grads"].items():
        assert np.array_equal(np.isnan(g), np.isnan(runs[1]["grads"][k])), k


@pytest.mark.parametrize("cfg", range(4))
def test_gcn_weight_poison_masks_do_not_depend_on_precision(cfg):
    """A NaN in the middle element of each weight: the list-form reference in fp64 and in fp32 gives all-NaN logits, a
    NaN loss and the SAME NaN mask for every gradient - the condition under which test_gpu_nonfinite.py may compare
    the kernels' gradient masks with the fp64 reference's exactly (a ReLU unit whose sign differed between the two
    precisions would show here)."""
    _, _, _, model, x, A, y = gcn_case(cfg)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    for k, t in state.items():
        model.load_state_dict(dict(state, **{k: nf.put(t, nf.w_site(t), nf.QNAN).reshape(t.shape)}))
        r64, r32 = (nf.gcn_list_run(model, x, A, y, dt) for dt in (torch.float64, torch.float32))
        assert np.isnan(r64["logits"]).all() and np.isnan(r32["logits"]).all(), k
        assert np.isnan(r64["loss"]) and np.isnan(r32["loss"]), k
        for name, g in r64["grads"].items():
            assert np.array_equal(np.isnan(g), np.isnan(r32["grads"][name])), (k, name)
