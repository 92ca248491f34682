"""Integer-exact inputs for the graph-convolution classifiers: cases on which the kernels of csrc/gcn.hip must equal an
fp64 reference BIT FOR BIT.  Not a test module.

The model is linear maps and ReLU only.  With small-integer x, A, weights and output gradient every product and every
partial sum is an integer; when, for every dot product the kernels form, the sum of the ABSOLUTE values of its terms
stays below 2^24 (the integer range of fp32), every partial sum is exactly representable in ANY summation order, fmaf
included, so fp32 arithmetic is exact.  A dropped, doubled or misindexed list entry then moves some integer by at
least 1, and z == 0 occurs often: the ReLU-mask edge (h > 0 against relu'(0) = 0).

Ingredients: x in {-1, 0, 1, 2}; A with a +-1 dense row (N // 2) and a +-1 dense column (N // 3) plus entries from
{-2, -1, 1, 2} at density 4 / N; weights and biases in {-1, 0, 1} at density min(1, fan / fan_in), fan = 12 unless a
case thins it to keep the term bound; the classifier weight all +-1; output gradient G in {-2, -1, 1, 2}; loss
(out * G).sum().

`exact_case` checks the conditions that make "bit for bit" legitimate and raises ExactCaseError when one fails:
the term bound, fp32 == fp64 on the CPU, not degenerate, and sensitive to the last entry of the widest row list and
of the widest column list.  tests/test_gcn_exact_host.py runs it on every entry of CASES; the GPU tests read the
same table.
"""
import numpy as np
import torch

import gcn_fp64 as ref

LIMIT = float(2 ** 24)


class ExactCaseError(AssertionError):
    pass


class Case:
    """x [B, N, F], A [B, N, N], G [B, N] (fp32 numpy, integer-valued), `model` (a DenseGCN with integer-valued fp32
    parameters) and the shape it was built for; `dead`: the units whose bias is -100 in every layer; `term_bound`:
    the largest sum of absolute terms of any dot product (None when not verified)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def state(self):
        return self.model.state_dict()


# ---- the shared case table ---------------------------------------------------------------------------------------------
# name -> arguments of exact_case.  N = None: the largest N the library accepts for (F, max(dims)), filled in by
# `resolve`, which asks _lib.gcn_supported.  A seed is one for which the conditions hold; `fan` below 12 thins the
# weights of a case whose term bound would otherwise pass 2^24.
def _c(N, B, F, dims, kind, conv, seed, **kw):
    return dict(N=N, B=B, F=F, dims=dims, kind=kind, conv=conv, seed=seed, **kw)


CASES = {
    # idle-thread widths: every width as din and as dout; above 128 one row per pass
    "idle_gcrn_graphconv_129_85_200_86": _c(40, 3, 7, [129, 85, 200, 86], "gcrn", "graphconv", 1, fan=2),
    "idle_gcn_graphconv_255_128_256": _c(70, 2, 3, [255, 128, 256], "gcn", "graphconv", 2, fan=4),
    "idle_gcn_selfint_86_256_85_129": _c(40, 2, 3, [86, 256, 85, 129], "gcn", "selfint", 3, fan=2),
    # the same widths at an N small enough for the layer's weights to be staged in LDS beside the row buffers
    "idle_staged_gcn_selfint_129_85_86_129": _c(8, 2, 3, [129, 85, 86, 129], "gcn", "selfint", 22, fan=3),
    # widest net, cin = 320, at the largest N the LDS check lets through (weights not staged, x read from global
    # memory) and at N = 58, the largest at which the forward still stages x in LDS
    "widest_gcrn_selfint_f64_256_256": _c(None, 2, 64, [256, 256], "gcrn", "selfint", 104),
    "widest_gcrn_selfint_f64_256_256_x_staged": _c(58, 2, 64, [256, 256], "gcrn", "selfint", 104),
    # most nodes: the dense row and column make the list width 4096
    "nodes_4096": _c(4096, 2, 1, [2, 2], "gcn", "selfint", 605),
    # F extremes.  F = 64 at N = 200: the two row buffers and x together pass the LDS limit, so the forward reads x
    # from global memory; the same net at N = 181 and 182, the two sides of that decision, and at its largest N
    "f64_gcrn_selfint_8_16": _c(200, 2, 64, [8, 16], "gcrn", "selfint", 6),
    "f64_gcrn_selfint_8_16_x_staged": _c(181, 2, 64, [8, 16], "gcrn", "selfint", 23),
    "f64_gcrn_selfint_8_16_x_global": _c(182, 2, 64, [8, 16], "gcrn", "selfint", 23),
    "f64_gcrn_selfint_8_16_largest_n": _c(None, 2, 64, [8, 16], "gcrn", "selfint", 23),
    "f1_gcn_graphconv_8_12_16": _c(37, 3, 1, [8, 12, 16], "gcn", "graphconv", 7),
    # LDS limit: the largest accepted N of [64, 64] F = 3 (weights NOT staged) and of a narrow pair; N = 37: staged
    "lds_gcrn_selfint_64_64_max": _c(None, 2, 3, [64, 64], "gcrn", "selfint", 8),
    "lds_gcrn_selfint_64_64_staged": _c(37, 2, 3, [64, 64], "gcrn", "selfint", 9),
    "lds_gcn_selfint_4_4_max": _c(None, 2, 1, [4, 4], "gcn", "selfint", 10, fan=2),
    # many graphs: the grid exceeds 65 535 and k_gcn_reduce sums 70 000 partials (weights thinned for the sum over B)
    "graphs_70000": _c(4, 70000, 3, [8, 8], "gcn", "selfint", 11, fan=1.5),
    # degenerate
    "one_node": _c(1, 1, 3, [4, 4], "gcn", "selfint", 412),
    "holes": _c(37, 3, 3, [8, 12, 16], "gcrn", "selfint", 13, adjacency="holes"),
    # ballot and list boundaries
    "ballot_63": _c(63, 2, 3, [8, 12], "gcn", "selfint", 314),
    "ballot_64": _c(64, 2, 3, [8, 12], "gcrn", "graphconv", 15),
    "ballot_65": _c(65, 2, 3, [8, 12], "gcn", "selfint", 16),
    "ballot_257": _c(257, 2, 3, [8, 12], "gcrn", "selfint", 17),
    "ballot_257_lists_64_65": _c(257, 2, 3, [8, 12], "gcn", "selfint", 18, adjacency="ballot"),
    # dead units: two units of every layer have bias -100
    "dead_units": _c(37, 3, 3, [8, 12, 16], "gcn", "selfint", 319, dead=True, fan=4),
    # slices: adj[1:B-1] of a B = 5 batch
    "slices": _c(37, 5, 3, [8, 12, 16], "gcrn", "selfint", 20),
    # the deepest net the term bound allows with these ingredients (see DEEPEST below)
    "deepest": None,
}

# The deepest net: width 8, N = 16, B = 2, F = 3, GCN GraphConvSelfInt, weights thinned to two entries per row (fan = 2).
# Every layer multiplies the term bound by about 12 (|Wn| + |Wg| |A|, the dense row and column of A included): four
# graph-convolution layers reach 1.35e7, just below 2^24 = 1.68e7, and a fifth passes it tenfold for every seed
# (test_gcn_exact_host.py pins that).  Depth itself stays with the 16-layer float test of test_gpu_gcn.py.
DEEPEST_LAYERS = 4
CASES["deepest"] = _c(16, 2, 3, [8] * (DEEPEST_LAYERS + 1), "gcn", "selfint", 421, fan=2)
LDS_PAIRS = ["lds_gcrn_selfint_64_64_max", "widest_gcrn_selfint_f64_256_256", "lds_gcn_selfint_4_4_max"]


def largest_n(F, maxw, list_width=1):
    """The largest N that gnn_gcn_supported accepts for (F, maxw): asked, not computed from the LDS formula."""
    from gnn_fpga_amd import _lib
    ok = lambda n: _lib.gcn_supported(n, F, maxw, min(list_width, n))           # noqa: E731
    if not ok(1):
        raise ExactCaseError("the library refuses N = 1 for F %d width %d" % (F, maxw))
    lo, hi = 1, 4097                                            # ok(lo), not ok(hi): N <= 4096 is the node limit
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ok(mid):
            lo = mid
        else:
            hi = mid
    return lo


def resolve(name):
    """The arguments of CASES[name] with N filled in."""
    kw = dict(CASES[name])
    if kw["N"] is None:
        kw["N"] = largest_n(kw["F"], max(kw["dims"]))
    return kw


_CACHE = {}


def get(name):
    """(case, reference) of a table entry, built and verified once per process and left unchanged."""
    if name not in _CACHE:
        case = exact_case(**resolve(name))
        _CACHE[name] = (case, case.reference)
    return _CACHE[name]


# ---- generator ---------------------------------------------------------------------------------------------------------
def _signs(rng, shape):
    return rng.integers(0, 2, size=shape) * 2 - 1


def _nonzero(rng, shape):
    """Entries from {-2, -1, 1, 2}."""
    return _signs(rng, shape) * rng.integers(1, 3, size=shape)


def _adjacency(rng, B, N, style):
    A = (rng.random((B, N, N)) < min(1.0, 4.0 / N)) * _nonzero(rng, (B, N, N))
    if style == "dense":                                        # list width = N
        A[:, N // 2, :] = _signs(rng, (B, N))
        A[:, :, N // 3] = _signs(rng, (B, N))
    elif style == "holes":                                      # empty rows and columns, entries at index N - 1
        A[:, N // 2, :] = _signs(rng, (B, N))
        A[:, :, N // 3] = _signs(rng, (B, N))
        for k in (0, 5, N - 2):
            A[:, k, :] = 0
            A[:, :, k + 1] = 0
        A[:, N - 1, N - 1] = 2
        A[:, 2, N - 1] = -1
        A[:, N - 1, 3] = 1
    elif style == "ballot":
        # rows N-3, N-2, N-1: entries at columns 0..63 (exactly 64), 0..64 (exactly 65) and 64 alone; the columns
        # N-3, N-2, N-1 the same with rows
        if N < 68 + 3:
            raise ExactCaseError("the ballot adjacency needs N >= 71")
        A[:, N - 3:, :] = 0
        A[:, :, N - 3:] = 0
        A[:, N - 3, :64] = _signs(rng, (B, 64))
        A[:, N - 2, :65] = _signs(rng, (B, 65))
        A[:, N - 1, 64] = 2
        A[:, :64, N - 3] = _signs(rng, (B, 64))
        A[:, :65, N - 2] = _signs(rng, (B, 65))
        A[:, 64, N - 1] = -2
    else:
        raise ValueError(style)
    return A.astype(np.float32)


def _thin(rng, shape, density):
    """{-1, 0, 1}, non-zero with probability `density`."""
    return ((rng.random(shape) < density) * _signs(rng, shape)).astype(np.float32)


def exact_case(N, B, F, dims, kind, conv, seed, adjacency="dense", dead=False, fan=12, verify=True):
    """A Case built from the module's ingredients.  With `verify` the four conditions of the module docstring are
    checked here and ExactCaseError is raised when one fails; `case.reference` is then the fp64 reference."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-1, 3, size=(B, N, F)).astype(np.float32)
    A = _adjacency(rng, B, N, adjacency)
    G = _nonzero(rng, (B, N)).astype(np.float32)
    model = ref.DenseGCN(F, dims, kind, conv)
    dead_units = (1, min(dims) - 2) if dead else ()
    with torch.no_grad():
        for name, mod in model.named_modules():
            if not isinstance(mod, torch.nn.Linear):
                continue
            density = min(1.0, float(fan) / mod.in_features)
            if name == "classifier":
                mod.weight.copy_(torch.from_numpy(_signs(rng, tuple(mod.weight.shape)).astype(np.float32)))
            else:
                mod.weight.copy_(torch.from_numpy(_thin(rng, tuple(mod.weight.shape), density)))
            if mod.bias is not None:
                v = _thin(rng, tuple(mod.bias.shape), density)
                if dead and name != "classifier":
                    v[list(dead_units)] = -100.0
                mod.bias.copy_(torch.from_numpy(v))
    case = Case(N=N, B=B, F=F, dims=list(dims), kind=kind, conv=conv, seed=seed, adjacency=adjacency, x=x, A=A, G=G,
                model=model, dead=dead_units, term_bound=None, reference=None)
    if verify:
        _verify(case)
    return case


# ---- the reference -----------------------------------------------------------------------------------------------------
def _run(model, x, a, g, dtype):
    """DenseGCN in `dtype` with loss (out * G).sum(): logits, per-layer h, gradients (numpy, in `dtype`)."""
    import copy
    m = copy.deepcopy(model).to(dtype)
    m.zero_grad()
    hs = []
    out = m(x.to(dtype), a if a.dtype == dtype else a.to(dtype), keep=hs)
    (out * g.to(dtype)).sum().backward()
    return {"logits": out.detach().numpy(), "h": [h.detach().numpy() for h in hs],
            "grads": {n: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().numpy()
                      for n, p in m.named_parameters()}}


def exact_reference(case):
    """The fp64 reference of a case: {"logits", "h": [per layer], "grads": {name: array}}, float64 arrays."""
    return _run(case.model, torch.from_numpy(case.x), torch.from_numpy(case.A), torch.from_numpy(case.G),
                torch.float64)


def to_fp32(r):
    """A reference cast to fp32 (exact: every value is an integer below 2^24)."""
    return {"logits": r["logits"].astype(np.float32), "h": [h.astype(np.float32) for h in r["h"]],
            "grads": {k: v.astype(np.float32) for k, v in r["grads"].items()}}


def term_bound(case):
    """The largest, over every dot product the kernels form, of the sum of the absolute values of its terms: |x|,
    |A|, |W|, |b| propagated forward WITHOUT ReLU and |G| backward without the mask, in fp64.  The weight-gradient
    sums are taken over the nodes AND the graphs at once (k_gcn_bwd's per-graph sums and k_gcn_reduce's sum over B
    are both below it)."""
    f64 = torch.float64
    x, A, G = (torch.from_numpy(np.abs(v)).to(f64) for v in (case.x, case.A, case.G))
    P = {n: p.detach().abs().to(f64) for n, p in case.model.named_parameters()}
    residual, selfint = case.kind == "gcrn", case.conv == "selfint"
    worst = [0.0]

    def see(t):
        if t.numel():
            worst[0] = max(worst[0], float(t.max()))
        return t

    h = see(x @ P["feature_extractor.weight"].T + P["feature_extractor.bias"])
    hins = []
    for l in range(len(case.dims) - 1):
        hin = torch.cat([h, x], dim=-1) if residual else h
        hins.append(hin)
        ah = see(torch.matmul(A, hin))
        pre = "gc_layers.%d." % l
        if selfint:
            h = see(hin @ P[pre + "node_mod.weight"].T + P[pre + "node_mod.bias"] + ah @ P[pre + "neighbor_mod.weight"].T)
        else:
            h = see(ah @ P[pre + "linear.weight"].T + P[pre + "linear.bias"])
    see(h @ P["classifier.weight"].T + P["classifier.bias"])
    # backward
    see(torch.einsum("bn,bnc->c", G, h))                       # classifier.weight
    see(G.sum())                                                # classifier.bias
    gz = see(G.unsqueeze(-1) * P["classifier.weight"])
    for l in range(len(case.dims) - 2, -1, -1):
        hin, din = hins[l], case.dims[l]
        pre = "gc_layers.%d." % l
        q = see(torch.matmul(A.transpose(1, 2), gz))
        see(gz.sum(dim=(0, 1)))                                 # bias
        see(torch.einsum("bno,bnc->oc", q, hin))                # neighbor_mod.weight / linear.weight
        if selfint:
            see(torch.einsum("bno,bnc->oc", gz, hin))           # node_mod.weight
            gz = see(gz @ P[pre + "node_mod.weight"] + q @ P[pre + "neighbor_mod.weight"])[..., :din]
        else:
            gz = see(q @ P[pre + "linear.weight"])[..., :din]
    see(torch.einsum("bno,bnf->of", gz, x))                     # feature_extractor.weight
    see(gz.sum(dim=(0, 1)))
    return worst[0]


def widest_list_last_entry(A, columns=False):
    """(b, i, j) of the LAST entry of the widest row list (or column list) of A; None for an all-zero A."""
    nz = A != 0
    cnt = nz.sum(axis=1 if columns else 2)                      # [B, N]: per column / per row
    if cnt.size == 0 or cnt.max() == 0:
        return None
    b, k = np.unravel_index(int(np.argmax(cnt)), cnt.shape)
    if columns:
        i = int(np.nonzero(nz[b, :, k])[0][-1])
        return int(b), i, int(k)
    j = int(np.nonzero(nz[b, k, :])[0][-1])
    return int(b), int(k), j


def _same(r1, r2):
    """Bit-for-bit equality of two results, the second cast to the first's type."""
    bad = []
    if not np.array_equal(r1["logits"], r2["logits"].astype(r1["logits"].dtype)):
        bad.append("logits")
    bad += ["h%d" % l for l, (a, b) in enumerate(zip(r1["h"], r2["h"])) if not np.array_equal(a, b.astype(a.dtype))]
    bad += [k for k, v in r1["grads"].items() if not np.array_equal(v, r2["grads"][k].astype(v.dtype))]
    return bad


def _verify(case):
    what = "exact case N=%d B=%d F=%d %s %s %s seed %d" % (case.N, case.B, case.F, case.dims, case.kind, case.conv,
                                                           case.seed)
    for v in (case.x, case.A, case.G) + tuple(p.detach().numpy() for p in case.model.parameters()):
        if not np.array_equal(v, np.round(v)):
            raise ExactCaseError("%s: an input is not integer-valued" % what)
    # 1. term bound
    case.term_bound = term_bound(case)
    if not case.term_bound < LIMIT:
        raise ExactCaseError("%s: term bound %.4g is not below 2^24" % (what, case.term_bound))
    # 2. fp32 equals fp64 on the CPU
    x, G = torch.from_numpy(case.x), torch.from_numpy(case.G)
    a32 = torch.from_numpy(case.A)
    a64 = a32.to(torch.float64)
    r64 = _run(case.model, x, a64, G, torch.float64)
    r32 = _run(case.model, x, a32, G, torch.float32)
    bad = _same(r32, r64)
    if bad:
        raise ExactCaseError("%s: fp32 differs from fp64 on the CPU in %s" % (what, bad))
    case.reference = r64
    if case.B == 0:
        return
    # 3. not degenerate
    for l, h in enumerate(r64["h"]):
        share = float((h > 0).mean())
        if not 0.10 <= share <= 0.90:
            raise ExactCaseError("%s: share of h > 0 in layer %d is %.3f, outside [0.10, 0.90]" % (what, l, share))
    for k, g in r64["grads"].items():
        share = float((g != 0).mean())
        if share < 0.25:
            raise ExactCaseError("%s: only %.3f of grad %s is non-zero" % (what, share, k))
    for u in case.dead:
        for l, h in enumerate(r64["h"]):
            if h[..., u].any():
                raise ExactCaseError("%s: unit %d of layer %d is meant to be dead and is not" % (what, u, l))
    # 4. sensitive to the last entry of the widest row list, and of the widest column list
    if len(case.dims) > 1:
        for columns in (False, True):
            b, i, j = widest_list_last_entry(case.A, columns)
            keep = float(a64[b, i, j])
            a64[b, i, j] = 0.0
            r = _run(case.model, x[b:b + 1], a64[b:b + 1], G[b:b + 1], torch.float64)
            a64[b, i, j] = keep
            # (the loss is a plain sum over the graphs: graph b's own gradient moves iff the batch's does)
            whole = _run(case.model, x[b:b + 1], a64[b:b + 1], G[b:b + 1], torch.float64)
            moved_logit = not np.array_equal(r["logits"], whole["logits"])
            moved_grad = any(not np.array_equal(r["grads"][k], whole["grads"][k]) for k in whole["grads"])
            if not (moved_logit and moved_grad):
                raise ExactCaseError("%s: zeroing A[%d, %d, %d], the last entry of the widest %s list, moves %s"
                                     % (what, b, i, j, "column" if columns else "row",
                                        "no logit" if not moved_logit else "no gradient entry"))
