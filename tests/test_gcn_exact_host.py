"""Host checks of the integer-exact graph-convolution cases (tests/gcn_exact.py): the conditions that make the GPU
tests' "bit for bit" legitimate, proven on the CPU for exactly the inputs the GPU sees, and the measurement that says
why the exact file exists.  No GPU needed."""
import numpy as np
import pytest
import torch

import gcn_exact as ex
import gcn_fp64 as ref
from gnn_fpga_amd import _lib


@pytest.mark.parametrize("name", sorted(ex.CASES))
def test_case_is_exact(name):
    """exact_case raises unless: every dot product's sum of absolute terms is below 2^24, fp32 equals fp64 on the
    CPU bit for bit, every layer has 10 % to 90 % of h > 0 and every gradient tensor at least 25 % non-zero entries,
    and zeroing the last entry of the widest row list (and, separately, column list) moves a logit and a gradient."""
    case, r = ex.get(name)
    kw = ex.resolve(name)
    assert (case.N, case.B, case.F, case.dims, case.kind, case.conv) == \
        (kw["N"], kw["B"], kw["F"], kw["dims"], kw["kind"], kw["conv"])
    assert case.term_bound is not None and case.term_bound < 2 ** 24
    assert r is case.reference and r["logits"].dtype == np.float64 and r["logits"].shape == (case.B, case.N)
    assert [h.shape for h in r["h"]] == [(case.B, case.N, d) for d in case.dims]
    assert set(r["grads"]) == set(case.state)
    biggest = max(float(np.abs(v).max()) for v in [r["logits"]] + r["h"] + list(r["grads"].values()))
    assert biggest <= case.term_bound                           # the bound bounds the results too
    r32 = ex.to_fp32(r)                                         # the cast the GPU tests compare with loses nothing
    assert np.array_equal(r32["logits"].astype(np.float64), r["logits"])
    assert all(np.array_equal(r32["grads"][k].astype(np.float64), v) for k, v in r["grads"].items())
    if len(case.dims) > 1 and case.adjacency == "dense":        # the dense row and column: list width N
        assert int((case.A != 0).sum(-1).max()) == case.N and int((case.A != 0).sum(-2).max()) == case.N
    # the ReLU-mask edge is there: some pre-activation is exactly 0 where a positive one would have been possible
    assert any(float((h == 0).mean()) > 0.1 for h in r["h"])


def test_table_covers_the_corners():
    kws = {n: ex.resolve(n) for n in ex.CASES}
    idle = [kw["dims"] for n, kw in kws.items() if n.startswith("idle_")]
    for w in (85, 86, 129, 256):                                # each idle-thread width as din and as dout
        assert any(w in d[:-1] for d in idle) and any(w in d[1:] for d in idle), w
    assert any(w > 128 for d in idle for w in d)
    wide = kws["widest_gcrn_selfint_f64_256_256"]
    assert wide["F"] == 64 and wide["dims"] == [256, 256] and wide["kind"] == "gcrn" and wide["N"] == 63
    assert kws["f64_gcrn_selfint_8_16"]["N"] == 200 and kws["f64_gcrn_selfint_8_16"]["dims"] == [8, 16]
    assert kws["nodes_4096"]["N"] == 4096 and kws["graphs_70000"]["B"] > 65535
    assert {kws[n]["F"] for n in kws} >= {1, 64}
    assert kws["one_node"]["N"] == 1 and kws["one_node"]["B"] == 1
    assert {kws["ballot_%d" % n]["N"] for n in (63, 64, 65, 257)} == {63, 64, 65, 257}
    assert len(kws["deepest"]["dims"]) - 1 == ex.DEEPEST_LAYERS


def test_lds_limit_cases_sit_at_the_limit():
    """N of the LDS-limit cases is the largest the library accepts, asked of gnn_gcn_supported; the refusal of N + 1
    names the LDS limit.  Restated from gcn.hip only to record which side of the forward's two staging decisions
    each case is on: [64, 64] F = 3 stages its weights at N = 37 and not at its largest N, and x is staged in LDS
    up to N = 58 of the widest net and N = 181 of the F = 64 [8, 16] net and read from global memory above."""
    for name in ex.LDS_PAIRS:
        kw = ex.resolve(name)
        N, F, w = kw["N"], kw["F"], max(kw["dims"])
        assert _lib.gcn_supported(N, F, w, N) and not _lib.gcn_supported(N + 1, F, w, 1)
        assert N + 1 <= 4096 and "LDS" in _lib.load().gnn_last_error().decode()
    assert ex.resolve("lds_gcrn_selfint_64_64_max")["N"] == 305

    def x_staged(N, F, dims):
        return (2 * N * ((max(dims) + F) | 1) + N * F) * 4 <= 160 * 1024

    def staged(N, F, dims, residual):
        lds = (2 * N * ((max(dims) + F) | 1) + (N * F if x_staged(N, F, dims) else 0)) * 4
        wfl = max(2 * (dims[l] + (F if residual else 0)) * dims[l + 1] for l in range(len(dims) - 1))
        return lds + 4 * wfl <= 160 * 1024

    assert staged(37, 3, [64, 64], True) and not staged(305, 3, [64, 64], True)
    assert not staged(58, 64, [256, 256], True) and not staged(63, 64, [256, 256], True)
    assert x_staged(58, 64, [256, 256]) and not x_staged(59, 64, [256, 256]) and not x_staged(63, 64, [256, 256])
    assert x_staged(181, 64, [8, 16]) and not x_staged(182, 64, [8, 16]) and not x_staged(200, 64, [8, 16])
    assert not x_staged(ex.resolve("f64_gcrn_selfint_8_16_largest_n")["N"], 64, [8, 16])
    assert x_staged(37, 3, [64, 64]) and not x_staged(305, 3, [64, 64])
    assert x_staged(ex.resolve("lds_gcn_selfint_4_4_max")["N"], 1, [4, 4])
    # the idle-thread widths run on both sides too
    assert not staged(40, 3, [86, 256, 85, 129], False) and not staged(70, 3, [255, 128, 256], False)
    assert not staged(40, 7, [129, 85, 200, 86], True) and staged(8, 3, [129, 85, 86, 129], False)


def test_one_more_layer_passes_the_term_bound():
    """The "deepest" case is the deepest: with one more layer the term bound passes 2^24 for every seed tried."""
    kw = ex.resolve("deepest")
    kw["dims"] = kw["dims"] + [kw["dims"][-1]]
    for seed in (21, 121, 221, 321, 421):
        kw["seed"] = seed
        with pytest.raises(ex.ExactCaseError, match="term bound"):
            ex.exact_case(**kw)


def test_conditions_are_enforced():
    """exact_case refuses inputs that miss a condition (each of these was met while the table was chosen)."""
    kw = ex.resolve("idle_gcn_selfint_86_256_85_129")
    kw["fan"] = 12                                              # full ingredients on a wide net: not order-independent
    with pytest.raises(ex.ExactCaseError, match="term bound"):
        ex.exact_case(**kw)
    with pytest.raises(ex.ExactCaseError, match="share of h > 0"):
        ex.exact_case(1, 1, 3, [4, 4], "gcn", "selfint", 12)
    with pytest.raises(ex.ExactCaseError, match="widest column list, moves no logit"):
        ex.exact_case(63, 2, 3, [8, 12], "gcn", "selfint", 14)
    with pytest.raises(ex.ExactCaseError, match="of grad classifier.bias is non-zero"):
        ex.exact_case(58, 2, 64, [256, 256], "gcrn", "selfint", 4)
    case, _ = ex.get("ballot_64")
    half = ex.Case(**dict(case.__dict__, x=case.x * np.float32(0.5)))
    with pytest.raises(ex.ExactCaseError, match="not integer-valued"):
        ex._verify(half)
    assert ex.exact_case(63, 2, 3, [8, 12], "gcn", "selfint", 14, verify=False).reference is None


def test_widest_list_last_entry():
    A = np.zeros((2, 5, 5), np.float32)
    A[1, 3, [0, 2, 4]] = 1
    A[0, [1, 2], 2] = -1
    assert ex.widest_list_last_entry(A) == (1, 3, 4)
    A[1, :4, 1] = 2
    assert ex.widest_list_last_entry(A, columns=True) == (1, 3, 1)
    assert ex.widest_list_last_entry(np.zeros((1, 3, 3), np.float32)) is None


def test_float_checks_cannot_see_one_dropped_entry_at_4096_nodes():
    """Why the exact tests exist.  N = 4096, B = 2, F = 1, [2, 2] GCN GraphConvSelfInt on test_gpu_gcn.py's
    synthetic()-style float inputs: setting ONE adjacency entry to zero - the smallest of the dense row of graph 0 -
    moves the fp64 reference's logits and loss by LESS than the bound a GPU result is held to there (4 x the fp32
    reference's own error, at least 16 ulp), and leaves the least sensitive gradient where it was.  On the integer
    case of the same shape the same kind of drop moves a logit and a gradient by at least 1 (test_case_is_exact)."""
    N, B, F, dims = 4096, 2, 1, [2, 2]
    rng = np.random.default_rng(1000 * N + B)
    A = (rng.random((B, N, N)) < 6.0 / N) * rng.normal(size=(B, N, N))
    A[:, N // 2, :] = rng.normal(size=(B, N)) / np.sqrt(N)
    A[:, :, N // 3] = rng.normal(size=(B, N)) / np.sqrt(N)
    i = np.arange(N)
    A[:, i, i] = rng.normal(size=(B, N))
    A = A.astype(np.float32)
    x = rng.normal(size=(B, N, F)).astype(np.float32)
    y = (rng.random((B, N)) < 0.3).astype(np.float32)
    torch.manual_seed(7)
    model = ref.DenseGCN(F, dims, "gcn", "selfint")
    r64 = ref.run(model, x, A, y, torch.float64)
    r32 = ref.run(model, x, A, y, torch.float32)
    j = int(np.argmin(np.where(A[0, N // 2] != 0, np.abs(A[0, N // 2]), np.inf)))
    assert A[0, N // 2, j] != 0
    A[0, N // 2, j] = 0.0
    d64 = ref.run(model, x, A, y, torch.float64)
    moved = ref.rel_err(d64["logits"], r64["logits"])
    bound = ref.bound(ref.rel_err(r32["logits"], r64["logits"]))
    print("\nlogits move %.3e, bound %.3e" % (moved, bound))
    assert 0.0 < moved < bound
    moved = ref.rel_err(d64["loss"], r64["loss"])
    bound = ref.bound(ref.rel_err(r32["loss"], r64["loss"]))
    print("loss moves %.3e, bound %.3e" % (moved, bound))
    assert moved < bound
    least = min(ref.rel_err(d64["grads"][k], g) / ref.bound(ref.rel_err(r32["grads"][k], g))
                for k, g in r64["grads"].items())
    print("least sensitive gradient moves %.3e x its bound" % least)
    assert least < 1.0
