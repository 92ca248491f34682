"""Bit-for-bit GPU checks of the graph-convolution kernels (csrc/gcn.hip) on integer-exact inputs.

Every comparison here is np.array_equal against the fp64 reference cast to fp32: there is no tolerance anywhere.
tests/gcn_exact.py builds the cases and proves, per case, why fp32 arithmetic is exact on them in any summation
order (every dot product's sum of absolute terms is below 2^24); tests/test_gcn_exact_host.py runs those proofs on
the CPU for the same table.  A dropped, doubled or misindexed list entry, a wrong ReLU mask at z == 0 or a partial
sum left out moves some integer by at least 1, so a mismatch is a kernel or glue bug by construction.

Each case checks the logits of the training forward and of eval() under no_grad, every layer of gcn_forward_layers
and every parameter gradient of (m(x, adj) * G).sum().backward(), with a SparseAdjacency and with the dense a."""
import numpy as np
import pytest
import torch

import gcn_exact as ex
from gnn_fpga_amd import _lib
from gnn_fpga_amd.autograd import gcn_forward_layers
from gnn_fpga_amd.gcn import (GCNBinaryClassifier, GCRNBinaryClassifier, GraphConv, GraphConvSelfInt, SparseAdjacency,
                              compress_adjacency)

pytestmark = pytest.mark.gpu
FORMS = ["sparse", "dense"]


def package_model(case):
    cls = GCRNBinaryClassifier if case.kind == "gcrn" else GCNBinaryClassifier
    m = cls(case.F, case.dims, gc_type=GraphConvSelfInt if case.conv == "selfint" else GraphConv)
    m.load_state_dict(case.state)
    return m.cuda()


def first_difference(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "shape %s, expected %s" % (got.shape, want.shape)
    where = np.argwhere(got != want)
    at = tuple(int(v) for v in where[0])
    return "%d of %d entries differ, first at %s: %r, expected %r" % (len(where), want.size, at, got[at], want[at])


def same(what, got, want):
    """[] when `got` equals the reference cast to fp32 bit for bit, else one line that names the first difference."""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want).astype(np.float32)
    if got.dtype == np.float32 and np.array_equal(got, want):
        return []
    return ["%s: %s" % (what, first_difference(got, want))]


def run(case, x, a, G, m=None):
    """The three forwards and the backward of one model on device tensors: (train logits, eval logits, layer
    logits, [h], {name: grad})."""
    m = package_model(case) if m is None else m
    m.train()
    m.zero_grad()
    out = m(x, a)
    (out * G).sum().backward()
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
    with torch.no_grad():
        out_eval = m.eval()(x, a)
    out_layers, hs = gcn_forward_layers(m, x, a)
    return out.detach(), out_eval, out_layers, hs, grads


def compare(res, r, sl=slice(None), grads=None):
    """Mismatches of run()'s result against the reference `r` (graphs `sl`; `grads`: the expected gradients when they
    are not the whole batch's)."""
    out, out_eval, out_layers, hs, g = res
    bad = same("logits (training forward)", out, r["logits"][sl])
    bad += same("logits (eval, no_grad)", out_eval, r["logits"][sl])
    bad += same("logits (gcn_forward_layers)", out_layers, r["logits"][sl])
    assert len(hs) == len(r["h"])
    for l, h in enumerate(hs):
        bad += same("h of layer %d" % l, h, r["h"][l][sl])
    want = r["grads"] if grads is None else grads
    assert set(g) == set(want)
    for k in want:
        bad += same("grad " + k, g[k], want[k])
    return bad


def device_inputs(case, form):
    x, G = torch.from_numpy(case.x).cuda(), torch.from_numpy(case.G).cuda()
    a = torch.from_numpy(case.A).cuda()
    if form == "sparse":
        a = compress_adjacency(a)
        assert isinstance(a, SparseAdjacency)
    return x, a, G


def check_case(name, form):
    case, r = ex.get(name)
    x, a, G = device_inputs(case, form)
    bad = compare(run(case, x, a, G), r)
    assert not bad, "\n".join([name + " (" + form + ")"] + bad)
    return case, r, a


# ---- the corners of the envelope ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["idle_gcrn_graphconv_129_85_200_86", "idle_gcn_graphconv_255_128_256",
                                  "idle_gcn_selfint_86_256_85_129", "idle_staged_gcn_selfint_129_85_86_129"])
def test_idle_thread_widths(hip, name, form):
    """Widths above 128 (one row per pass, the threads at tid >= dout idle) and 85 / 86 / 129 (1 to 127 idle threads
    per pass), each as din and as dout; the last case with the layer's weights staged in LDS."""
    check_case(name, form)


@pytest.mark.parametrize("form", FORMS)
def test_widest_net(hip, form):
    """F = 64, [256, 256], GCRN: cin = 320, more than the 256 threads, at the largest N the library accepts (the
    forward reads x from global memory there) and at N = 58, the largest at which it stages x in LDS."""
    case, _, _ = check_case("widest_gcrn_selfint_f64_256_256", form)
    assert case.dims[0] + case.F == 320 and not _lib.gcn_supported(case.N + 1, case.F, 256, 1)
    check_case("widest_gcrn_selfint_f64_256_256_x_staged", form)


@pytest.mark.parametrize("form", FORMS)
def test_most_nodes(hip, form):
    """N = 4096; the dense row and the dense column make the list width 4096."""
    case, _, a = check_case("nodes_4096", form)
    if form == "sparse":
        assert a.width == 4096 and int(a.row_cnt.max()) == 4096 and int(a.col_cnt.max()) == 4096


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["f64_gcrn_selfint_8_16_x_staged", "f64_gcrn_selfint_8_16_x_global",
                                  "f64_gcrn_selfint_8_16_largest_n", "f1_gcn_graphconv_8_12_16"])
def test_feature_extremes(hip, name, form):
    """F = 64 on a narrow GCRN net at N = 181, the largest at which the forward stages x in LDS, at 182, where it
    reads x from global memory, and at the largest N the library accepts for it; and F = 1 with GraphConv."""
    case, _, _ = check_case(name, form)
    if name.endswith("_largest_n"):
        assert not _lib.gcn_supported(case.N + 1, case.F, max(case.dims), 1)


@pytest.mark.parametrize("form", FORMS)
def test_f64_at_200_nodes(hip, form):
    """(200, 2, 64, [8, 16], gcrn, selfint).  The forward's two [N][(16 + 64) | 1] row buffers and x [N][64] would
    take 200 * (2 * 81 + 64) * 4 = 180 800 bytes of LDS against the 163 840 of a CU: it keeps the row buffers there
    (129 600 bytes) and reads x from global memory."""
    check_case("f64_gcrn_selfint_8_16", form)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ex.LDS_PAIRS + ["lds_gcrn_selfint_64_64_staged"])
def test_lds_limit_runs(hip, name, form):
    """The largest N the library accepts for three (F, dims) pairs, where the weights are not staged beside the row
    buffers (and, for the first two, neither is x), and [64, 64] at N = 37, where they are."""
    case, _, _ = check_case(name, form)
    if name.endswith("_max"):
        assert not _lib.gcn_supported(case.N + 1, case.F, max(case.dims), 1)


@pytest.mark.parametrize("name", ex.LDS_PAIRS)
def test_lds_limit_refuses_one_more_node(hip, name):
    kw = ex.resolve(name)
    N, F = kw["N"] + 1, kw["F"]
    cls = GCRNBinaryClassifier if kw["kind"] == "gcrn" else GCNBinaryClassifier
    m = cls(F, kw["dims"]).cuda()
    x, a = torch.zeros(1, N, F, device="cuda"), torch.zeros(1, N, N, device="cuda")
    with pytest.raises(RuntimeError, match="LDS"):
        m(x, a)
    with torch.no_grad(), pytest.raises(RuntimeError, match="LDS"):
        m.eval()(x, compress_adjacency(a))
    with pytest.raises(RuntimeError, match="LDS"):
        gcn_forward_layers(m, x, a)


@pytest.mark.parametrize("form", FORMS)
def test_many_graphs(hip, form):
    """B = 70 000: the grid exceeds 65 535 workgroups and k_gcn_reduce sums 70 000 partials."""
    case, _, _ = check_case("graphs_70000", form)
    assert case.B > 65535


# ---- degenerate inputs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_no_graphs(hip, form):
    """B = 0: compression of a [0, N, N] tensor, logits of shape [0, N], all-zero gradients."""
    case, _ = ex.get("slices")
    N, F = case.N, case.F
    a = torch.zeros(0, N, N, device="cuda")
    if form == "sparse":
        a = compress_adjacency(a)
        assert len(a) == 0 and a.shape == (0, N, N) and a.width == 1
        assert a.to_dense().shape == (0, N, N)
    x, G = torch.zeros(0, N, F, device="cuda"), torch.zeros(0, N, device="cuda")
    m = package_model(case)
    out, out_eval, out_layers, hs, grads = run(case, x, a, G, m)
    for o in (out, out_eval, out_layers):
        assert tuple(o.shape) == (0, N) and o.dtype == torch.float32
    assert [tuple(h.shape) for h in hs] == [(0, N, d) for d in case.dims]
    for n, p in m.named_parameters():
        assert grads[n].shape == p.shape and not grads[n].any(), n


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["one_node", "holes"])
def test_degenerate(hip, name, form):
    """B = 1 with N = 1; an adjacency with empty rows and empty columns and entries at index N - 1."""
    case, _, a = check_case(name, form)
    if name == "holes":
        N = case.N
        assert not case.A[:, 0].any() and not case.A[:, :, 1].any() and case.A[:, N - 1, N - 1].all()
        if form == "sparse":
            assert int(a.row_cnt[:, 0].sum()) == 0 and int(a.col_cnt[:, 1].sum()) == 0
            assert int(a.row_cnt[:, N - 2].sum()) == 0 and int(a.col_cnt[:, 6].sum()) == 0


# ---- ballot and list boundaries ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("N", [63, 64, 65, 257])
def test_ballot_boundaries(hip, N, form):
    """A full row and a full column of N = 63, 64, 65, 257 entries: one short of a 64-lane ballot, exactly one, one
    past it (the entry at j = 64), and four ballots and one."""
    case, _, a = check_case("ballot_%d" % N, form)
    if form == "sparse":
        assert a.width == N and int(a.row_cnt[0, N // 2]) == N and int(a.col_cnt[0, N // 3]) == N


@pytest.mark.parametrize("form", FORMS)
def test_lists_of_64_and_65_entries(hip, form):
    """Rows and columns that hold exactly 64 and exactly 65 entries, and a row and a column whose one entry sits at
    index 64."""
    case, _, a = check_case("ballot_257_lists_64_65", form)
    N = case.N
    nz = case.A != 0
    assert nz.sum(-1)[:, N - 3:].tolist() == [[64, 65, 1]] * case.B
    assert nz.sum(-2)[:, N - 3:].tolist() == [[64, 65, 1]] * case.B
    assert nz[:, N - 1, 64].all() and nz[:, 64, N - 1].all() and nz[:, N - 2, 64].all() and nz[:, 64, N - 2].all()
    if form == "sparse":
        assert a.width == 65
        assert a.row_cnt[:, N - 3:].tolist() == [[64, 65, 1]] * case.B
        assert a.col_cnt[:, N - 3:].tolist() == [[64, 65, 1]] * case.B
        assert a.row_idx[:, N - 2, 64].tolist() == [64] * case.B and a.row_idx[:, N - 1, 0].tolist() == [64] * case.B
        assert a.col_idx[:, N - 2, 64].tolist() == [64] * case.B and a.col_idx[:, N - 1, 0].tolist() == [64] * case.B
        assert torch.equal(a.to_dense(), torch.from_numpy(case.A).cuda())
        assert torch.equal(a.to_dense(transposed=True), torch.from_numpy(case.A).cuda())


# ---- dead units, slices, depth -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_dead_units(hip, form):
    """Two units of every layer have a bias of -100: h is exactly 0 there and so are the matching gradient rows."""
    case, r = ex.get("dead_units")
    assert len(case.dead) == 2
    x, a, G = device_inputs(case, form)
    res = run(case, x, a, G)
    bad = compare(res, r)
    assert not bad, "\n".join(bad)
    _, _, _, hs, grads = res
    dead = list(case.dead)
    for l, h in enumerate(hs):
        assert not h[..., dead].any(), l
    for n, g in grads.items():
        if not n.startswith("classifier"):
            assert not g[dead].any(), n                          # the unit's own weight rows and bias
        if n.endswith("weight") and not n.startswith("feature_extractor"):
            assert not g[..., dead].any(), n                     # what reads the unit's h (the first columns of hin)


def test_slices(hip):
    """adj[1:B-1] with the matching x and G slices equals a fresh compression of the same graphs, bit for bit, and
    the reference's slice."""
    case, r = ex.get("slices")
    B = case.B
    assert B >= 4
    sl = slice(1, B - 1)
    x, adj, G = device_inputs(case, "sparse")
    part = adj[sl]
    assert len(part) == B - 2 and part.row_idx.data_ptr() == adj.row_idx[1].data_ptr()
    own = compress_adjacency(torch.from_numpy(case.A[sl].copy()).cuda())
    # the reference's gradients of these graphs alone (the loss is a plain sum over the graphs)
    sub = ex._run(case.model, torch.from_numpy(case.x[sl]), torch.from_numpy(case.A[sl]), torch.from_numpy(case.G[sl]),
                  torch.float64)
    assert np.array_equal(sub["logits"], r["logits"][sl])
    m = package_model(case)
    xs, Gs = x[sl], G[sl]
    res_view = run(case, xs, part, Gs, m)
    res_own = run(case, xs, own, Gs, m)
    bad = compare(res_view, r, sl, sub["grads"]) + compare(res_own, r, sl, sub["grads"])
    assert not bad, "\n".join(bad)
    for v, o in zip(res_view[:3], res_own[:3]):
        assert torch.equal(v, o)
    for k in res_view[4]:
        assert torch.equal(res_view[4][k], res_own[4][k]), k


@pytest.mark.parametrize("form", FORMS)
def test_deepest_exact_net(hip, form):
    """Four graph-convolution layers of width 8: the deepest net whose term bound stays below 2^24 (gcn_exact.py)."""
    case, _, _ = check_case("deepest", form)
    assert len(case.dims) - 1 == ex.DEEPEST_LAYERS
