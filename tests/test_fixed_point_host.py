"""gnn_fpga_amd/fixed_point.py and include/gnn_hip_fixed.h without a GPU: the numpy specification against a scalar
restatement in unbounded Python integers, the tables, the quantisation, the overflow modes, the distance to the float64
forward, and the binding."""
import ctypes
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

import fixed_point_cases as fc
from gnn_fpga_amd import (FixedPointFormat, HitGraph, HitGraphBatch, _lib, fixed_forward_numpy, quantize_model)
from gnn_fpga_amd import fixed_point as fp
from oracle import index_numpy

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = list(itertools.product(("trn", "rnd"), ("wrap", "sat")))


# ---- the scalar restatement: plain Python ints, loops, nothing shared with the specification but the format ------------
def _rint_half_even(v):
    fl = math.floor(v)
    d = v - fl
    if d > 0.5 or (d == 0.5 and fl % 2):
        return fl + 1
    return fl


def _quant(v, f):
    v = float(v)
    if math.isnan(v):
        return 0
    lo, hi = -(1 << (f.total_bits - 1)), (1 << (f.total_bits - 1)) - 1
    if math.isinf(v):
        return hi if v > 0 else lo
    return min(max(_rint_half_even(v * 2.0 ** (f.total_bits - f.int_bits)), lo), hi)


class _Scalar:
    def __init__(self, f, n_iters):
        self.f, self.W, self.Fb = f, f.total_bits, f.total_bits - f.int_bits
        self.lo, self.hi = -(1 << (self.W - 1)), (1 << (self.W - 1)) - 1
        n = 1 << f.table_bits
        self.t_tanh = [_quant(math.tanh(-4 + 8 * i / n), f) for i in range(n)]
        self.t_sig = [_quant(1 / (1 + math.exp(-(-8 + 16 * i / n))), f) for i in range(n)]
        self.counts = [[0] * 6 for _ in range(n_iters + 1)]

    def requant(self, acc, row, col):
        if self.f.rounding == "rnd" and self.Fb > 0:
            acc += 1 << (self.Fb - 1)
        k = acc >> self.Fb                      # Python's >> floors
        if k < self.lo or k > self.hi:
            self.counts[row][col] += 1
            if self.f.overflow == "sat":
                k = self.lo if k < self.lo else self.hi
            else:
                k &= (1 << self.W) - 1
                if k >= 1 << (self.W - 1):
                    k -= 1 << self.W
        return k

    def look(self, table, k, s):
        idx = ((k << s) >> self.Fb) + (1 << (self.f.table_bits - 1))
        return table[min(max(idx, 0), (1 << self.f.table_bits) - 1)]

    def tanh(self, k):
        return self.look(self.t_tanh, k, self.f.table_bits - 3)

    def sig(self, k):
        return self.look(self.t_sig, k, self.f.table_bits - 4)


def scalar_forward(X, src, dst, weights, T, f):
    m = _Scalar(f, T)
    Win, bin_, W1, b1, W2, b2, W3, b3, W4, b4 = [[[_quant(v, f) for v in row] for row in np.atleast_2d(w)] for w in weights]
    bin_, b1, b2, b3, b4 = bin_[0], b1[0], b2[0], b3[0], b4[0]
    N, F, D, E, Fb = len(X), len(X[0]), len(Win), len(src), m.Fb
    C = D + F
    x = [[_quant(v, f) for v in row] for row in X]
    dot = lambda w, v: sum(a * b for a, b in zip(w, v))          # noqa: E731
    H = [[m.tanh(m.requant(dot(Win[d], x[n]) + (bin_[d] << Fb), 0, 0)) for d in range(D)] + x[n] for n in range(N)]
    e_trace, H_trace = [], []
    for t in range(T + 1):
        H_trace.append([row[:] for row in H])
        e = []
        for j in range(E):
            pair = (H[src[j]] + H[dst[j]]) if src[j] >= 0 else [0] * (2 * C)
            a = [m.tanh(m.requant(dot(W1[d], pair) + (b1[d] << Fb), t, 1)) for d in range(D)]
            e.append(m.sig(m.requant(dot(W2[0], a) + (b2[0] << Fb), t, 2)))
        e_trace.append(e)
        if t == T:
            break
        Hn = []
        for n in range(N):
            mi = [m.requant(sum(e[j] * H[src[j]][c] for j in range(E) if dst[j] == n), t, 3) for c in range(C)]
            mo = [m.requant(sum(e[j] * H[dst[j]][c] for j in range(E) if src[j] == n), t, 3) for c in range(C)]
            M = mi + mo + H[n]
            q = [m.tanh(m.requant(dot(W3[d], M) + (b3[d] << Fb), t, 4)) for d in range(D)]
            Hn.append([m.tanh(m.requant(dot(W4[d], q) + (b4[d] << Fb), t, 5)) for d in range(D)] + x[n])
        H = Hn
    return e_trace, H_trace, m.counts


def _small_case():
    rng = np.random.default_rng(7)
    N, E, F, D = 12, 30, 3, 4
    X = rng.uniform(-2.0, 2.0, size=(N, F)).astype(np.float32)
    src, dst = rng.integers(0, N, size=E), rng.integers(0, N, size=E)
    src[[4, 17]] = dst[[4, 17]] = -1
    C = F + D
    shapes = ((D, F), (D,), (D, 2 * C), (D,), (1, D), (1,), (D, 3 * C), (D,), (D, D), (D,))
    weights = [rng.uniform(-0.9, 0.9, size=s).astype(np.float32) for s in shapes]
    return X, src.astype(np.int32), dst.astype(np.int32), weights


@pytest.mark.parametrize("rounding,overflow", PAIRS)
@pytest.mark.parametrize("W,I", [(8, 3), (16, 6), (24, 2), (6, 4)])
def test_specification_equals_the_scalar_restatement(W, I, rounding, overflow):
    X, src, dst, weights = _small_case()
    f = FixedPointFormat(W, I, rounding, overflow, 8)
    out = fixed_forward_numpy(X, src, dst, weights, 2, f)
    e_trace, H_trace, counts = scalar_forward(X.tolist(), src.tolist(), dst.tolist(), weights, 2, f)
    assert out.e_trace.tolist() == e_trace
    assert out.H_trace.tolist() == H_trace
    assert out.counts.tolist() == counts
    assert out.raw.tolist() == e_trace[2] and out.raw.dtype == np.int32 and out.scores.dtype == np.float32
    assert out.scores.tolist() == [k * 2.0 ** -(W - I) for k in e_trace[2]]
    assert out.counts.shape == (3, 6) and not out.counts[2, [0, 3, 4, 5]].any() and not out.counts[1:, 0].any()


def test_the_small_case_exercises_overflow_and_both_modes():
    """The restatement is only a check of requant's overflow branch if the case overflows somewhere."""
    X, src, dst, weights = _small_case()
    totals = {o: fixed_forward_numpy(X, src, dst, weights, 2, FixedPointFormat(24, 2, "trn", o, 8)).counts.sum(axis=0)
              for o in ("wrap", "sat")}
    print(totals)
    for t in totals.values():               # the input stage, an edge stage, the aggregate and a node stage
        assert t[0] > 0 and t[1] > 0 and t[3] > 0 and t[4] > 0
    assert (src < 0).sum() == 2


# ---- tables -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tb", [4, 7, 10, 12])
@pytest.mark.parametrize("W,I", [(8, 3), (16, 6), (24, 2), (6, 4), (12, 12), (24, 8), (4, 2)])
def test_table_facts(W, I, tb):
    f = FixedPointFormat(W, I, table_bits=tb)
    t_tanh, t_sig = fp.activation_tables(f)
    assert t_tanh.shape == t_sig.shape == (1 << tb,) and t_tanh.dtype == np.int64
    assert t_tanh[1 << (tb - 1)] == 0
    if f.frac_bits >= 1:
        assert t_sig[1 << (tb - 1)] == 1 << (f.frac_bits - 1)
    assert np.all(np.diff(t_tanh) >= 0) and np.all(np.diff(t_sig) >= 0)
    assert t_tanh.min() >= f.lo and t_tanh.max() <= f.hi and t_sig.min() >= 0 and t_sig.max() <= 1 << f.frac_bits


# ---- quantisation -------------------------------------------------------------------------------------------------------
def test_masks_give_exact_zeros():
    from gnn_fpga_amd.model import SegmentClassifier
    torch.manual_seed(3)
    F, D = 3, 8
    C = F + D
    g = torch.Generator().manual_seed(4)
    masks_e = [(torch.rand(D, 2 * C, generator=g) < 0.5).float(), (torch.rand(1, D, generator=g) < 0.5).float()]
    masks_n = [(torch.rand(D, 3 * C, generator=g) < 0.5).float(), (torch.rand(D, D, generator=g) < 0.5).float()]
    m = SegmentClassifier(F, D, 2, masks_e=masks_e, masks_n=masks_n)
    with torch.no_grad():                   # a mask must win over a weight that is large where it is zero
        for lin in (m.edge_network.network[0], m.node_network.network[0]):
            lin.weight.add_(3.0)
    q = fp.quantize_weights(m.effective_weights(), FixedPointFormat(16, 6))
    for i, mask in zip((2, 4, 6, 8), masks_e + masks_n):
        dead = mask.numpy() == 0
        assert dead.any() and not q[i][dead].any() and q[i][~dead].any()


def test_quantisation_rounds_half_to_even_and_saturates():
    f = FixedPointFormat(8, 3)              # Fb = 5: one step is 1 / 32
    v = np.array([0.5 / 32, 1.5 / 32, 2.5 / 32, -0.5 / 32, -1.5 / 32, 100.0, -100.0, 127.4 / 32])
    assert fp.quantize(v, f).tolist() == [0, 2, 2, 0, -2, 127, -128, 127]
    sat = FixedPointFormat(8, 3, overflow="wrap")
    assert fp.quantize(np.array([100.0]), sat).tolist() == [127]          # whatever `overflow` says


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_weight_that_is_not_finite_raises(bad):
    _, _, _, weights = _small_case()
    weights[6] = weights[6].copy()
    weights[6][1, 2] = bad
    with pytest.raises(ValueError, match="finite"):
        fp.quantize_weights(weights, FixedPointFormat(16, 6))
    with pytest.raises(ValueError, match="finite"):
        fixed_forward_numpy(*_small_case()[:3], weights, 1, FixedPointFormat(16, 6))


def test_nan_and_infinite_inputs():
    f = FixedPointFormat(12, 4)
    X = np.array([[np.nan, np.inf, -np.inf]], dtype=np.float32)
    assert fp.quantize(X, f).tolist() == [[0, f.hi, f.lo]]
    _, _, _, weights = _small_case()
    out = fixed_forward_numpy(X, np.zeros(0, np.int32), np.zeros(0, np.int32), weights, 0, f)
    assert out.H_trace[0, 0, 4:].tolist() == [0, f.hi, f.lo]


def test_format_validation():
    assert FixedPointFormat()._key() == (16, 6, "trn", "wrap", 10)
    assert FixedPointFormat(24, 24).frac_bits == 0 and FixedPointFormat(4, 2).lo == -8 and FixedPointFormat(4, 2).hi == 7
    for kw in (dict(total_bits=3), dict(total_bits=25), dict(int_bits=1), dict(total_bits=8, int_bits=9),
               dict(rounding="nearest"), dict(overflow="clip"), dict(table_bits=3), dict(table_bits=13),
               dict(total_bits=8.5)):
        with pytest.raises(ValueError):
            FixedPointFormat(**kw)
    f = FixedPointFormat(8, 3)
    with pytest.raises(AttributeError):
        f.total_bits = 9
    assert f == FixedPointFormat(8, 3) and f != FixedPointFormat(8, 4) and len({f, FixedPointFormat(8, 3)}) == 1


# ---- the overflow condition -----------------------------------------------------------------------------------------------
def test_star_graph_overflows_and_the_modes_differ():
    """Hit 0 sums 130 products: at three integer bits the aggregate leaves the word.  (Measured on the host with this
    specification: 47 overflows, all in the aggregate stage; 300 of 306 raw scores differ between the modes.)"""
    g = fc.cached_star()
    w = fc.host_weights(fc.default_model(3, 8, 3))
    wrap, sat = fc.spec(g, w, 3, fc.fmt(16, 3, overflow="wrap")), fc.spec(g, w, 3, fc.fmt(16, 3, overflow="sat"))
    assert g.src.size == 306 and (g.src < 0).sum() == 6
    assert wrap.counts.sum() > 0 and sat.counts.sum() > 0 and wrap.counts[:, 3].sum() > 0
    assert int((wrap.raw != sat.raw).sum()) > 306 // 2
    assert np.array_equal(wrap.e_trace[0], sat.e_trace[0])          # nothing has overflowed before the first sum


# ---- distance to the float64 forward -----------------------------------------------------------------------------------
# max |score - float64 score| measured on the host with this specification (layered_graph(70, 150, 3, seed=1), torch's
# default initialisation under manual_seed(0), hidden_dim 8, 3 iterations, trn / wrap)
MEASURED = {(24, 8, 12): 1.0172e-3, (24, 8, 10): 4.0297e-3, (8, 3, 8): 2.7842e-2}


def test_distance_to_the_float64_forward():
    g = fc.layered()
    m = fc.default_model(3, 8, 3)
    w = fc.host_weights(m)
    params = {k: v.detach().numpy() for k, v in m.state_dict().items()}
    ref = index_numpy.segment_classifier(g.X, g.src, g.dst, params, 3, dtype=np.float64)
    err = {}
    for (W, I, tb), measured in MEASURED.items():
        out = fc.spec(g, w, 3, fc.fmt(W, I, tb=tb))
        err[W, I, tb] = float(np.abs(out.scores.astype(np.float64) - ref).max())
        print("(%d, %d) table_bits %d: max |fixed - float64| = %.4e (measured %.4e)" % (W, I, tb, err[W, I, tb], measured))
        assert not out.counts.any()
    assert err[24, 8, 12] < err[24, 8, 10] < err[8, 3, 8]
    for k, measured in MEASURED.items():
        assert err[k] <= 2 * measured, (k, err[k])


# ---- header, binding, arguments ------------------------------------------------------------------------------------------
def _declared():
    text = open(os.path.join(REPO, "include", "gnn_hip_fixed.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gnn_fx_[a-z0-9_]+)\s*\(", text)))


def test_header_binding_and_library_export_the_same_names():
    names = _declared()
    assert len(names) == 3 and sorted(_lib.FX_SIGNATURES) == names
    assert not set(_lib.FX_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.ITER_SIGNATURES))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), n
    src = open(os.path.join(REPO, "gnn-fpga_amd", "csrc", "fixed_point.hip")).read()
    assert sorted(set(re.findall(r"^(?:int|size_t) (gnn_fx_[a-z0-9_]+)\(", src, flags=re.M))) == names
    mk = open(os.path.join(REPO, "gnn-fpga_amd", "csrc", "Makefile")).read()
    assert "fixed_point" in re.search(r"^UNITS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    assert re.search(r"^\$\(ROOT\)/build/fixed_point\.o: \$\(ROOT\)/include/gnn_hip_fixed\.h$", mk, re.M)
    hdr = open(os.path.join(REPO, "include", "gnn_hip_fixed.h")).read()
    for decl in re.findall(r"/\*(?:(?!\*/).)*\*/\s*(?:int|size_t) gnn_fx_", hdr, flags=re.S):
        assert re.search(r"gnn/model\.py:\d+", decl), decl[:80]         # every declaration cites the reference
    assert _lib.GNN_FX_ROUNDING == {"trn": 0, "rnd": 1} and _lib.GNN_FX_OVERFLOW == {"wrap": 0, "sat": 1}
    for name, value in (("GNN_FX_TRN", 0), ("GNN_FX_RND", 1), ("GNN_FX_WRAP", 0), ("GNN_FX_SAT", 1), ("GNN_FX_STAGES", 6)):
        assert re.search(r"#define %s\s+%d\b" % (name, value), hdr), name
    assert _lib.GNN_ABI_VERSION == 7


def test_struct_layouts_match_the_header():
    assert ctypes.sizeof(_lib.GnnFxFormat) == 20
    assert ctypes.sizeof(_lib.GnnFxParams) == 10 * ctypes.sizeof(ctypes.c_void_p) + 8
    assert ctypes.sizeof(_lib.GnnFxTables) == 2 * ctypes.sizeof(ctypes.c_void_p)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gnn_hip_fixed.h")).read(), flags=re.S)
    body = re.search(r"typedef struct gnn_fx_format \{(.*?)\}", hdr, re.S).group(1)
    assert re.findall(r"int32_t (\w+);", body) == [n for n, _ in _lib.GnnFxFormat._fields_]


def test_supported_and_workspace_answer_without_a_gpu():
    lib = _lib.load()
    for F, D in [(2, 4), (3, 8), (2, 32), (11, 8), (4, 16), (3, 64), (4, 64), (11, 16)]:
        assert lib.gnn_shape_supported(F, D) and lib.gnn_fx_supported(F, D, 16, 6, 10), (F, D)
        assert lib.gnn_fx_supported(F, D, 24, 2, 12) and lib.gnn_fx_supported(F, D, 4, 2, 4)
    assert not lib.gnn_fx_supported(5, 7, 16, 6, 10)
    for W, I, tb in [(3, 2, 10), (25, 6, 10), (16, 1, 10), (16, 17, 10), (16, 6, 3), (16, 6, 13)]:
        assert not lib.gnn_fx_supported(3, 8, W, I, tb), (W, I, tb)
    small, big = _lib.fx_workspace_bytes(10, 20, 3, 8), _lib.fx_workspace_bytes(1000, 5000, 3, 8)
    # two hit tables, mi | mo, P | Q as int64 and one score per segment - at least
    assert small >= 10 * 12 * 4 * 4 + 10 * 16 * 8 + 20 * 4 and big > small
    assert _lib.fx_workspace_bytes(0, 0, 3, 8) > 0
    assert _lib.fx_workspace_bytes(-1, 0, 3, 8) == 0 and b"n_hits" in lib.gnn_last_error()
    assert _lib.fx_workspace_bytes(10, 20, 5, 7) == 0 and b"input_dim=5" in lib.gnn_last_error()


def test_bad_arguments_give_their_errors():
    lib = _lib.load()
    g, p, t = _lib.GnnGraph(), _lib.GnnFxParams(), _lib.GnnFxTables()
    p.F, p.D = 3, 8
    f = _lib.fx_format_struct(16, 6, "trn", "wrap", 10)
    call = lambda g_, p_, f_, t_, T=1: lib.gnn_fx_forward(g_, p_, f_, t_, T, None, None, None, None, None, None, 0, None)  # noqa: E731
    assert call(None, p, f, t) == _lib.GNN_ERR_BADARG and b"null" in lib.gnn_last_error()
    assert call(g, p, f, t, -1) == _lib.GNN_ERR_BADARG and b"n_iters" in lib.gnn_last_error()
    g.n_hits = -1
    assert call(g, p, f, t) == _lib.GNN_ERR_BADARG and b"n_hits" in lib.gnn_last_error()
    g.n_hits = 0
    assert call(g, p, _lib.GnnFxFormat(16, 6, 2, 0, 10), t) == _lib.GNN_ERR_BADARG and b"rounding" in lib.gnn_last_error()
    assert call(g, p, _lib.GnnFxFormat(16, 6, 0, 5, 10), t) == _lib.GNN_ERR_BADARG and b"overflow" in lib.gnn_last_error()
    assert call(g, p, _lib.GnnFxFormat(30, 6, 0, 0, 10), t) == _lib.GNN_ERR_UNSUPPORTED
    p.D = 7
    assert call(g, p, f, t) == _lib.GNN_ERR_UNSUPPORTED and b"hidden_dim=7" in lib.gnn_last_error()
    p.D = 8
    assert call(g, p, f, t) == _lib.GNN_ERR_BADARG and b"weight pointer" in lib.gnn_last_error()
    with pytest.raises(KeyError):
        _lib.fx_format_struct(16, 6, "nearest", "wrap", 10)


def test_no_cpu_path_and_no_other_activation():
    from torch import nn
    m = fc.default_model(3, 8, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        quantize_model(m, FixedPointFormat())
    with pytest.raises(TypeError):
        quantize_model(m, (16, 6))
    m.node_network.network[1] = nn.ReLU()
    with pytest.raises(NotImplementedError, match="ReLU"):
        quantize_model(m, FixedPointFormat())


def test_list_length_bound_raises():
    """Every per-hit list must be shorter than 2^(65 - 2 W) entries: 131 072 at 24 bits."""
    f = FixedPointFormat(24, 8)
    assert f.max_list_entries == 131072 and FixedPointFormat(16, 6).max_list_entries == 1 << 33
    _, _, _, weights = _small_case()
    n = f.max_list_entries
    X = np.zeros((3, 3), dtype=np.float32)
    src, dst = np.ones(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    with pytest.raises(ValueError, match="131072"):
        fixed_forward_numpy(X, src, dst, weights, 1, f)
    with pytest.raises(ValueError, match="131072"):
        fixed_forward_numpy(X, dst, src, weights, 1, f)             # the out list
    out = fixed_forward_numpy(X, src[:-1], dst[:-1], weights, 1, f)  # one entry fewer: exact, and it runs
    assert out.raw.shape == (n - 1,)
    fp._refuse_long_lists(n - 1, f)
    with pytest.raises(ValueError):
        fp._refuse_long_lists(n, f)


def test_star_graph_is_what_the_tests_say():
    g = fc.cached_star()
    ok = g.src >= 0
    deg_in, deg_out = np.bincount(g.dst[ok], minlength=140), np.bincount(g.src[ok], minlength=140)
    assert g.X.shape == (140, 3) and deg_in[0] == 130 and deg_out[0] == 130 and (~ok).sum() == 6
    assert not (deg_in[136:] + deg_out[136:]).any() and np.all(g.src[ok] != g.dst[ok])
    b = HitGraphBatch.from_graphs([HitGraph(g.X, g.src, g.dst, g.y)])
    assert b.n_segments == 306 and int(b.in_ptr[1]) == 130
