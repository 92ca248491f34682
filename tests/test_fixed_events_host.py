"""The one-launch fixed-point forward (include/gnn_hip_fixed_events.h, csrc/fixed_events.hip) without a GPU: its names in
the header, the binding, the library and the build; the LDS byte counts its route decision rests on; its refusals; the
route rule `call_route.choose_fixed`; the build's resource remarks; and the statement the per-graph overflow counters
rest on - the specification run on a graph's slice gives that slice of the batch's result."""
import ctypes
import os
import re

import numpy as np
import pytest

import fixed_events_cases as fe
from gnn_fpga_amd import FixedPointFormat, _lib
from gnn_fpga_amd import call_route as cr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "gnn_hip_fixed_events.h")
SHAPES = [(2, 4), (2, 8), (2, 16), (2, 32), (3, 4), (3, 8), (3, 16), (3, 32), (3, 64), (4, 8), (4, 16), (4, 32), (4, 64),
          (11, 4), (11, 8), (11, 16)]
LDS_LIMIT = 160 * 1024


# ---- names and build ---------------------------------------------------------------------------------------------------
def test_header_binding_library_and_build_agree():
    hdr = open(HEADER).read()
    names = sorted(set(re.findall(r"\b(gnn_fxev_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert names == ["gnn_fxev_forward", "gnn_fxev_lds_bytes", "gnn_fxev_supported"] == sorted(_lib.FXEV_SIGNATURES)
    assert not set(_lib.FXEV_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.ITER_SIGNATURES) | set(_lib.FX_SIGNATURES))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), n
    src = open(os.path.join(REPO, "gnn-fpga_amd", "csrc", "fixed_events.hip")).read()
    assert sorted(set(re.findall(r"^(?:int|size_t) (gnn_fxev_[a-z0-9_]+)\(", src, flags=re.M))) == names
    mk = open(os.path.join(REPO, "gnn-fpga_amd", "csrc", "Makefile")).read()
    assert "fixed_events" in re.search(r"^UNITS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    assert re.search(r"^\$\(ROOT\)/build/fixed_events\.o: \$\(ROOT\)/include/gnn_hip_fixed\.h "
                     r"\$\(ROOT\)/include/gnn_hip_fixed_events\.h$", mk, re.M)
    decls = re.findall(r"/\*(?:(?!\*/).)*\*/\s*(?:int|size_t) gnn_fxev_", hdr, flags=re.S)
    assert len(decls) == 3
    for decl in decls:
        assert re.search(r"gnn/model\.py:\d+", decl), decl[:80]         # every declaration cites the reference
    assert '#include "gnn_hip_fixed.h"' in hdr and _lib.GNN_ABI_VERSION == 7


# ---- gnn_fxev_lds_bytes / gnn_fxev_supported ---------------------------------------------------------------------------
def _layout_bytes(F, D, tb, nh, ns):
    """DESIGN.md's formula: P | Q as int64 (4 D words per hit), H, Hn, mi | mo (4 LDH), a score per segment (padded to
    four), the weights with every streamed layer padded to LDH rows, both tables, the overflow total, the local ids."""
    ldh = (F + D + 3) & ~3
    weights = F * D + D + 2 * ldh * D + D + D + 4 + 3 * ldh * D + D + D * D + D
    return 4 * (nh * (4 * D + 4 * ldh) + ((ns + 3) & ~3) + weights + 2 * (1 << tb) + 4 + 2 * (nh + 1) + 6 * ns)


def test_lds_bytes_grow_and_decide_supported():
    lib = _lib.load()
    base = _lib.fxev_lds_bytes(11, 8, 10, 35, 142)
    assert 0 < base < _lib.fxev_lds_bytes(11, 8, 10, 36, 142)
    assert base < _lib.fxev_lds_bytes(11, 8, 10, 35, 143 + 3)           # (scores are padded to four)
    assert base < _lib.fxev_lds_bytes(11, 8, 11, 35, 142)
    # at least: two tables of hit rows, mi | mo, P | Q as int64, a score per segment, both tables
    assert base >= 4 * (35 * 4 * 20 + 35 * 4 * 8 + 142 + 2 * 1024)
    for F, D in SHAPES:
        for tb in (4, 10, 12):
            for nh, ns in [(0, 0), (1, 0), (35, 142), (140, 306), (700, 1200), (5000, 50000)]:
                need = _lib.fxev_lds_bytes(F, D, tb, nh, ns)
                assert need == _layout_bytes(F, D, tb, nh, ns)
                want = 0 < need <= LDS_LIMIT and bool(lib.gnn_fx_supported(F, D, 16, 6, tb))
                assert need > 0 and _lib.fxev_supported(F, D, tb, nh, ns) == want, (F, D, tb, nh, ns, need)
    for args in [(11, 8, 12, 35, 142), (3, 8, 10, 140, 306), (2, 32, 10, 40, 144)]:
        assert _lib.fxev_supported(*args), args
    for args in [(2, 32, 10, 140, 306), (3, 64, 12, 140, 306)]:
        assert not _lib.fxev_supported(*args) and _lib.fxev_lds_bytes(*args) > LDS_LIMIT, args
    for args in [(5, 7, 10, 35, 142), (3, 8, 3, 35, 142), (3, 8, 13, 35, 142), (3, 8, 10, -1, 142), (3, 8, 10, 35, -1)]:
        assert not _lib.fxev_supported(*args) and _lib.fxev_lds_bytes(*args) == 0, args
    # the counts the layout is documented with ("Fixed point: small events in one launch")
    assert _lib.fxev_lds_bytes(3, 8, 10, 140, 306) == 65160 and _lib.fxev_lds_bytes(2, 32, 10, 40, 144) == 84136


# ---- refusals: no device needed ----------------------------------------------------------------------------------------
def test_bad_arguments_give_their_errors():
    lib = _lib.load()
    g, p, t = _lib.GnnGraph(), _lib.GnnFxParams(), _lib.GnnFxTables()
    p.F, p.D = 3, 8
    f = _lib.fx_format_struct(16, 6, "trn", "wrap", 10)

    def call(g_=g, p_=p, f_=f, t_=t, n_graphs=1, max_hits=10, max_segments=10, T=1):
        return lib.gnn_fxev_forward(g_, p_, f_, t_, None, None, n_graphs, max_hits, max_segments, T, None, None, None,
                                    None, None, None, None)
    bad, err = _lib.GNN_ERR_BADARG, lib.gnn_last_error
    for kw in ({"g_": None}, {"p_": None}, {"f_": None}, {"t_": None}):
        assert call(**kw) == bad and b"null" in err()
    assert call(n_graphs=-1) == bad and b"n_graphs" in err()
    assert call(T=-1) == bad and b"n_iters" in err()
    assert call(max_hits=-1) == bad and b"max_hits" in err()
    assert call(max_segments=-1) == bad and b"max_segments" in err()
    g.n_hits = -1
    assert call() == bad and b"n_hits" in err()
    g.n_hits = 0
    assert call(f_=_lib.GnnFxFormat(16, 6, 2, 0, 10)) == bad and b"rounding" in err()
    assert call(f_=_lib.GnnFxFormat(16, 6, 0, 5, 10)) == bad and b"overflow" in err()
    assert call(f_=_lib.GnnFxFormat(30, 6, 0, 0, 10)) == _lib.GNN_ERR_UNSUPPORTED and b"total_bits" in err()
    p.D = 7
    assert call() == _lib.GNN_ERR_UNSUPPORTED and b"hidden_dim=7" in err()
    p.D = 8
    # a graph too large for a workgroup: the bytes needed and the limit, before any pointer is looked at
    assert call(max_hits=5000, max_segments=50000) == _lib.GNN_ERR_UNSUPPORTED
    msg = err().decode()
    assert str(_lib.fxev_lds_bytes(3, 8, 10, 5000, 50000)) in msg and str(LDS_LIMIT) in msg and "5000 hits" in msg
    assert call() == bad and b"weight pointer" in err()


# ---- the route rule ------------------------------------------------------------------------------------------------------
def test_choose_fixed_every_clause_flips_the_answer():
    lay = object()
    yes = dict(use_events=True, trace=False, n_graphs=64, layout=lay, fits=True)
    assert cr.choose_fixed(**yes) == "events"
    for k, v in (("use_events", False), ("trace", True), ("n_graphs", 0), ("n_graphs", cr.EVENTS_MAX_GRAPHS + 1),
                 ("layout", None), ("fits", False)):
        assert cr.choose_fixed(**dict(yes, **{k: v})) == "per_module", k
    assert cr.choose_fixed(**dict(yes, n_graphs=1)) == "events"
    assert cr.choose_fixed(**dict(yes, n_graphs=cr.EVENTS_MAX_GRAPHS)) == "events"


# ---- the build's resource remarks ----------------------------------------------------------------------------------------
def test_kernel_resource_remarks():
    path = os.path.join(REPO, "build", "fixed_events.remarks")
    if not os.path.exists(path):
        pytest.fail("build/fixed_events.remarks is missing: build the library first")
    txt = open(path).read()
    seen = set()
    for blk in txt.split("Function Name: ")[1:]:
        m = re.match(r"\S*?k_fx_eventILi(\d+)ELi(\d+)E", blk)
        if m:
            seen.add((int(m.group(1)), int(m.group(2))))
            # one accumulator per lane, everything else in LDS: no scratch at any shape
            assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", blk), blk.split("\n", 1)[0]
    assert seen == set(SHAPES), seen ^ set(SHAPES)


# ---- graph by graph, the specification gives the batch's result ---------------------------------------------------------
@pytest.mark.parametrize("kind", ["mixed600", "mixed600_padded"])
def test_the_specification_is_per_graph(kind):
    """What `graph_overflows` and the one-workgroup-per-graph kernel rest on: no value of a graph depends on another
    graph.  (24, 2, rnd, wrap, 8) at hidden_dim 16 with the weights doubled: most graphs overflow, some do not."""
    hb = fe.host_batch(kind, 11)
    assert hb.n_graphs == 600 and hb.hit_ptr[101] == hb.hit_ptr[100] and hb.seg_ptr[301] - hb.seg_ptr[300] == (
        0 if kind == "mixed600" else hb.dense_shape[2])
    assert int(np.diff(hb.hit_ptr).max()) <= 35 and int(np.diff(hb.seg_ptr).max()) <= 142
    f = FixedPointFormat(24, 2, "rnd", "wrap", 8)
    w = fe.gained(11, 16, 2, 2.0)
    whole, parts = fe.spec(hb, w, 2, f), fe.spec_per_graph(hb, w, 2, f)
    assert np.array_equal(np.concatenate([p.raw for p in parts]), whole.raw)
    assert np.array_equal(sum(p.counts for p in parts), whole.counts)
    per_graph = np.array([int(p.counts.sum()) for p in parts])
    spoiled = int((per_graph > 0).sum())
    print("%s: %d of 600 graphs overflow" % (kind, spoiled))
    assert 500 < spoiled < 600
    if kind == "mixed600":
        assert per_graph[100] == 0 and parts[100].raw.size == 0
    else:       # the empty graph scores its padded segments like any other: sigmoid(W2 tanh(b1) + b2)
        assert parts[100].raw.size == hb.dense_shape[2] and len(set(parts[100].raw.tolist())) == 1
