"""CPU-side checks: the C-ABI library loads and exports every symbol include/gnn_hip.h
declares; host logic (index-form batch, dense adapter, npz loader, module tree)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from golden_util import Fixture
from gnn_fpga_amd import HitGraphBatch, synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_functions():
    text = open(os.path.join(REPO, "include", "gnn_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gnn_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from gnn_fpga_amd import _lib
    names = _declared_functions()
    assert len(names) >= 10
    assert sorted(_lib.SIGNATURES) == names          # binding covers the whole header
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), n
    loaded = _lib.load()                              # no GPU needed for these calls
    assert loaded.gnn_abi_version() == _lib.GNN_ABI_VERSION
    assert loaded.gnn_shape_supported(3, 8) == 1
    assert loaded.gnn_shape_supported(5, 7) == 0
    assert loaded.gnn_h_stride(3, 8) == 12
    assert loaded.gnn_forward_workspace_bytes(10, 20, 3, 8) > 0


def test_no_cpu_fallback_in_product():
    """The product path must not import the oracle or run on CPU tensors."""
    pkg = os.path.join(REPO, "gnn-fpga_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert "import oracle" not in src and "from oracle" not in src, fn
    from gnn_fpga_amd.model import SegmentClassifier
    m = SegmentClassifier(input_dim=3, hidden_dim=8, n_iters=1).eval()
    g = synth.layered_graph(30, 50, 3, seed=0)
    with torch.no_grad(), pytest.raises(RuntimeError):
        m(HitGraphBatch.from_graphs([g]))


def test_module_tree_matches_reference_state_dict():
    from gnn_fpga_amd.model import SegmentClassifier
    fx = Fixture("sector_s0")
    m = SegmentClassifier(input_dim=3, hidden_dim=8, n_iters=4)
    assert list(m.state_dict().keys()) == list(fx.params.keys())
    for k, v in m.state_dict().items():
        assert tuple(v.shape) == fx.params[k].shape
    assert sum(p.numel() for p in m.parameters()) == 569
    assert list(m.named_buffers()) == []
    m.load_state_dict({k: torch.from_numpy(v) for k, v in fx.params.items()})
    # what gnn/estimator.py:54-55 iterates
    assert len([l.weight for l in m.node_network.network if hasattr(l, "weight")]) == 2
    assert len([l.weight for l in m.edge_network.network if hasattr(l, "weight")]) == 2


def test_masked_linear_semantics():
    from gnn_fpga_amd.model import MaskedLinear
    torch.manual_seed(0)
    l = MaskedLinear(6, 4)
    assert l.mask_flag is False
    w0 = l.weight.detach().clone()
    mask = (torch.rand(4, 6) < 0.5).float()
    l.set_mask(mask)
    assert l.mask_flag is True
    assert torch.equal(l.weight.detach(), w0 * mask)          # gnn/model.py:21
    x = torch.randn(3, 6)
    assert torch.allclose(l(x), torch.nn.functional.linear(x, w0 * mask, l.bias))
    assert "mask" not in l.state_dict()


def test_csr_layout_and_on_disk_order():
    g = synth.layered_graph(200, 900, 3, seed=4)
    b = HitGraphBatch.from_graphs([g])
    in_ptr, in_eid, in_nbr = b.in_ptr.numpy(), b.in_eid.numpy(), b.in_nbr.numpy()
    out_ptr, out_eid, out_nbr = b.out_ptr.numpy(), b.out_eid.numpy(), b.out_nbr.numpy()
    for n in range(200):
        seg = in_eid[in_ptr[n]:in_ptr[n + 1]]
        assert np.all(g.dst[seg] == n) and np.all(np.diff(seg) > 0)
        assert np.all(in_nbr[in_ptr[n]:in_ptr[n + 1]] == g.src[seg])
        seg = out_eid[out_ptr[n]:out_ptr[n + 1]]
        assert np.all(g.src[seg] == n) and np.all(np.diff(seg) > 0)
        assert np.all(out_nbr[out_ptr[n]:out_ptr[n + 1]] == g.dst[seg])
    # the reference's on-disk SparseGraph arrays (nonzero() of the dense matrices,
    # gnn/graph.py:23-26) are this CSR order already
    X, Ri, Ro = synth.to_dense(g)
    Ri_rows, Ri_cols = Ri.nonzero()
    Ro_rows, Ro_cols = Ro.nonzero()
    assert np.array_equal(Ri_cols, in_eid) and np.array_equal(Ro_cols, out_eid)
    b2 = HitGraphBatch.from_sparse_arrays(X, Ri_rows, Ri_cols, Ro_rows, Ro_cols)
    for k in ("src", "dst", "in_ptr", "in_eid", "in_nbr", "out_ptr", "out_eid", "out_nbr"):
        assert torch.equal(getattr(b, k), getattr(b2, k)), k


def test_dense_round_trip_and_padding(tmp_path):
    """Dense <-> index round trip (gnn/GraphConstructionDev_mu200.ipynb cell 41-44) and the
    zero-padded batch of gnn/trainSegmentClassifier.py:66-95."""
    gs = [synth.muon_graph(s) for s in range(3)]
    Nmax = max(g.X.shape[0] for g in gs)
    Emax = max(g.src.shape[0] for g in gs)
    dense = [synth.to_dense(g, Nmax, Emax) for g in gs]
    X, Ri, Ro = (torch.from_numpy(np.stack([d[i] for d in dense])) for i in range(3))
    b = HitGraphBatch.from_dense(X, Ri, Ro)
    assert b.dense_shape == (3, Nmax, Emax)
    src = b.src.numpy().reshape(3, Emax)
    dst = b.dst.numpy().reshape(3, Emax)
    for i, g in enumerate(gs):
        E = g.src.shape[0]
        assert np.array_equal(src[i, :E], g.src + i * Nmax)
        assert np.array_equal(dst[i, :E], g.dst + i * Nmax)
        assert np.all(src[i, E:] == -1) and np.all(dst[i, E:] == -1)
    assert int(b.in_ptr[-1]) == sum(g.src.shape[0] for g in gs)
    # npz written with the reference's key schema (gnn/graph.py:179-181)
    g = gs[0]
    Xd, Rid, Rod = synth.to_dense(g)
    rr, rc = Rid.nonzero()
    orr, oc = Rod.nonzero()
    fn = str(tmp_path / "event000000.npz")
    np.savez(fn, X=Xd, Ri_rows=rr, Ri_cols=rc, Ro_rows=orr, Ro_cols=oc, y=g.y)
    bl = HitGraphBatch.from_npz(fn)
    assert np.array_equal(bl.src.numpy(), g.src) and np.array_equal(bl.dst.numpy(), g.dst)


def test_bad_inputs_raise():
    g = synth.layered_graph(30, 50, 3, seed=0)
    with pytest.raises(ValueError):
        HitGraphBatch(g.X, g.src + 100, g.dst)
    with pytest.raises(ValueError):
        HitGraphBatch(g.X, np.where(np.arange(50) == 0, -1, g.src), g.dst)
    X, Ri, Ro = synth.to_dense(g)
    Ri[0, 0] = Ri[1, 0] = 1
    with pytest.raises(ValueError):
        HitGraphBatch.from_dense(X, Ri, Ro)


def test_pipelined_kernels_never_spill():
    """Cfg::pipelined shapes keep asm-loaded registers in flight across a slice; that is only
    legal with zero scratch (a spill would save a register before its load has landed).  The
    compiler's resource remarks of the real build are kept in build/sell_pipeline.remarks."""
    import subprocess
    path = os.path.join(REPO, "build", "sell_pipeline.remarks")
    if not os.path.exists(path):
        pytest.skip("no build remarks (library was built elsewhere)")
    txt = open(path).read()
    blocks = re.split(r"remark: Function Name: ", txt)[1:]
    seen = 0
    for b in blocks:
        name = subprocess.run(["c++filt", b.split()[0]], capture_output=True, text=True).stdout
        m = re.search(r"(k_iter2?)<(\d+), (\d+), (true|false), (true|false)(, (true|false))?>", name)
        if not m:
            continue
        F, D = int(m.group(2)), int(m.group(3))
        if m.group(1) == "k_iter":
            pipelined = (D <= 8 and F <= 3) or D == 4             # mirrors Cfg::pipelined
            if m.group(7) == "true":                              # the training variant (TR) waits for its prefetch
                pipelined = False                                 # at once: nothing asm-loaded is in flight across work
        else:
            pipelined = D <= 8                                    # mirrors Cfg::iter2
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        agprs = int(re.search(r"AGPRs: (\d+)", b).group(1))
        if pipelined:
            seen += 1
            assert agprs == 0, "%s<%d,%d> is pipelined but parks values in AGPRs" % (m.group(1), F, D)
            assert scratch == 0, "%s<%d,%d> is pipelined but spills %d bytes" % (m.group(1), F, D, scratch)
    assert seen >= 20 + 27          # k_iter: 5 shapes x 4 variants; k_iter2: 6 shapes x 4 + 3 fused-first


def test_event_layout_checks_block_diagonality():
    """HitGraphBatch.event_layout: per-graph offsets for the one-workgroup-per-graph kernel, and
    None when a segment crosses a graph boundary (that kernel indexes LDS by local hit id)."""
    graphs = [synth.muon_graph(seed=i) for i in range(5)]
    b = HitGraphBatch.from_graphs(graphs)
    lay = b.event_layout()
    assert lay is not None and lay is b.event_layout()          # cached
    assert lay.hit_ptr.dtype == torch.int32 and lay.hit_ptr.tolist() == b.hit_ptr.tolist()
    assert lay.seg_ptr.tolist() == b.seg_ptr.tolist()
    assert lay.max_hits == max(g.X.shape[0] for g in graphs)
    assert lay.max_segments == max(g.src.shape[0] for g in graphs)
    g = synth.layered_graph(60, 100, 3, seed=2)
    assert HitGraphBatch(g.X, g.src, g.dst).event_layout() is not None      # one graph: trivially fine
    assert HitGraphBatch(g.X, g.src, g.dst, hit_ptr=[0, 30, 60],
                         seg_ptr=[0, 50, 100]).event_layout() is None
    # padded segments (-1) are allowed anywhere
    X, Ri, Ro = synth.to_dense(graphs[0], 40, 200)
    pb = HitGraphBatch.from_dense(torch.from_numpy(X)[None], torch.from_numpy(Ri)[None],
                                  torch.from_numpy(Ro)[None])
    assert pb.event_layout() is not None and pb.event_layout().max_segments == 200


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    """Error behaviour of the C ABI (include/gnn_hip.h: 0 on success, GNN_ERR_* otherwise,
    gnn_last_error() explains): every entry point validates its arguments before it touches the
    device, so this runs on the CPU-only build box."""
    from gnn_fpga_amd import _lib
    lib = _lib.load()
    G, P = _lib.GnnGraph(), _lib.GnnParams()
    P.F, P.D = 3, 8
    G.n_hits, G.n_segments = 5, 7                     # sizes without arrays
    BAD, UNS = _lib.GNN_ERR_BADARG, _lib.GNN_ERR_UNSUPPORTED
    err = lambda: lib.gnn_last_error().decode()
    assert lib.gnn_segclf_forward(None, None, 1, None, None, None, None, 0, None) == BAD and "bad argument" in err()
    assert lib.gnn_segclf_forward(ctypes.byref(G), ctypes.byref(P), -1, None, None, None, None, 0, None) == BAD
    assert lib.gnn_input_fwd(None, None, None, None, 4, 3, 8, 12, None) == BAD
    assert lib.gnn_segclf_forward_events(ctypes.byref(G), ctypes.byref(P), None, None, 2, 5, 7, 1, None, None) == BAD
    assert "offsets" in err()
    assert lib.gnn_bce_loss(None, None, 5, 1.0, None, None, None, None) == BAD
    assert lib.gnn_segclf_forward_plan(None, None, 1, None, None, 0, None) != 0
    # shapes without kernels are reported as unsupported, not run
    P.F, P.D = 5, 7
    assert lib.gnn_events_supported(5, 7, 10, 10) == 0
    assert lib.gnn_events_supported(3, 8, 10 ** 6, 10 ** 7) == 0          # does not fit one workgroup
    assert lib.gnn_events_supported(11, 8, 40, 150) == 1
    assert lib.gnn_plan_shape_supported(5, 7) == 0 and lib.gnn_plan_shape_supported(3, 64) == 1
    lim = (ctypes.c_int32 * 4)()
    assert lib.gnn_plan_limits(5, 7, lim) == UNS and "input_dim=5" in err()
    assert lib.gnn_plan_limits(3, 8, lim) == 0 and lim[0] >= 16 and lim[2] >= 1024
    assert lib.gnn_forward_workspace_bytes(-1, 5, 3, 8) == 0 or True       # size queries never fail hard
    assert lib.gnn_plan_workspace_bytes(10, 20, 5, 7) == 0


def test_csr_is_built_on_first_use_only():
    """The two CSRs are not needed by the tiled pipeline: HitGraphBatch builds them when a consumer
    (per-module kernels, small-event kernel, backward) first asks, also after a device move."""
    g = synth.layered_graph(200, 900, 3, seed=4)
    b = HitGraphBatch.from_graphs([g, g])
    assert b._csr is None
    b.build_plan(8, dict(tile_hits=64, iter_records=40, chunk_segments=50, edge_records=60))
    assert b._csr is None                                   # the plan does not touch them
    b.to("cpu")
    ip, ie, inb = b.in_ptr, b.in_eid, b.in_nbr
    assert b._csr is not None and b._src_host is None
    assert ip.dtype == torch.int32 and ip.shape == (401,) and int(ip[-1]) == 1800
    src, dst = b.src.numpy(), b.dst.numpy()
    assert np.array_equal(inb.numpy(), src[ie.numpy()])
    assert np.all(np.diff(dst[ie.numpy()]) >= 0)            # grouped by end hit
    assert np.array_equal(b.out_nbr.numpy(), dst[b.out_eid.numpy()])


def test_calls_refuse_tensors_of_another_device():
    """_lib._on makes the tensors' device current for a call and refuses structs / tensors that
    live elsewhere (a launch on device 0 with device-1 pointers is a GPU fault, not an exception)."""
    import torch
    from gnn_fpga_amd import _lib
    with pytest.raises(_lib.GnnHipError):
        _lib._on(torch.zeros(3))                                   # CPU tensor: no CPU path
    g = _lib.GnnGraph()
    g._device = torch.device("cuda", 1)
    with pytest.raises(_lib.GnnHipError):
        _lib._on(torch.device("cuda", 0), g)                       # struct built for another device
    _lib._on(torch.device("cuda", 1), g)                           # same device: accepted (not entered)
    # while a call on cuda:1 is in progress, a cuda:0 / CPU tensor is refused by _dev()
    _lib._cur_dev = torch.device("cuda", 1)
    try:
        with pytest.raises(_lib.GnnHipError):
            _lib._dev(torch.zeros(3), torch.float32, "x")
    finally:
        _lib._cur_dev = None


def test_event_route_decision_is_pinned():
    """`_lib.events_preferred` (which batches take the one-workgroup-per-graph kernels) on both sides of
    each threshold: <= 1200 segments per graph (tools/cliff_probe.py: 256 x (150, 1000) one-launch 0.050
    ms vs tiled 0.066; 256 x (300, 2000) 0.119 vs 0.069), hidden_dim <= 16 (one D = 32 toy graph 0.123 vs
    0.089), the graph must fit the kernel's LDS.  The GPU twin of this test
    (test_gpu_formats.py::test_event_route_crossover) checks the kernels that ran and their times."""
    from gnn_fpga_amd import _lib
    from gnn_fpga_amd.hitgraph import _EventLayout

    def lay(h, s):
        return _EventLayout([0, h], [0, s])

    assert _lib.EVENTS_MAX_SEGMENTS == 1200
    assert _lib.events_preferred(3, 8, lay(150, 1000))
    assert _lib.events_preferred(3, 8, lay(150, 1200))
    assert not _lib.events_preferred(3, 8, lay(150, 1201))
    assert not _lib.events_preferred(3, 8, lay(300, 2000))
    assert _lib.events_preferred(11, 8, lay(40, 150))                 # the reference's muon graphs
    assert _lib.events_preferred(3, 16, lay(100, 250))
    assert not _lib.events_preferred(2, 32, lay(40, 144))             # wide hidden layers: tiled
    assert not _lib.events_preferred(3, 8, None)                      # not block-diagonal
    assert not _lib.events_preferred(3, 8, lay(40000, 1000))          # does not fit the LDS of one workgroup


_ROUTE_SWITCHES = ("GNN_NO_ITER2", "GNN_NO_FUSE_FIRST", "GNN_NO_WIDE_EXACT", "GNN_WIDE_LOCKSTEP", "GNN_WIDE_ROLES")
_LISTS16 = ("in_off16", "in_nbr16", "out_off16", "out_nbr16", "sched_a", "sched_b")
XP, BF = 1, 2          # GNN_FLAG_EXP_PRODUCT, GNN_FLAG_BF16_MLP


def _route_plan(n_pad=1024, n_tiles=4, n_lds_tiles=None, lds_in=100, lds_out=100, missing=()):
    """A gnn_plan_t as gnn_plan_route reads it: scalars, and pointers that are only NULL or not."""
    from gnn_fpga_amd import _lib
    g = _lib.GnnPlan()
    for name, kind in _lib.GnnPlan._fields_:
        if kind is ctypes.c_void_p and name not in missing:
            setattr(g, name, 0x1000)
    g.n_pad, g.n_segments, g.n_tiles, g.n_chunks = n_pad, 5000, n_tiles, 1
    g.n_lds_tiles = n_tiles if n_lds_tiles is None else n_lds_tiles
    g.iter_lds_in, g.iter_lds_out, g.iter_lds_records, g.edge_lds_rows = lds_in, lds_out, 204, 300
    return g


def test_plan_route_is_pinned(monkeypatch):
    """gnn_plan_route: which kernels the fused forward takes, on both sides of every condition.  The expected routes
    were written down from forward_t / forward_train_t as they stood BEFORE the route decision was gathered into
    choose_route (csrc/sell_pipeline.hip): (records, input stage, iteration kernel, fused first launch, edge kernel,
    k_pack).  The GPU twin (test_gpu_plan_route.py) checks the kernels that ran."""
    from gnn_fpga_amd import _lib
    for k in _ROUTE_SWITCHES:
        monkeypatch.delenv(k, raising=False)

    def route(F, D, T=3, flags=XP, training=False, **plan):
        r = _lib.plan_route(_route_plan(**plan), F, D, T, flags=flags, training=training)
        return r and (r["records"], r["input"], r["family"], r["fuse_first"], r["edge"], r["pack"])

    fused = ("fp32", None, "k_iter2", True, "k_edge", False)            # T x k_iter2, the first with the input network
    iter2 = ("fp32", "k_input4", "k_iter2", False, "k_edge", False)
    general = ("fp32", "k_input4", "k_iter", False, "k_edge", False)
    exact16 = ("exact", "k_input4_x", "k_iter_w", False, "k_edge", True)
    exact = ("exact", "k_input4_x", "k_iter_w", False, "k_edge_w", True)
    exact_wx = ("exact", "k_input4_x", "k_iter_wx", False, "k_edge_w", True)
    bf16 = ("bf16", "k_input4_bf", "k_iter_w", False, "k_edge_w", True)
    bf16_wx = ("bf16", "k_input4_bf", "k_iter_wx", False, "k_edge_w", True)
    general_wide = ("fp32", "k_input4", "k_iter", False, "k_edge_w", True)     # big table: k_pack; wide rows: k_edge_w
    # every shape of PlanShapes: 3 iterations, exp-product on, every tile in LDS mode, 1024 padded hits
    default = {(2, 4): fused, (2, 8): iter2, (2, 16): exact16, (2, 32): exact, (3, 4): fused, (3, 8): fused,
               (3, 16): exact16, (3, 32): exact, (3, 64): exact, (11, 4): iter2, (11, 8): iter2, (11, 16): general}
    trains = {(2, 4), (2, 8), (3, 4), (3, 8), (11, 4), (11, 8), (11, 16)}     # D <= 16 without the wide route
    for (F, D), want in default.items():
        assert _lib.plan_shape_supported(F, D)
        assert route(F, D) == want, (F, D)
        # n_pad = 0: k_pack and nothing else before the edge pass
        assert route(F, D, n_pad=0) == ("fp32", None, "k_iter", False, want[4], True), (F, D)
        # the fused training forward: the general route where it exists (whatever the flags say), refused elsewhere
        for flags in (0, XP | BF):
            assert route(F, D, flags=flags, training=True) == (general if (F, D) in trains else None), (F, D)
    assert len(default) == 12 and not _lib.plan_shape_supported(5, 7)
    with pytest.raises(_lib.GnnHipError, match="input_dim=5"):
        route(5, 7)
    # exp-product off: no fused first launch
    assert route(3, 8, flags=0) == iter2 and route(2, 4, flags=0) == iter2 and route(3, 64, flags=0) == exact
    # n_iters 2 / 1 / 0: the fused first launch needs two iterations, the wide record forms one
    assert route(3, 8, T=2) == fused and route(3, 8, T=1) == iter2 and route(3, 8, T=0) == iter2
    assert route(3, 64, T=1) == exact and route(3, 64, T=0) == general_wide
    assert route(3, 64, T=1, flags=XP | BF) == bf16 and route(3, 64, T=0, flags=XP | BF) == general_wide
    assert route(3, 16, T=0) == general
    # k_iter2 needs every tile in LDS mode, tiles at all, and all six 16-bit lists / schedules
    assert route(3, 8, n_lds_tiles=3) == general and route(3, 8, n_tiles=0) == general
    for name in _LISTS16:
        assert route(3, 8, missing=(name,)) == general, name
    assert route(3, 8, missing=("in_nbr", "out_nbr")) == fused            # (k_iter2 reads the 16-bit lists only)
    # ... and both windows inside the 160 KB of LDS: (652 table + 848 matrix-core + 4 + 16 (cap_a + cap_b)) floats
    r = _lib.plan_route(_route_plan(lds_in=1216, lds_out=1216), 3, 8, 3, flags=XP)
    assert (r["family"], r["fuse_first"], r["cap_a"], r["cap_b"], r["iter2_lds"]) == ("k_iter2", True, 1232, 1232, 163712)
    r = _lib.plan_route(_route_plan(lds_in=1217, lds_out=1216), 3, 8, 3, flags=XP)
    assert (r["family"], r["input"], r["cap_a"], r["cap_b"], r["iter2_lds"]) == ("k_iter", "k_input4", 1248, 1232, 164736)
    assert route(3, 8, lds_in=1216, lds_out=1217) == general
    # the sizes of a small plan: k_iter (652 + 16 x 204 records + 4) floats, k_iter2 (1504 + 16 x 256), k_edge (8 x 300 + 4)
    r = _lib.plan_route(_route_plan(), 3, 8, 3, flags=XP)
    assert (r["iter_lds"], r["iter2_lds"], r["cap_a"], r["cap_b"], r["edge_lds"], r["wide_window"]) == \
        (15680, 22400, 128, 128, 9616, 0)
    # bf16 flag: hidden_dim 32 / 64 up to input_dim 8 only
    assert route(3, 32, flags=XP | BF) == bf16 and route(2, 32, flags=BF) == bf16 and route(3, 64, flags=XP | BF) == bf16
    assert route(3, 16, flags=XP | BF) == exact16 and route(11, 16, flags=XP | BF) == general
    assert route(3, 8, flags=XP | BF) == fused
    # groups of k_iter_w / k_iter_wx: 3 MB of record rows (8 D bytes exact, 4 D bytes bf16); no LDS windows
    for F, D, flags, window in ((3, 64, XP, 6144), (3, 64, XP | BF, 12288), (3, 32, XP, 12288), (3, 32, XP | BF, 24576),
                                (3, 16, XP, 24576)):
        r = _lib.plan_route(_route_plan(), F, D, 3, flags=flags)
        assert (r["wide_window"], r["iter2_lds"], r["cap_a"]) == (window, 0, 0), (F, D, flags)
    assert _lib.plan_route(_route_plan(), 3, 64, 3)["edge_lds"] == 16
    assert _lib.plan_route(_route_plan(), 3, 16, 3)["iter_lds"] == (2004 + 4) * 4        # wide16: no record windows
    # the role-split kernel from 32768 padded hits on
    for F, D, flags, small, large in ((3, 64, XP, exact, exact_wx), (3, 64, XP | BF, bf16, bf16_wx),
                                      (2, 32, 0, exact, exact_wx)):
        assert route(F, D, flags=flags, n_pad=32767) == small and route(F, D, flags=flags, n_pad=32768) == large
    assert route(3, 16, n_pad=32767) == exact16 and route(3, 16, n_pad=32768) == exact16[:2] + ("k_iter_wx",) + exact16[3:]
    # 32-bit record offsets, D = 64: (n_pad + 2) rows of 512 bytes (exact) / 256 bytes (bf16) below 4 GiB
    assert route(3, 64, n_pad=8388605) == exact_wx and route(3, 64, n_pad=8388606) == general_wide
    assert route(3, 64, flags=XP | BF, n_pad=16777213) == bf16_wx
    assert route(3, 64, flags=XP | BF, n_pad=16777214) == general_wide
    assert route(3, 64, flags=XP | BF, n_pad=8388606) == bf16_wx
    # the switches, one at a time
    monkeypatch.setenv("GNN_NO_ITER2", "1")
    assert route(3, 8) == general and route(2, 8) == general and route(3, 64) == exact
    monkeypatch.delenv("GNN_NO_ITER2")
    monkeypatch.setenv("GNN_NO_FUSE_FIRST", "1")
    assert route(3, 8) == iter2 and route(2, 4) == iter2 and route(3, 64) == exact
    monkeypatch.delenv("GNN_NO_FUSE_FIRST")
    monkeypatch.setenv("GNN_NO_WIDE_EXACT", "1")
    assert route(3, 64) == general_wide and route(3, 32) == general_wide and route(3, 16) == general
    assert route(3, 64, flags=XP | BF) == bf16 and route(3, 8) == fused
    monkeypatch.delenv("GNN_NO_WIDE_EXACT")
    monkeypatch.setenv("GNN_WIDE_ROLES", "1")
    assert route(3, 64) == exact_wx and route(3, 32, flags=XP | BF) == bf16_wx and route(3, 8) == fused
    monkeypatch.setenv("GNN_WIDE_LOCKSTEP", "1")                        # both: the barrier kernel
    assert route(3, 64) == exact and route(3, 64, n_pad=40000) == exact
    monkeypatch.delenv("GNN_WIDE_ROLES")
    assert route(3, 64, n_pad=40000) == exact and route(3, 64, flags=XP | BF, n_pad=40000) == bf16
    monkeypatch.delenv("GNN_WIDE_LOCKSTEP")
    assert route(3, 64, n_pad=40000) == exact_wx
    # bad arguments are refused before anything is read
    lib, out = _lib.load(), (ctypes.c_int32 * len(_lib.ROUTE_FIELDS))()
    assert lib.gnn_plan_route(None, None, 1, 0, out) == _lib.GNN_ERR_BADARG
    P = _lib.GnnParams()
    P.F, P.D = 3, 8
    assert lib.gnn_plan_route(ctypes.byref(_route_plan()), ctypes.byref(P), -1, 0, out) == _lib.GNN_ERR_BADARG
    assert lib.gnn_plan_route(ctypes.byref(_route_plan()), ctypes.byref(P), 1, 0, None) == _lib.GNN_ERR_BADARG


def test_plan_workspace_bytes_are_pinned():
    """gnn_plan_workspace_bytes per shape at n_pad 0, 1, 255, 256 and 100000, as recorded from the build before the
    workspace was carved with common.h's Carver."""
    from gnn_fpga_amd import _lib
    recorded = {
        (2, 4): [11520, 11520, 54784, 56576, 17611520],
        (2, 8): [21248, 21248, 109568, 111360, 35221248],
        (2, 16): [52992, 52992, 231424, 233216, 70452992],
        (2, 32): [132608, 133632, 491264, 493056, 140932608],
        (3, 4): [11520, 11520, 54784, 56576, 17611520],
        (3, 8): [21248, 21248, 109568, 111360, 35221248],
        (3, 16): [53504, 53504, 231936, 233728, 70453504],
        (3, 32): [133376, 134400, 492032, 493824, 140933376],
        (3, 64): [379904, 382720, 1097984, 1100800, 281979904],
        (11, 4): [12288, 12288, 55552, 57344, 17612288],
        (11, 8): [22784, 22784, 111104, 112896, 35222784],
        (11, 16): [46080, 46080, 224512, 226304, 70446080],
    }
    for (F, D), want in recorded.items():
        assert [_lib.plan_workspace_bytes(n, 0, F, D) for n in (0, 1, 255, 256, 100000)] == want, (F, D)


def test_backward_workspace_bytes_are_pinned():
    """gnn_backward_workspace_bytes per backward shape at (hits, segments) = (0, 0), (1, 0), (909, 6011) and
    (40000, 300000), and gnn_backward_events_workspace_bytes at 0, 1 and 1024 graphs, as recorded from the build before
    the gradient replica's size came from one function and the workspace was carved with common.h's Carver."""
    from gnn_fpga_amd import _lib
    recorded = {
        (2, 4): ([7168, 8960, 335360, 14811392], [1792, 1792, 811264]),
        (2, 8): ([20992, 22784, 606208, 26673408], [4864, 4864, 2433280]),
        (2, 16): ([67072, 68864, 1199872, 52560128], [15104, 15104, 7840000]),
        (2, 32): ([242176, 245248, 2747904, 119825664], [54016, 54016, 28385536]),
        (3, 4): ([7168, 8960, 335360, 14811392], [1792, 1792, 811264]),
        (3, 8): ([20992, 22784, 606208, 26673408], [4864, 4864, 2433280]),
        (3, 16): ([69376, 71168, 1206272, 52830464], [15616, 15616, 8110336]),
        (3, 32): ([249088, 252160, 2767104, 120636672], [55552, 55552, 29196544]),
        (3, 64): ([940288, 945664, 6664448, 288777472], [209152, 209152, 110297344]),
        (4, 8): ([23296, 25088, 612608, 26943744], [5376, 5376, 2703616]),
        (4, 16): ([73984, 75776, 1219072, 53371136], [16640, 16640, 8651008]),
        (4, 32): ([256000, 259072, 2786304, 121447680], [57088, 57088, 30007552]),
        (4, 64): ([954112, 959488, 6702848, 290399488], [212224, 212224, 111919360]),
        (11, 4): ([14080, 15872, 471040, 20742400], [3328, 3328, 1622272]),
        (11, 8): ([34816, 36608, 761344, 33415424], [7936, 7936, 4055296]),
        (11, 16): ([97024, 98816, 1399040, 61194496], [21760, 21760, 11354368]),
    }
    with open(os.path.join(REPO, "gnn-fpga_amd", "csrc", "common.h")) as f:         # the list the backward dispatches over
        listed = re.search(r"using ModelShapes = ShapeList<(.*?)>;", f.read(), flags=re.S).group(1)
    assert sorted(recorded) == sorted((int(a), int(b)) for a, b in re.findall(r"Shape<(\d+), (\d+)>", listed))
    lib = _lib.load()
    for (F, D), (want, want_events) in recorded.items():
        got = [lib.gnn_backward_workspace_bytes(n, e, F, D) for n, e in ((0, 0), (1, 0), (909, 6011), (40000, 300000))]
        assert got == want, (F, D)
        assert [lib.gnn_backward_events_workspace_bytes(g, F, D) for g in (0, 1, 1024)] == want_events, (F, D)
