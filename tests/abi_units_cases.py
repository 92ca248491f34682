"""What tests/test_abi_units_host.py asks of the library and tools/gen_abi_units_golden.py records: the answers of every
entry point that says whether a shape has kernels or how much memory it needs, over a grid of shapes and sizes, and the
(return code, gnn_last_error()) of calls that every entry point refuses before it launches anything.  None of these
calls reaches the GPU: they need the built library only.

The recorded files (tests/golden/abi_units/*.json) come from the library as it was before the entry points moved next to
their kernels and the shape lists became types (csrc/common.h ShapeList): they pin every list at every shape, listed or
not, and every message.
"""
import ctypes
import itertools

from gnn_fpga_amd import _lib

FS = list(range(1, 13))
DS = [1, 4, 8, 12, 16, 32, 64, 128]
SIZES = [0, 1, 300, 5000]
PAIRS = list(itertools.product(SIZES, SIZES))
FX_FORMATS = [(16, 6, 10), (24, 8, 12), (3, 2, 4), (16, 6, 13)]          # (total_bits, int_bits, table_bits); two are refused
ITER_COUNTS = [0, 1, 16, 17]                                             # GNN_ITER_MAX = 16


def bind(path):
    """The library at `path` with _lib's signatures (the in-tree one: _lib.load())."""
    lib = ctypes.CDLL(path)
    for table in (_lib.SIGNATURES, _lib.ITER_SIGNATURES, _lib.FX_SIGNATURES, _lib.FXEV_SIGNATURES):
        for name, (res, args) in table.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


def shape_answers(lib):
    """name -> the answers in the order of (F in FS, D in DS, the function's further arguments)."""
    def limits(F, D):
        out = (ctypes.c_int32 * 4)(-7, -7, -7, -7)
        return [lib.gnn_plan_limits(F, D, out)] + list(out)

    per_shape = {
        "gnn_shape_supported": lambda F, D: [lib.gnn_shape_supported(F, D)],
        "gnn_h_stride": lambda F, D: [lib.gnn_h_stride(F, D)],
        "gnn_plan_shape_supported": lambda F, D: [lib.gnn_plan_shape_supported(F, D)],
        "gnn_plan_limits": limits,
        "gnn_forward_workspace_bytes": lambda F, D: [lib.gnn_forward_workspace_bytes(n, e, F, D) for n, e in PAIRS],
        "gnn_backward_workspace_bytes": lambda F, D: [lib.gnn_backward_workspace_bytes(n, e, F, D) for n, e in PAIRS],
        "gnn_plan_workspace_bytes": lambda F, D: [lib.gnn_plan_workspace_bytes(n, e, F, D) for n, e in PAIRS],
        "gnn_events_supported": lambda F, D: [lib.gnn_events_supported(F, D, n, e) for n, e in PAIRS],
        "gnn_events_backward_supported": lambda F, D: [lib.gnn_events_backward_supported(F, D, n, e) for n, e in PAIRS],
        "gnn_backward_events_workspace_bytes": lambda F, D: [lib.gnn_backward_events_workspace_bytes(n, F, D) for n in SIZES],
        "gnn_iter_events_supported": lambda F, D: [lib.gnn_iter_events_supported(F, D, n, e, b)
                                                   for n, e in PAIRS for b in (0, 1)],
        "gnn_iter_grad_floats": lambda F, D: [lib.gnn_iter_grad_floats(F, D, t, s) for t in ITER_COUNTS for s in (0, 1)],
        "gnn_fx_supported": lambda F, D: [lib.gnn_fx_supported(F, D, *fmt) for fmt in FX_FORMATS],
        "gnn_fxev_supported": lambda F, D: [lib.gnn_fxev_supported(F, D, fmt[2], n, e) for fmt in FX_FORMATS for n, e in PAIRS],
        "gnn_fxev_lds_bytes": lambda F, D: [lib.gnn_fxev_lds_bytes(F, D, fmt[2], n, e) for fmt in FX_FORMATS for n, e in PAIRS],
    }
    return {name: [v for F in FS for D in DS for v in fn(F, D)] for name, fn in per_shape.items()}


PTR = 0x7000          # stands for a device array: refused calls never read through it
BIG = 1 << 40         # a workspace size no shape exceeds here
N, E, G = 16, 32, 2   # hits, segments, graphs of the calls with a shape


def _graph():
    g = _lib.GnnGraph()
    for name in ("X", "src", "dst", "in_ptr", "in_eid", "in_nbr", "out_ptr", "out_eid", "out_nbr"):
        setattr(g, name, PTR)
    g.n_hits, g.n_segments = N, E
    return g


def _weights(cls, F, D):
    p = cls()
    for name in ("Win", "bin", "W1", "b1", "W2", "b2", "W3", "b3", "W4", "b4"):
        setattr(p, name, PTR)
    if cls is not _lib.GnnGrads:
        p.F, p.D = F, D
    return p


def _plan():
    pl = _lib.GnnPlan()
    for name, ctype in _lib.GnnPlan._fields_:
        setattr(pl, name, PTR if ctype is _lib._f else 0)
    pl.n_pad, pl.n_segments, pl.n_tiles, pl.n_chunks = 1024, 4096, 8, 8
    return pl


def _iter_params(F, D):
    p = _lib.GnnIterParams()
    p.Win = p.bin = PTR
    for s in [p.out] + [p.edge[t] for t in range(2)] + [p.node[t] for t in range(2)]:
        s.Wa = s.ba = s.Wb = s.bb = PTR
    p.F, p.D, p.n_iters, p.shared = F, D, 2, 0
    return p


def _fx(F, D):
    p = _weights(_lib.GnnFxParams, F, D)
    fmt = _lib.GnnFxFormat(16, 6, 0, 1, 10)
    tb = _lib.GnnFxTables(PTR, PTR)
    return p, fmt, tb


def refusal_calls(lib):
    """([(label, function, arguments)], the structs the arguments point at): calls that are refused before any launch."""
    ref, P = ctypes.byref, PTR
    calls = []

    def add(label, fn, *args):
        calls.append((label, fn, args))

    # ---- every pointer null, every count -1
    add("gnn_profile_begin(-1)", lib.gnn_profile_begin, -1)
    add("gnn_input_fwd null", lib.gnn_input_fwd, None, None, None, None, -1, -1, -1, -1, None)
    add("gnn_edge_fwd null", lib.gnn_edge_fwd, None, -1, None, None, None, None, None, None, None, None, -1, -1, -1, -1, None)
    add("gnn_node_fwd null", lib.gnn_node_fwd, None, -1, None, None, None, None, None, None, None, -1, -1, None)
    add("gnn_segclf_forward null", lib.gnn_segclf_forward, None, None, -1, None, None, None, None, 0, None)
    add("gnn_segclf_forward_train null", lib.gnn_segclf_forward_train, None, None, -1, None, None, None, None, 0, None)
    add("gnn_nodeclf_forward null", lib.gnn_nodeclf_forward, None, None, None, None, -1, None, None, None, 0, None)
    add("gnn_nodeclf_forward_train null", lib.gnn_nodeclf_forward_train, None, None, None, None, -1, None, None, None, None,
        None, 0, None)
    add("gnn_segclf_forward_events null", lib.gnn_segclf_forward_events, None, None, None, None, -1, -1, -1, -1, None, None)
    add("gnn_segclf_forward_train_events null", lib.gnn_segclf_forward_train_events, None, None, None, None, -1, -1, -1, -1,
        None, None, None)
    add("gnn_segclf_backward null", lib.gnn_segclf_backward, None, None, -1, None, None, None, None, None, None, 0, None)
    add("gnn_nodeclf_backward null", lib.gnn_nodeclf_backward, None, None, None, None, -1, None, None, None, None, None, None,
        None, None, None, 0, None)
    add("gnn_edge_bwd null", lib.gnn_edge_bwd, None, -1, None, None, None, None, None, None, None, 0, None)
    add("gnn_node_bwd null", lib.gnn_node_bwd, None, -1, None, None, None, None, None, None, None, None, None, 0, None)
    add("gnn_segclf_backward_events null", lib.gnn_segclf_backward_events, None, None, None, None, -1, -1, -1, -1, None, None,
        None, None, None, 0, None)
    add("gnn_bce_loss null", lib.gnn_bce_loss, None, None, -1, 0.0, None, None, None, None)
    add("gnn_dense_to_index null", lib.gnn_dense_to_index, None, None, -1, -1, -1, None, None, None, None)
    add("gnn_plan_limits null", lib.gnn_plan_limits, -1, -1, None)
    add("gnn_plan_route null", lib.gnn_plan_route, None, None, -1, -1, None)
    add("gnn_segclf_forward_plan null", lib.gnn_segclf_forward_plan, None, None, -1, None, None, 0, None)
    add("gnn_segclf_forward_train_plan null", lib.gnn_segclf_forward_train_plan, None, None, -1, None, None, None, None, None,
        None, None, None, 0, None)
    add("gnn_exp_product_bound null", lib.gnn_exp_product_bound, None, None, None, None)
    add("gnn_iter_forward_events null", lib.gnn_iter_forward_events, None, None, None, None, -1, -1, -1, None, None, None, None)
    add("gnn_iter_backward_events null", lib.gnn_iter_backward_events, None, None, None, None, -1, -1, -1, None, None, None,
        None, None, 0, None)
    add("gnn_iter_backward_workspace_bytes(-1)", lib.gnn_iter_backward_workspace_bytes, -1, -1, -1, -1)
    add("gnn_fx_forward null", lib.gnn_fx_forward, None, None, None, None, -1, None, None, None, None, None, None, 0, None)
    add("gnn_fx_workspace_bytes(-1)", lib.gnn_fx_workspace_bytes, -1, -1, -1, -1)
    add("gnn_fxev_forward null", lib.gnn_fxev_forward, None, None, None, None, None, None, -1, -1, -1, -1, None, None, None,
        None, None, None, None)

    # ---- a shape without kernels, everything else in order.  (5, 7) is in no list; (4, 8) has no fused pipeline,
    # (3, 32) no fused training forward and no one-launch backward, (3, 64) no per-iteration kernel
    def shaped(F, D):
        tag = " (%d, %d)" % (F, D)
        ldh = (F + D + 3) & ~3
        g, p, gr = _graph(), _weights(_lib.GnnParams, F, D), _weights(_lib.GnnGrads, F, D)
        keep = (g, p, gr)
        add("gnn_input_fwd" + tag, lib.gnn_input_fwd, P, P, P, P, N, F, D, ldh, None)
        add("gnn_edge_fwd" + tag, lib.gnn_edge_fwd, P, ldh, P, P, P, P, P, P, P, P, N, E, F, D, None)
        add("gnn_node_fwd" + tag, lib.gnn_node_fwd, P, ldh, P, ref(g), P, P, P, P, P + 64, F, D, None)
        add("gnn_segclf_forward" + tag, lib.gnn_segclf_forward, ref(g), ref(p), 2, P, None, None, P, BIG, None)
        add("gnn_segclf_forward_train" + tag, lib.gnn_segclf_forward_train, ref(g), ref(p), 2, P, P, P, P, BIG, None)
        add("gnn_nodeclf_forward" + tag, lib.gnn_nodeclf_forward, ref(g), ref(p), P, P, 2, P, None, P, BIG, None)
        add("gnn_nodeclf_forward_train" + tag, lib.gnn_nodeclf_forward_train, ref(g), ref(p), P, P, 2, P, P, P, P, P, BIG, None)
        add("gnn_segclf_forward_events" + tag, lib.gnn_segclf_forward_events, ref(g), ref(p), P, P, G, N, E, 2, P, None)
        add("gnn_segclf_forward_train_events" + tag, lib.gnn_segclf_forward_train_events, ref(g), ref(p), P, P, G, N, E, 2, P,
            P, None)
        add("gnn_segclf_backward" + tag, lib.gnn_segclf_backward, ref(g), ref(p), 2, P, P, P, P, ref(gr), P, BIG, None)
        add("gnn_nodeclf_backward" + tag, lib.gnn_nodeclf_backward, ref(g), ref(p), P, P, 2, P, P, P, P, P, ref(gr), P, P, P,
            BIG, None)
        for stride in (ldh, 0):       # gnn_h_stride of a shape without kernels is 0: only that stride gets to the dispatch
            add("gnn_edge_bwd ldh %d" % stride + tag, lib.gnn_edge_bwd, P, stride, ref(g), ref(p), P, P, P, ref(gr), P, BIG, None)
            add("gnn_node_bwd ldh %d" % stride + tag, lib.gnn_node_bwd, P, stride, P, P, ref(g), ref(p), P, P, P, ref(gr), P,
                BIG, None)
        add("gnn_segclf_backward_events" + tag, lib.gnn_segclf_backward_events, ref(g), ref(p), P, P, G, N, E, 2, P, P, P,
            ref(gr), P, BIG, None)
        return keep

    def planned(F, D):
        tag = " (%d, %d)" % (F, D)
        pl, p = _plan(), _weights(_lib.GnnParams, F, D)
        out4, route = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * len(_lib.ROUTE_FIELDS))()
        add("gnn_plan_limits" + tag, lib.gnn_plan_limits, F, D, out4)
        add("gnn_plan_route" + tag, lib.gnn_plan_route, ref(pl), ref(p), 2, 0, route)
        add("gnn_segclf_forward_plan" + tag, lib.gnn_segclf_forward_plan, ref(pl), ref(p), 2, P, P, BIG, None)
        return (pl, p, out4, route) + planned_train(F, D)

    def planned_train(F, D):
        tag = " (%d, %d)" % (F, D)
        pl, p = _plan(), _weights(_lib.GnnParams, F, D)
        route = (ctypes.c_int32 * len(_lib.ROUTE_FIELDS))()
        add("gnn_plan_route training" + tag, lib.gnn_plan_route, ref(pl), ref(p), 2, 1, route)
        add("gnn_segclf_forward_train_plan" + tag, lib.gnn_segclf_forward_train_plan, ref(pl), ref(p), 2, P, P, P, P, P, P, P,
            P, BIG, None)
        return (pl, p, route)

    def iterated(F, D):
        tag = " (%d, %d)" % (F, D)
        g, p = _graph(), _iter_params(F, D)
        add("gnn_iter_forward_events" + tag, lib.gnn_iter_forward_events, ref(g), ref(p), P, P, G, N, E, P, None, None, None)
        add("gnn_iter_backward_events" + tag, lib.gnn_iter_backward_events, ref(g), ref(p), P, P, G, N, E, P, P, P, P, P, BIG,
            None)
        add("gnn_iter_backward_workspace_bytes" + tag, lib.gnn_iter_backward_workspace_bytes, G, F, D, 2)
        return (g, p)

    def fixed(F, D):
        tag = " (%d, %d)" % (F, D)
        g = _graph()
        p, fmt, tb = _fx(F, D)
        add("gnn_fx_workspace_bytes" + tag, lib.gnn_fx_workspace_bytes, N, E, F, D)
        add("gnn_fx_forward" + tag, lib.gnn_fx_forward, ref(g), ref(p), ref(fmt), ref(tb), 2, P, P, P, None, None, P, BIG, None)
        add("gnn_fxev_forward" + tag, lib.gnn_fxev_forward, ref(g), ref(p), ref(fmt), ref(tb), P, P, G, N, E, 2, P, P, P, None,
            None, None, None)
        return (g, p, fmt, tb)

    alive = [shaped(5, 7), planned(5, 7), iterated(5, 7), fixed(5, 7), planned(4, 8), planned_train(3, 32), iterated(3, 64)]
    g, p, gr = _graph(), _weights(_lib.GnnParams, 3, 32), _weights(_lib.GnnGrads, 3, 32)
    add("gnn_segclf_backward_events (3, 32)", lib.gnn_segclf_backward_events, ref(g), ref(p), P, P, G, N, E, 2, P, P, P, ref(gr),
        P, BIG, None)
    alive.append((g, p, gr))
    return calls, alive


def refusals(lib):
    """label -> [return value, gnn_last_error()] of every refused call."""
    out = {}
    calls, alive = refusal_calls(lib)          # (`alive` keeps the structs until the last call has returned)
    for label, fn, args in calls:
        assert label not in out, label
        rc = fn(*args)
        out[label] = [rc, lib.gnn_last_error().decode()]
    del alive
    return out
