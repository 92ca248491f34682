"""The per-iteration entry points (include/gnn_hip_iter.h) on poisoned workspaces and guarded outputs, and on arrays that
start off the 16-byte grid: the checks every entry point of gnn_hip.h has (test_gpu_uninitialised.py `check`,
test_gpu_offset_arrays.py `sweep`), through the binding's wrappers.  COVERS maps every function of
_lib.ITER_SIGNATURES that takes a device pointer to the test here that runs it."""
import ctypes

import numpy as np
import pytest
import torch

from gnn_fpga_amd import HitGraphBatch, synth
from offset_arrays import shift_batch
from test_gpu_offset_arrays import sweep
from test_gpu_uninitialised import check

pytestmark = pytest.mark.gpu

COVERS = {
    "gnn_iter_forward_events": "test_forward_and_backward",
    "gnn_iter_backward_events": "test_forward_and_backward",
    "gnn_iter_input_bwd": "test_input_backward",
}
NO_ARRAYS = {"gnn_iter_events_supported", "gnn_iter_grad_floats", "gnn_iter_backward_workspace_bytes",
             "gnn_iter_input_bwd_workspace_bytes"}

# (F, D, T, shared, graphs): the notebook's event shape at its width; ragged muon-schema graphs, one without segments
CASES = {
    "toy_d32": (2, 32, 3, False, lambda: [synth.toy2d_graph(s) for s in range(3)]),
    "toy_d32_shared": (2, 32, 3, True, lambda: [synth.toy2d_graph(s) for s in range(2)]),
    "muon_d8": (11, 8, 2, False, lambda: [synth.muon_graph(s) for s in range(4)] +
                [synth.HitGraph(synth.muon_graph(9).X, *(a[:0] for a in synth.muon_graph(9)[1:]))]),
}


def test_covers_every_entry_point(hip):
    takes_pointer = {n for n, (_, args) in hip.ITER_SIGNATURES.items()
                     if any(a is ctypes.c_void_p or isinstance(a, type(ctypes.POINTER(ctypes.c_int))) for a in args)}
    assert takes_pointer == set(COVERS) and takes_pointer | NO_ARRAYS == set(hip.ITER_SIGNATURES)
    assert all(v in globals() for v in COVERS.values())


def _weights(F, D, T, shared, seed=0):
    """(Win, bin, edge sets, node sets, out set) as host tensors; shared: one edge and one node set."""
    g = torch.Generator().manual_seed(seed)
    C = F + D
    r = lambda *s: (torch.rand(*s, generator=g) - 0.5) * 0.6      # noqa: E731
    edge = lambda: [r(D, 2 * C), r(D), r(1, D), r(1)]             # noqa: E731
    node = lambda: [r(D, 3 * C), r(D), r(D, D), r(D)]             # noqa: E731
    if shared:
        e, n = edge(), node()
        return r(D, F), r(D), [e] * T, [n] * T, e
    return r(D, F), r(D), [edge() for _ in range(T)], [node() for _ in range(T)], edge()


def _call(case):
    from gnn_fpga_amd import _lib
    F, D, T, shared, graphs = CASES[case]
    hb = HitGraphBatch.from_graphs(graphs())
    win, bin_, edge, node, out = _weights(F, D, T, shared)
    go = torch.rand(hb.n_segments, generator=torch.Generator().manual_seed(5)) - 0.5

    def call(S=None):
        s = S if S is not None else (lambda t: t)
        b = shift_batch(hb, S if S is not None else 0)
        seen = {}

        def dev(t):                  # (a shared set is ONE set of tensors, wherever it is pointed at)
            if id(t) not in seen:
                seen[id(t)] = s(t.cuda())
            return seen[id(t)]
        ip = _lib.iter_params_struct(dev(win), dev(bin_), [[dev(t) for t in e] for e in edge],
                                     [[dev(t) for t in n] for n in node], [dev(t) for t in out], F, D, shared)
        lay = b.event_layout()
        assert lay is not None and _lib.iter_events_supported(F, D, lay.max_hits, lay.max_segments, True)
        scores = _lib.iter_forward_events(b, lay, ip)
        kept = _lib.iter_forward_events(b, lay, ip, train=True)
        e_all, H_all = (s(t) for t in kept)
        flat = _lib.iter_backward_events(b, lay, ip, e_all, H_all, s(go.cuda()))
        assert torch.equal(scores, kept[0][T])
        return [scores, kept, flat]
    return call


@pytest.mark.parametrize("case", sorted(CASES))
def test_forward_and_backward(hip, case):
    call = _call(case)
    check(call)
    sweep(call)


@pytest.mark.parametrize("n,F,D", [(37, 2, 32), (2500, 11, 8), (0, 2, 8)])
def test_input_backward(hip, n, F, D):
    from gnn_fpga_amd import _lib
    g = torch.Generator().manual_seed(n)
    X, Win, bin_ = torch.rand(n, F, generator=g) - 0.5, torch.rand(D, F, generator=g) - 0.5, torch.rand(D, generator=g)
    gH = torch.rand(n, F + D, generator=g) - 0.5

    def call(S=None):
        s = S if S is not None else (lambda t: t)
        Xd = s(X.cuda())
        # (gnn_input_fwd takes no empty batch; the backward does: every gradient is zero)
        H0 = _lib.input_fwd(Xd, s(Win.cuda()), s(bin_.cuda())) if n else torch.zeros(0, _lib.h_stride(F, D)).cuda()
        return [_lib.iter_input_bwd(Xd, s(H0), s(gH.cuda()), F, D)]
    flat = check(call)[0].cpu().double()
    sweep(call)
    Xd, h = X.double(), torch.tanh(X.double() @ Win.double().T + bin_.double())
    gz = gH[:, :D].double() * (1 - h * h)
    want = torch.cat([(gz.T @ Xd).reshape(-1), gz.sum(0)])
    assert float((flat - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))
