"""gnn_fx_forward (include/gnn_hip_fixed.h) on poisoned workspaces and guarded outputs, and on arrays that start off the
16-byte grid: the checks every entry point of gnn_hip.h has (test_gpu_uninitialised.py `check`,
test_gpu_offset_arrays.py `sweep`), through the binding's wrapper.  The kernels read hit rows and the per-hit halves 16
bytes at a time, but only from the workspace, which the entry point aligns itself; X, the weights, the tables and every
output are a caller's and may start anywhere.  The counters are zeroed by the call: poison must not show in them.
COVERS maps every function of _lib.FX_SIGNATURES that takes a device pointer to the test here that runs it."""
import ctypes

import numpy as np
import pytest
import torch

import fixed_point_cases as fc
from gnn_fpga_amd import FixedPointFormat, HitGraphBatch
from gnn_fpga_amd import fixed_point as fp
from offset_arrays import shift_batch
from test_gpu_offset_arrays import sweep
from test_gpu_uninitialised import check

pytestmark = pytest.mark.gpu

COVERS = {"gnn_fx_forward": "test_forward"}
NO_ARRAYS = {"gnn_fx_supported", "gnn_fx_workspace_bytes"}

# (graphs, pad_segments, F, D, T, format, gain): the default shape with traces, overflowing sums on lists longer than a
# wave, a wide model (the node MLP's 64 KB and more of LDS) on a padded block-diagonal batch, a batch without segments
CASES = {
    "layered_d8": (lambda: [fc.layered(70, 150, 3, 1)], False, 3, 8, 3, FixedPointFormat(16, 6), 1.0),
    "star_d8_overflow": (lambda: [fc.cached_star(0, 3)], False, 3, 8, 2, FixedPointFormat(16, 3, "rnd", "sat", 12), 2.0),
    "block3_d64": (lambda: [fc.layered(70, 150, 3, 1), fc.layered(33, 41, 3, 2), fc.cached_star(5, 3)], True, 3, 64, 1,
                   FixedPointFormat(24, 8, "trn", "wrap", 12), 1.0),
    "muon_d16_no_segments": (lambda: [fc.layered(40, 50, 11, 3)._replace(src=np.zeros(0, np.int32),
                                                                          dst=np.zeros(0, np.int32),
                                                                          y=np.zeros(0, np.float32))], False, 11, 16, 2,
                             FixedPointFormat(8, 3), 1.0),
}


def test_covers_every_entry_point(hip):
    takes_pointer = {n for n, (_, args) in hip.FX_SIGNATURES.items()
                     if any(a is ctypes.c_void_p or isinstance(a, type(ctypes.POINTER(ctypes.c_int))) for a in args)}
    assert takes_pointer == set(COVERS) and takes_pointer | NO_ARRAYS == set(hip.FX_SIGNATURES)
    assert all(v in globals() for v in COVERS.values())


@pytest.mark.parametrize("case", sorted(CASES))
def test_forward(hip, case):
    from gnn_fpga_amd import _lib
    graphs, pad, F, D, T, f, gain = CASES[case]
    hb = HitGraphBatch.from_graphs(graphs(), pad_segments=pad)
    weights = [w * np.float32(gain) for w in fc.host_weights(fc.default_model(F, D, T))]
    q = [torch.from_numpy(w.astype(np.int32)) for w in fp.quantize_weights(weights, f)]
    tabs = [torch.from_numpy(t.astype(np.int32)) for t in fp.activation_tables(f)]
    fmt = _lib.fx_format_struct(*f._key())

    def call(S=None):
        s = S if S is not None else (lambda t: t)
        b = shift_batch(hb, S if S is not None else 0)
        params = _lib.fx_params_struct([s(t.cuda()) for t in q], F, D)
        tables = _lib.fx_tables_struct(s(tabs[0].cuda()), s(tabs[1].cuda()), f.table_bits)
        plain = _lib.fx_forward(b, params, fmt, tables, T)
        traced = _lib.fx_forward(b, params, fmt, tables, T, trace=True)
        assert plain[3] is None and plain[4] is None
        for a, c in zip(plain[:3], traced[:3]):
            assert torch.equal(a, c)
        return list(traced)

    raw, scores, counts, et, Ht = (t.cpu().numpy() for t in check(call))
    sweep(call)
    want = fp.fixed_forward_numpy(hb.X.numpy(), hb.src.numpy(), hb.dst.numpy(), weights, T, f)
    for got, w in ((raw, want.raw), (counts, want.counts), (et, want.e_trace), (Ht, want.H_trace)):
        assert got.dtype == w.dtype and np.array_equal(got, w)
    assert np.array_equal(scores.view(np.uint32), want.scores.view(np.uint32))
    if case == "star_d8_overflow":
        assert counts.sum() > 0
