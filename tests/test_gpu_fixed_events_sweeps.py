"""gnn_fxev_forward (include/gnn_hip_fixed_events.h) on guarded, poisoned outputs and on arrays that start off the
16-byte grid: the checks every entry point of gnn_hip.h has (test_gpu_uninitialised.py `check`,
test_gpu_offset_arrays.py `sweep`), through the binding's wrapper.  The kernel reads hit rows and the per-hit halves 16
bytes at a time, but only from LDS; X, the lists, hit_ptr / seg_ptr, the weights, the tables and every output are a
caller's and may start anywhere.  The call writes every element of every output - the counters and the per-graph counts
included: poison must not show in them.
COVERS maps every function of _lib.FXEV_SIGNATURES that takes a device pointer to the test here that runs it."""
import ctypes
import types

import numpy as np
import pytest
import torch

import fixed_events_cases as fe
from gnn_fpga_amd import FixedPointFormat
from offset_arrays import shift_batch
from test_gpu_offset_arrays import sweep
from test_gpu_uninitialised import check

pytestmark = pytest.mark.gpu

COVERS = {"gnn_fxev_forward": "test_forward"}
NO_ARRAYS = {"gnn_fxev_supported", "gnn_fxev_lds_bytes"}

# (batch, F, D, T, format, gain): the trigger's batch with every stage overflowing, lists longer than a wave on a padded
# block-diagonal batch, a batch without segments
CASES = {
    "muon64": ("muon64", 11, 8, 3, FixedPointFormat(24, 2, "rnd", "wrap", 10), 2.0),
    "block3_padded": ("block3_padded", 3, 8, 2, FixedPointFormat(16, 3, "rnd", "sat", 12), 2.0),
    "no_segments": ("no_segments", 11, 16, 2, FixedPointFormat(8, 3), 1.0),
}


def test_covers_every_entry_point(hip):
    takes_pointer = {n for n, (_, args) in hip.FXEV_SIGNATURES.items()
                     if any(a is ctypes.c_void_p or isinstance(a, type(ctypes.POINTER(ctypes.c_int))) for a in args)}
    assert takes_pointer == set(COVERS) and takes_pointer | NO_ARRAYS == set(hip.FXEV_SIGNATURES)
    assert all(v in globals() for v in COVERS.values())


@pytest.mark.parametrize("case", sorted(CASES))
def test_forward(hip, case):
    kind, F, D, T, f, gain = CASES[case]
    hb = fe.host_batch(kind, F)
    weights = fe.gained(F, D, T, gain)
    sizes = (int(np.diff(hb.hit_ptr).max()), int(np.diff(hb.seg_ptr).max()))
    assert hip.fxev_supported(F, D, f.table_bits, *sizes)

    def call(S=None):
        s = S if S is not None else (lambda t: t)
        b = shift_batch(hb, S if S is not None else 0)
        params, fmt, tables = fe.device_args(weights, f, F, D, s)
        assert b.event_layout() is not None
        lay = types.SimpleNamespace(hit_ptr=s(torch.from_numpy(hb.hit_ptr.astype(np.int32)).cuda()),
                                    seg_ptr=s(torch.from_numpy(hb.seg_ptr.astype(np.int32)).cuda()),
                                    max_hits=sizes[0], max_segments=sizes[1])
        plain = hip.fxev_forward(b, lay, params, fmt, tables, T)
        traced = hip.fxev_forward(b, lay, params, fmt, tables, T, trace=True)
        assert plain[4] is None and plain[5] is None
        for a, c in zip(plain[:4], traced[:4]):
            assert torch.equal(a, c)
        return list(traced)

    raw, scores, counts, per_graph, et, Ht = (t.cpu().numpy() for t in check(call))
    sweep(call)
    want = fe.spec(hb, weights, T, f)
    for got, w in ((raw, want.raw), (counts, want.counts), (et, want.e_trace), (Ht, want.H_trace)):
        assert got.dtype == w.dtype and np.array_equal(got, w)
    assert np.array_equal(scores.view(np.uint32), want.scores.view(np.uint32))
    assert np.array_equal(per_graph, [int(p.counts.sum()) for p in fe.spec_per_graph(hb, weights, T, f)])
    assert per_graph.sum() == counts.sum() and (counts.sum() > 0 or case == "no_segments")
