"""The per-iteration kernels' shape matrix without a GPU (tests/toy_mpnn_cases.py): MATRIX is what csrc/iter_events.hip
builds, the two batches every shape runs on are what their description says, and the bounds of
test_gpu_toy_mpnn_shapes.py can see the faults those runs are there to catch - a mis-wired weight set and a backward that
forgets the padded segments - in fp64 on the CPU alone."""
import os
import re

import numpy as np
import pytest
import torch

import toy_mpnn_fp64 as ref
from gnn_fpga_amd import HitGraphBatch, _lib, synth
from gnn_fpga_amd.call_route import EVENTS_MAX_GRAPHS
from toy_mpnn_cases import (BATCH_SIZES, MATRIX, MATRIX_CAPS, MATRIX_T, host_arrays, matrix_batch, matrix_reference,
                            random_graph)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_matrix_is_every_shape_the_library_builds():
    """A shape added to IterShapes and not to MATRIX (or the reverse) fails here: no built shape goes unrun."""
    built = {(F, D) for F in range(1, 17) for D in range(1, 65) if _lib.iter_events_supported(F, D, 1, 1, False)}
    assert len(MATRIX) == len(set(MATRIX)) == 14
    assert built == set(MATRIX), "built and not in MATRIX: %s; in MATRIX and not built: %s" % (
        sorted(built - set(MATRIX)), sorted(set(MATRIX) - built))
    src = open(os.path.join(REPO, "gnn-fpga_amd", "csrc", "iter_events.hip")).read()
    listed = re.search(r"using IterShapes = ShapeList<(.*?)>;", src, flags=re.S).group(1)
    assert [(int(a), int(b)) for a, b in re.findall(r"Shape<(\d+), (\d+)>", listed)] == MATRIX
    # both matrix batches take the one-launch route, forward and backward, at every shape
    assert MATRIX_CAPS == (40, 144)
    for F, D in MATRIX:
        assert _lib.iter_events_supported(F, D, 40, 144, True), (F, D)


def test_the_batches_are_what_they_claim():
    assert BATCH_SIZES["ragged"] == [(30, 70), (1, 0), (9, 0), (2, 1), (40, 144), (17, 33)]
    assert BATCH_SIZES["padded"] == [(40, 144), (35, 120), (30, 100)]
    for F, D in [(2, 4), (11, 16)]:
        r = matrix_batch(F, D, "ragged")
        X, src, dst, y = host_arrays(r)
        assert (r.n_graphs, r.n_hits, r.n_segments) == (6, 99, 248) and r.dense_shape is None and X.shape == (99, F)
        assert (src >= 0).all() and np.abs(X).max() <= 1.0 and X.dtype == np.float32
        lay = r.event_layout()
        assert lay is not None and (lay.max_hits, lay.max_segments) == MATRIX_CAPS
        used = np.zeros(r.n_hits, bool)
        used[src] = used[dst] = True
        hp = np.asarray(r.hit_ptr)
        for i, (nh, ns) in enumerate(BATCH_SIZES["ragged"]):
            lone = (~used[hp[i]:hp[i + 1]]).sum()
            assert lone >= 1 if nh >= 3 or ns == 0 else lone == 0, (i, lone)
        p = matrix_batch(F, D, "padded")
        X, src, dst, y = host_arrays(p)
        assert p.dense_shape == (3, 40, 144) and p.n_segments == 432 and int((src < 0).sum()) == 68
        assert np.array_equal(src < 0, dst < 0) and not y[src < 0].any()
        assert np.array_equal(np.diff(np.asarray(p.seg_ptr)), [144] * 3) and 4 * 68 < 432
        lay = p.event_layout()
        assert lay is not None and (lay.max_hits, lay.max_segments) == MATRIX_CAPS


def test_counts_that_reach_the_kernels():
    """What test_gpu_toy_mpnn_shapes.py launches is not refused on the host: graphs without hits keep the event layout,
    and so do EVENTS_MAX_GRAPHS graphs."""
    rng = np.random.default_rng(0)
    g = random_graph(rng, 17, 33, 2)
    z = synth.HitGraph(np.zeros((0, 2), np.float32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    for graphs, caps in (([g, z, g], (17, 33)), ([z, g], (17, 33)), ([g, z], (17, 33)), ([z], (0, 0))):
        lay = HitGraphBatch.from_graphs(graphs).event_layout()
        assert lay is not None and (lay.max_hits, lay.max_segments) == caps
    assert _lib.iter_events_supported(2, 8, 0, 0, True)
    many = HitGraphBatch.from_graphs([random_graph(rng, 3, 2, 2, lone=False) for _ in range(EVENTS_MAX_GRAPHS)])
    assert EVENTS_MAX_GRAPHS == 1024 and many.n_graphs == 1024 and many.event_layout() is not None


# ---- the bounds can see the faults ---------------------------------------------------------------------------------------
OUTPUT_KEYS = ["output_network.network.0.bias", "output_network.network.2.weight", "output_network.network.2.bias"]


def forgetful_grads(params, X, src, dst, y, T):
    """fp64 gradients of a backward that forgets the padded segments: the loss summed over the real segments only,
    divided by the count of all of them."""
    p = {k: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for k, v in params.items()}
    s, d = (torch.tensor(a, dtype=torch.int64) for a in (src, dst))
    es, _ = ref.forward(p, torch.tensor(X, dtype=torch.float64), s, d, T)
    real = s >= 0
    loss = torch.nn.BCELoss(reduction="sum")(es[-1][real], torch.tensor(y, dtype=torch.float64)[real]) / len(s)
    loss.backward()
    return {k: v.grad.numpy() for k, v in p.items()}


@pytest.mark.parametrize("F,D", MATRIX)
def test_the_bounds_see_the_faults(F, D):
    """On the padded batch of every shape: exchanging the weight sets of passes 0 and 1, or scoring the last pass with
    output_network, moves the final scores by more than 10 x their bound; forgetting the padded segments in the
    backward moves output_network's first bias and second layer by more than 10 x each tensor's bound."""
    T = MATRIX_T
    params, r64, own = matrix_reference(F, D, False, "padded")
    X, src, dst, y = host_arrays(matrix_batch(F, D, "padded"))
    for f in (("swap", 0), ("out_for_last",)):
        got = ref.run(params, X, src, dst, None, T, faults=(f,))
        moved = float(np.abs(got["e"][T] - r64["e"][T]).max())
        print("  (%d, %d) %-20s moves the scores by %.2e = %.0f x the bound" % (F, D, f, moved, moved / ref.SCORE_BOUND))
        assert moved > 10 * ref.SCORE_BOUND, f
    forgot = forgetful_grads(params, X, src, dst, y, T)
    for k in OUTPUT_KEYS:
        moved, bound = ref.rel_err(forgot[k], r64["grads"][k]), ref.grad_bound(own[k])
        print("  (%d, %d) forgetting the padded segments moves %s by %.2e, bound %.2e" % (F, D, k, moved, bound))
        assert moved > 10 * bound, k
    print("  (%d, %d) the reference's own fp32 error: at most %.2e" % (F, D, max(own.values())))
