"""What tests/test_gpu_route_values.py rests on, recomputed on the CPU (tests/route_cases.py):

  - under the cases' upstream gradient every gradient tensor of the fp64 reference that is not identically zero has
    a largest entry of at least MIN_SCALE = 0.05, so golden_util.GRAD_ABS is below 4 % of GRAD_REL * scale and the
    comparison is a relative one;
  - the cases return every (BwdStart, BwdIter, fuse_fin_hit) choose_bwd_route can return, and the matrix holds every
    shape the library reports as supported (asked, not listed);
  - the float32 CPU oracle (oracle.index_torch / nodeclf_fp64 in float32) meets GRAD_REL on every case over three
    segment orders: the bound asks nothing of the kernels that float32 cannot give (measured: at most 6.6e-7);
  - the bound can see one segment: the fp64 reference without the valid segment of the largest upstream gradient lies
    more than 10 x GRAD_REL of the largest entry from the true one, in each of the ten tensors, for one case per
    iteration form (measured: 2.2e-4 ... 3.4e-3, 44 x the bound or more).
"""
import numpy as np
import pytest
import torch

import route_cases as rc
from golden_util import GRAD_ABS, GRAD_REL

CASES = rc.backward_cases()
IDS = [rc.case_id(c) for c in CASES]


def test_the_weights_are_in_the_oracles_key_order():
    from gnn_fpga_amd.model import SegmentClassifier
    assert list(SegmentClassifier(input_dim=3, hidden_dim=8, n_iters=1).state_dict()) == list(rc.KEYS)
    assert list(rc.nodeclf_fp64.KEYS[:10]) == list(rc.KEYS)


def test_the_recorded_cases_lead_the_list_and_names_are_unique():
    names = [c["name"] for c in CASES]
    assert names[:len(rc.bwd.CASES)] == list(rc.RECORDED_BWD) and len(set(names)) == len(names)
    assert not set(c["name"] for c in rc.matrix_cases()) & set(rc.RECORDED_BWD)
    for name in rc.INTO_CASES:
        assert rc.case_named(name)["kind"] in ("segclf", "events")
    into = [rc.case_named(n) for n in rc.INTO_CASES]
    assert {rc.route_of(c)[1] if rc.route_of(c) else c["kind"] for c in into} == {"quad", "wide", "events"}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_gradient_tensor_is_large_against_the_absolute_floor(case):
    ref = rc.REFS.backward(case)
    names = rc.tensor_names(case)
    assert len(ref) == len(names)
    zero = [n for n, r in zip(names, ref) if not np.any(r)]
    # at T = 0 there is no node pass: its four tensors are identically zero, and nothing else is anywhere
    assert zero == ([k for k in names if k.startswith("node_network")] if case["T"] == 0 else []), zero
    for n, r in zip(names, ref):
        if np.any(r):
            scale = float(np.abs(r).max())
            assert scale >= rc.MIN_SCALE, (case["name"], n, scale)
            assert GRAD_ABS <= 0.04 * GRAD_REL * scale


def test_upstream_gradients_are_positive_of_order_one_and_undivided():
    for case in CASES:
        go = rc.upstream(case)
        s = rc.UPSTREAM_SCALE.get(case["kind"], 1.0)
        assert go.dtype == torch.float32 and float(go.min()) >= 0.5 * s and float(go.max()) < 1.5 * s
        assert torch.equal(go, rc.upstream(case))                  # seeded


def test_the_cases_return_every_route_the_decision_can():
    got = {rc.route_of(c) for c in CASES} - {None}
    assert got == rc.reachable_routes()
    # (3 starts x 4 forms x 2, less what the decision excludes)
    assert len(got) == 10
    recorded = {rc.route_of(c) for c in rc.bwd.CASES} - {None}
    assert rc.reachable_routes() - recorded == {("seeded_head", "quad", False)}
    # the triple and the kernel names of a case say the same
    for c in CASES:
        r = rc.route_of(c)
        if r is None:
            continue
        start, it, fuse = r
        names, T = rc.kernels_of(c), c["T"]
        assert (names[0] == "k_head_bwd") == (start == "seeded_head")
        assert (names[:4] == rc.WIDE + ["k_edge_bwd"]) == (start == "wide_final_pass")
        assert (names[:3] == rc.EDGE_PASS) == (start == "edge_pass")
        assert names.count("k_seg_bwd4") == (T if it == "quad" else 0)
        assert names.count("k_seg_bwd") == (T if it == "one_lane" else 0)
        assert names.count("k_seg_bwdW") == (T + (start == "wide_final_pass") if it == "wide" else 0)
        assert names.count("k_node_bwd") == (T if it == "per_pass" else 0)
        assert names.count("k_fin_hit") == (T - 1 if fuse and T > 0 else 0)
        assert names.count("k_hit_bwd4") == (0 if it != "quad" else 1 if fuse else T)


def test_the_derived_kernels_of_the_recorded_cases_are_the_recorded_ones():
    for case in rc.bwd.CASES:
        assert rc.kernels_of(case) == rc.RECORDED_BWD[case["name"]], case["name"]


def test_the_matrix_holds_every_supported_shape():
    from gnn_fpga_amd import _lib
    shapes = [(F, D) for F in range(1, 17) for D in (4, 8, 16, 32, 64) if _lib.shape_supported(F, D)]
    assert len(shapes) >= 16
    per_pass = [c for c in CASES if c["kind"] == "segclf" and c["env"] is None]       # the matrix and the recorded ones
    for F, D in shapes:
        mine = {(c["T"], c["q"] and c["T"] > 0) for c in per_pass if (c["F"], c["D"]) == (F, D)}
        assert mine >= {(2, True), (2, False), (0, False)}, (F, D, mine)
    ev = rc.host_batch(rc.case_named("one launch 3x8 T=2"))
    mh, ms = int(np.diff(ev.hit_ptr).max()), int(np.diff(ev.seg_ptr).max())
    assert (ev.n_graphs, mh) == (3, 40)
    events = {(c["F"], c["D"]) for c in CASES if c["kind"] == "events" and c["T"] == 2}
    assert events == {s for s in shapes if _lib.events_backward_supported(s[0], s[1], mh, ms)} and len(events) >= 9
    b = rc.host_batch(rc.case_named("3x8 T=3 Q"))
    assert (b.n_hits, b.n_segments) == (909, 6011) and int((b.src.numpy() < 0).sum()) == len(range(7, 6011, 13))


_ORACLE_KEYS = sorted({rc.ref_key(c): c["name"] for c in reversed(CASES) if c["kind"] != "big"}.items())


@pytest.mark.parametrize("case_name", [n for _, n in _ORACLE_KEYS])
def test_the_float32_oracle_meets_the_bound(case_name):
    """(`big` apart: 270 k segments three times over would take the file past a minute; its shape and T are covered by
    "3x8 T=1 Q" on the small batch.)"""
    case = rc.case_named(case_name)
    ref = rc.REFS.backward(case)
    for o in rc.orders(case, 3):
        got = rc.reference(case, dtype=torch.float32, order=o)
        for n, err in zip(rc.tensor_names(case), rc.rel_errors(got, ref)):
            assert err < GRAD_REL, (case_name, n, err)


def test_every_case_has_a_float32_oracle_run():
    keys = {k for k, _ in _ORACLE_KEYS}
    assert all(rc.ref_key(c) in keys for c in CASES if c["kind"] != "big")


# one case per iteration form: quad, one_lane, wide, per_pass
@pytest.mark.parametrize("case_name", ["3x8 T=3 Q", "3x8 T=2 no Q", "3x64 T=1 Q", "3x32 T=2 no Q"])
def test_the_bound_sees_one_dropped_segment(case_name):
    case = rc.case_named(case_name)
    b = rc.host_batch(case)
    go = rc.upstream(case).numpy().copy()
    go[b.src.numpy() < 0] = -np.inf
    j = int(go.argmax())                                   # exactly one segment, the one with the largest gradient
    assert b.src.numpy()[j] >= 0
    ref = rc.REFS.backward(case)
    dropped = rc.reference(case, drop=j)
    assert len(ref) == len(dropped) == 10
    for n, r, d in zip(rc.tensor_names(case), ref, dropped):
        miss = float(np.abs(d - r).max()) / float(np.abs(r).max())
        assert miss > 10 * GRAD_REL, (case_name, n, miss)
