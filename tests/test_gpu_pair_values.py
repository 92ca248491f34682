"""The graph builder's pair arithmetic pinned on its values, on the MI355X: csrc/graph_build.hip (k_gb_pairs<0>,
k_gb_pairs<1>, k_cs_pairs) against the independent restatement of tests/pair_value_cases.py, with cuts and edges placed
on the float32 values themselves, single pairs at the arithmetic's corners, and layers on the kernels' row and tile
sizes.  tests/test_pair_values_host.py shows that these checks fail for a reciprocal-multiply and for an unrounded
dphi."""
import pytest

import pair_value_cases as pv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def device(ev):
    return pv.columns(ev.cols, DEV)


@pytest.mark.parametrize("variant", pv.PROBE_VARIANTS)
def test_every_value_through_the_cut_study(hip, variant):
    """45 (25) study calls with one-ulp bins on every |phi_slope| and |z0| of the probe event: the multiset of float32
    values per (layer pair, class) is the restatement's, to the bit."""
    assert pv.check_value_probe(device(pv.probe_event(variant)), variant) == {"one": 45, "front": 25}[variant]


@pytest.mark.parametrize("axis", ["slope", "z0"])
@pytest.mark.parametrize("variant", pv.PROBE_VARIANTS)
def test_cuts_on_the_values(hip, variant, axis):
    """The cut at a value v and at next(v), exact and a quarter of an ulp inside: src, dst, y and seg_ptr are the
    restatement's, the builds differ by exactly the pairs at v, and the study's kept counts are the builder's."""
    pv.check_cuts_on_values(device(pv.probe_event(variant)), variant, axis)


def test_hand_made_pairs(hip):
    """dphi on +-f32(pi) and one ulp either side, dr = 0 (inf and NaN), +-0, a subnormal quotient, z0 = -0, a large
    finite value below an edge of +inf: the bins and the kept flags of the restatement."""
    pv.check_hand_made(device(pv.hand_made()))


@pytest.mark.parametrize("variant", pv.TILE_VARIANTS)
def test_row_and_tile_edges(hip, variant):
    """Layers of 129, 513, 128, 512, 127, 511, 257, 1025, 1 and 1 hits: X, src, dst, y, hit_index, both pointers and one
    9 x 9 cut study against the specification."""
    ev = pv.tile_event(variant)
    c = device(ev)
    pv.check_tile_edges(c, variant)
    b = pv.run_build(c, ev, pv.TILE_CUTS)
    assert b.X.is_cuda and b.src.is_cuda and b.n_segments > 90000


def test_fixture_cuts_one_ulp_up(hip):
    """The reference-made fixture's cuts sit on values: one ulp further up, each cut lets exactly one more pair in."""
    ev = pv.probe_event("one")
    c = device(ev)
    cuts = pv.fixture_cuts()
    n = pv.run_build(c, ev, cuts).n_segments
    for k in range(3):
        above = list(cuts)
        above[k] = float(pv.up(cuts[k]))
        assert pv.run_build(c, ev, above).n_segments == n + 1, k
