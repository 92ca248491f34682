"""The entry points beside their kernels and the one shape dispatch (csrc/core.hip, csrc/common.h ShapeList) without a
GPU: every shape and size query, and every refusal that comes before a launch, answers as the library did when all of
them stood in csrc/gnn_kernels.hip behind four macro lists (tests/abi_units_cases.py asks,
tools/gen_abi_units_golden.py recorded tests/golden/abi_units/*.json from that earlier build)."""
import glob
import json
import os
import re

import abi_units_cases as cases
from gnn_fpga_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "abi_units")
CSRC = os.path.join(REPO, "gnn-fpga_amd", "csrc")


def _recorded(name):
    with open(os.path.join(GOLDEN, name)) as fh:
        return json.load(fh)


def test_shape_answers_equal_the_recorded_ones():
    """input_dim 1 .. 12 x hidden_dim {1, 4, 8, 12, 16, 32, 64, 128}, sizes {0, 1, 300, 5000}: fifteen queries, every
    list and every miss path at every shape, listed or not."""
    want = _recorded("shape_answers.json")
    grid = want.pop("grid")
    assert grid == {"F": cases.FS, "D": cases.DS, "sizes": cases.SIZES, "fx_formats": [list(f) for f in cases.FX_FORMATS],
                    "iter_counts": cases.ITER_COUNTS}, "the recorded grid is not the one asked"
    got = cases.shape_answers(_lib.load())
    assert sorted(got) == sorted(want)
    assert len(got) == 15
    for name in want:
        per = len(want[name]) // (len(cases.FS) * len(cases.DS))
        assert len(got[name]) == len(want[name]) == per * len(cases.FS) * len(cases.DS), name
        for i, (a, b) in enumerate(zip(got[name], want[name])):
            shape = (cases.FS[i // per // len(cases.DS)], cases.DS[i // per % len(cases.DS)])
            assert a == b, "%s at (input_dim, hidden_dim) = %s, answer %d of %d: %r, recorded %r" % (
                name, shape, i % per, per, a, b)
    # the recorded table is not empty-handed: the sixteen model shapes, twelve of them planned, are in it
    assert sum(want["gnn_shape_supported"]) == 16 and sum(want["gnn_plan_shape_supported"]) == 12


def test_refusals_equal_the_recorded_ones():
    """(return code, gnn_last_error()) of every moved or re-dispatched entry point on the all-null call and on a shape
    without kernels - (5, 7) everywhere, and the shapes that only one list lacks - word for word."""
    want = _recorded("refusals.json")
    got = cases.refusals(_lib.load())
    assert list(got) == list(want)
    for label in want:
        assert got[label] == want[label], label
    assert all(rc in (0, _lib.GNN_ERR_BADARG, _lib.GNN_ERR_UNSUPPORTED) and msg for rc, msg in want.values())


def test_no_cross_unit_declarations():
    """common.h declares nothing of the three units that own their entry points, and no unit writes a shape dispatch
    out as a macro block."""
    with open(os.path.join(CSRC, "common.h")) as fh:
        common = fh.read()
    code = re.sub(r"//[^\n]*", "", common)           # (comments may name the units)
    for word in ("sell_", "backward", "edge_bwd", "node_bwd", "bce_loss"):
        assert word not in code, "common.h still declares something with %r" % word
    sources = glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))
    assert len(sources) > 20
    for path in sources:
        with open(path) as fh:
            assert "#define X_" not in fh.read(), os.path.basename(path)
