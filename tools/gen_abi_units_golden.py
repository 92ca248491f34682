"""Records tests/golden/abi_units/shape_answers.json and refusals.json (tests/abi_units_cases.py says what is asked):
the answers of the shape and size queries over a grid of shapes, and the (return code, message) of calls that every
entry point refuses before a launch.  Recorded results only; no GPU is needed.

The files pin the library as it was BEFORE the entry points moved next to their kernels, so they are made from a build
of that commit: check it out elsewhere, `make -C gnn-fpga_amd/csrc` there, and pass its library.

usage: python tools/gen_abi_units_golden.py --lib /path/to/the/earlier/libgnn_hip.so
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
OUT = os.path.join(REPO, "tests", "golden", "abi_units")

import abi_units_cases as cases  # noqa: E402


def write(name, table):
    """One key per line: a diff of a recorded file shows which entry point moved."""
    lines = ["%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in table.items()]
    with open(os.path.join(OUT, name), "w") as fh:
        fh.write("{\n" + ",\n".join(lines) + "\n}\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", required=True, help="the library to record")
    args = ap.parse_args()
    lib = cases.bind(os.path.abspath(args.lib))
    os.makedirs(OUT, exist_ok=True)
    grid = {"F": cases.FS, "D": cases.DS, "sizes": cases.SIZES, "fx_formats": cases.FX_FORMATS,
            "iter_counts": cases.ITER_COUNTS}
    write("shape_answers.json", {"grid": grid, **cases.shape_answers(lib)})
    write("refusals.json", cases.refusals(lib))


if __name__ == "__main__":
    main()
