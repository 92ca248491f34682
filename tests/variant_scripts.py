"""What the host tests of every unit check about the variant builds of sell_pipeline.hip (tools/ab_build.sh,
tools/ablate_build.sh): a variant library must hold every unit, or `_lib.load()` refuses it."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assert_variant_libraries_link(unit):
    """`unit` is in the Makefile's UNITS, the `variant` target links every object of that list but sell_pipeline's
    own, and both scripts build through that target instead of naming objects themselves."""
    with open(os.path.join(REPO, "gnn-fpga_amd", "csrc", "Makefile")) as fh:
        mk = fh.read()
    assert unit in re.search(r"^UNITS\s*:=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert re.search(r"^OBJS\s*:=\s*\$\(addprefix \$\(ROOT\)/build/,\$\(addsuffix \.o,\$\(UNITS\)\)\)$", mk, flags=re.M)
    assert re.search(r"^OTHERS\s*:=\s*\$\(filter-out %/sell_pipeline\.o,\$\(OBJS\)\)$", mk, flags=re.M)
    assert re.search(r"^variant: \$\(OTHERS\)\n(\t.*\n)*\t\$\(HIPCC\) .*-shared .*-o \$\(VARIANT_OUT\) \$\(VARIANT_OBJ\) \$\(OTHERS\)$",
                     mk, flags=re.M)
    for tool in ("ab_build.sh", "ablate_build.sh"):
        with open(os.path.join(REPO, "tools", tool)) as fh:
            text = fh.read()
        assert re.search(r"^\s*make -C gnn-fpga_amd/csrc .*\bvariant\b", text, flags=re.M), tool
        assert not re.search(r"build/\w+\.o", text) and "hipcc" not in text, tool
        assert text.count("/dev/null") == 0 and "set -eo pipefail" in text, tool
