#!/bin/bash
# A / B on ONE box: the in-tree library against a build of sell_pipeline.hip with one more -D switch (e.g.
# -DGNN_NO_PIPE_B), three alternating bench runs each.  The BOX's copy of the library is swapped and put back on
# exit; nothing is written to the repository.  The variant is built by the Makefile's `variant` target (its own
# list of units); AB_VARIANT_LIB=<library> takes one that target built earlier instead of building now.
# usage: bash tools/ab_build.sh -DGNN_NO_PIPE_B [bench args]
#        bash tools/ab_build.sh -DGNN_NO_TRIM / -DGNN_FORWARD_WALK    (profiles/trim_walk_ab.txt: same scores, other work)
#        bash tools/ab_build.sh -DGNN_QUAD_SWEEP                      (profiles/lane_sweep_ab.txt: sweep16 everywhere)
set -eo pipefail
FLAG=${1:?switch}; shift || true
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
cd $ROOT
LIB=gnn-fpga_amd/libgnn_hip.so
cp $LIB /tmp/ab_a.so
trap 'cp /tmp/ab_a.so $LIB' EXIT
if [ -n "$AB_VARIANT_LIB" ]; then
  cp "$AB_VARIANT_LIB" /tmp/ab_b.so
else
  make -C gnn-fpga_amd/csrc --no-print-directory -j16 variant VARIANT_FLAGS="$FLAG" VARIANT_OBJ=/tmp/sell_ab.o VARIANT_OUT=/tmp/ab_b.so
fi
for i in 1 2 3; do
  for v in a b; do
    cp /tmp/ab_$v.so $LIB
    timeout -k 10 200 python bench.py --full --steps 100 --warmup 20 --no-cpu-baseline --no-train --no-pruned --no-c5 "$@" | python -c "
import json,sys; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); r=d['roofline']
print('$v' == 'a' and 'in-tree ' or '$FLAG', round(d['ms_per_step'],4), 'first', round(r['launch_ms_first'],4), 'middle', round(r['launch_ms_middle'],4), 'last', round(r['launch_ms_last'],4), 'other', round(r['other_kernels_ms'],4))"
  done
done
