# timing-only builds of sell_pipeline.hip with extra -D flags (results invalid), e.g.
#   VARIANTS="|-DGNN_TIMING_EXPPROD" bash tools/ablate_build.sh
# Each variant is built by the Makefile's `variant` target (its own list of units) over the in-tree libgnn_hip.so,
# which is saved first and put back on exit, whatever happens (a timing build must never be left in the
# tree).
set -eo pipefail
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
cd $ROOT
LIB=gnn-fpga_amd/libgnn_hip.so
cp $LIB /tmp/libgnn_hip.keep.so
trap 'cp /tmp/libgnn_hip.keep.so $LIB' EXIT
IFS='|' read -ra VS <<< "${VARIANTS:-|-DGNN_ABLATE_TRANS|-DGNN_ABLATE_LDS}"
for variant in "${VS[@]}"; do
  make -C gnn-fpga_amd/csrc --no-print-directory -j16 variant VARIANT_FLAGS="-DGNN_DIAG $variant" VARIANT_OBJ=/tmp/sell_ab.o VARIANT_OUT=$PWD/$LIB
  timeout -k 10 200 python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-train --no-pruned --no-c5 ${BENCH_ARGS:-} | python -c "
import json,sys; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('variant [$variant]', d['ms_per_step'], d['roofline']['kernel_ms'])"
done
