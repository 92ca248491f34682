# GPU box: wide-shape parity tests, then the c5 line (exact fp32 timed, bf16 beside it); logs go to $OUT
set -e
OUT=${OUT:-${TMPDIR:-/tmp}/c5_quick}
mkdir -p "$OUT"
python -m pytest tests -m gpu -x -q -k "golden or wide or c5 or bf16 or matrix" > "$OUT/tests.log" 2>&1 || { tail -30 "$OUT/tests.log"; exit 1; }
tail -2 "$OUT/tests.log"
python bench.py --full --workload c5 --dtype f32 --steps 20 --warmup 5 --no-train --no-cpu-baseline > "$OUT/f32.json" 2>"$OUT/bench.err"
python - "$OUT/f32.json" <<P
import json, sys
d=json.load(open(sys.argv[1])); r=d["roofline"]
print("f32 ms", round(d["ms_per_step"],4), "other(bf16)", round(d["other_dtype"]["ms_per_step"],4), r["launch_sequence_ms"])
P
