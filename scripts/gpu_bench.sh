#!/bin/bash
# The full bench run (bench.py --full), its JSON line kept as $OUT/<tag>.json (OUT defaults to bench_out).
#   OUT=<dir> bash scripts/gpu_bench.sh [tag] [extra bench.py args]
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
tag=${1:-bench}; shift || true
python bench.py --full --steps 20 --warmup 5 "$@" 2> "$OUT/${tag}.err" | tail -1 > "$OUT/${tag}.json"
python - "$OUT/${tag}.json" <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
keep = {k: d[k] for k in ("metric", "value", "ms_per_step", "roofline", "parity") if k in d}
keep["extras"] = d.get("extras")
keep["hot_path"] = d.get("hot_path")
print(json.dumps(keep, indent=1)[:6000])
PY
