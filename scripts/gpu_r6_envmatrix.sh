#!/bin/bash
# Same-box matrix of environment switches:  gpu_r6_envmatrix.sh "<label>:<ENV=V ...>;..." "cfg:steps ..." [reps]
export TMPDIR=/tmp
mkdir -p bench_out
IFS=';' read -ra RUNS <<< "$1"
run() {
  local label=$1 cfg=$2 steps=$3; shift 3
  env "$@" timeout 300 python bench.py --full --config $cfg --steps $steps --warmup 2 --cpu-sample 0 --no-convergence --no-lisi > bench_out/w.json 2> bench_out/w.err
  python - "$label" "$cfg" <<'PY'
import json, sys
try:
    d = json.loads(open("bench_out/w.json").read().splitlines()[0])
    r = d.get("roofline", {})
    print(sys.argv[1], sys.argv[2], round(d["value"] / 1e6, 2), "M", round(d["ms_per_step"], 3), "ms", "dominant_us", round(r.get("avg_launch_us", 0), 1), d.get("kernel_ms_per_step"))
except Exception as ex:
    print(sys.argv[1], sys.argv[2], "FAILED", ex, open("bench_out/w.err").read()[-800:])
PY
}
for rep in $(seq 1 ${3:-2}); do
  for cs in ${2:-c3:10 c2:40}; do
    for r in "${RUNS[@]}"; do run "${r%%:*}" ${cs%%:*} ${cs##*:} X=1 ${r#*:}; done
  done
done 2>&1 | tee bench_out/envmatrix.txt
