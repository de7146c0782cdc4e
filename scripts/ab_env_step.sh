#!/bin/bash
# whole-step A/B over environment settings on one box: bash scripts/ab_env_step.sh "VAR=a" "VAR=b" ...
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
cd $ROOT
OUT=${OUT:-bench_out}/ab     # results
mkdir -p $OUT
i=0
for e in "$@"; do
  i=$((i+1))
  env $e timeout -k 10 240 python bench.py --steps 8 --warmup 3 --full --no-cpu-baseline --no-dense-compare > $OUT/step_$i.json 2> $OUT/step_$i.err || { tail -5 $OUT/step_$i.err; exit 1; }
  python - "$e" $OUT/step_$i.json <<'PY'
import json, sys
r = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
print(sys.argv[1], "ms/step", r["ms_per_step"], "NT TF", r["roofline"]["achieved"], "avg us", r["roofline"]["avg_launch_us"])
PY
done
