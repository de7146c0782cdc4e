#!/bin/bash
# A/B over ENVIRONMENT settings on one build: bash scripts/ab_env.sh TAG1 "VAR=1 VAR2=2" TAG2 "" ...
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
cd $ROOT
OUT=${OUT:-bench_out}     # results
mkdir -p $OUT
while [ $# -ge 2 ]; do
  tag=$1; envs=$2; shift 2
  env $envs python scripts/bench_gemm.py --no-torch --iters 20 > $OUT/abe_${tag}_gemm.txt 2>&1
  env $envs python bench.py --steps 8 --warmup 3 --full --no-cpu-baseline --no-dense-compare > $OUT/abe_${tag}_bench.json 2> $OUT/abe_${tag}_bench.err
  echo "== $tag ($envs)"; grep -v wgrad $OUT/abe_${tag}_gemm.txt | tail -17
  python - <<PY
import json
try:
    r=json.loads(open("$OUT/abe_${tag}_bench.json").read().strip().splitlines()[-1])
    print("$tag ms/step", r["ms_per_step"], "NT avg us", r["roofline"]["avg_launch_us"], "TF", r["roofline"]["achieved"])
except Exception as e:
    print("$tag bench failed", e); print(open("$OUT/abe_${tag}_bench.err").read()[-800:])
PY
done
