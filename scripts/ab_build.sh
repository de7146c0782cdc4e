#!/bin/bash
# Generic A/B on the GPU box.  Usage: bash scripts/ab_build.sh TAG1 "FLAGS1" TAG2 "FLAGS2" ...   (FLAGS = extra hipcc flags,
# "" = the default build).  Per arm: rebuild if needed, per-shape GEMM times, step time, FETCH traffic of the GEMM kernels.
# Results go to $OUT (default bench_out/).
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
cd $ROOT
OUT=${OUT:-bench_out}
mkdir -p $OUT
run() {
  tag=$1
  python scripts/bench_gemm.py --no-torch --iters 20 > $OUT/ab_${tag}_gemm.txt 2>&1
  python bench.py --steps 8 --warmup 3 --full --no-cpu-baseline --no-dense-compare > $OUT/ab_${tag}_bench.json 2> $OUT/ab_${tag}_bench.err
  (cd /tmp && export TMPDIR=/tmp && rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $ROOT/$OUT/ab_${tag}_fetch -- python3 $ROOT/bench.py --serial-towers --steps 1 --warmup 1 --full --no-cpu-baseline --no-dense-compare > $ROOT/$OUT/ab_${tag}_fetch.log 2>&1)
  python scripts/pmc_summary.py $OUT/ab_${tag}_fetch | grep -A1 "gemm_bf16" > $OUT/ab_${tag}_fetch.txt
  rm -rf $OUT/ab_${tag}_fetch
  echo "== $tag"; grep -v wgrad $OUT/ab_${tag}_gemm.txt | tail -17
  python - <<PY
import json
try:
    r=json.loads(open("$OUT/ab_${tag}_bench.json").read().strip().splitlines()[-1])
    print("$tag ms/step", r["ms_per_step"], "NT avg us", r["roofline"]["avg_launch_us"], "TF", r["roofline"]["achieved"], "alg bytes", r["roofline"]["algorithmic_bytes_per_launch"])
except Exception as e:
    print("$tag bench failed", e); print(open("$OUT/ab_${tag}_bench.err").read()[-1500:])
PY
  grep -v "^--" $OUT/ab_${tag}_fetch.txt | paste - - | awk '{print $1, $2, $(NF-2)}' | cut -c1-120
}
first=1
while [ $# -ge 2 ]; do
  tag=$1; flags=$2; shift 2
  if [ $first -eq 0 ] || [ -n "$flags" ]; then
    CLIPX_EXTRA_FLAGS="$flags" python -m colxlip_amd.build --force > $OUT/ab_build_${tag}.log 2>&1 || { echo "build failed for $tag"; tail -5 $OUT/ab_build_${tag}.log; continue; }
  fi
  first=0
  run $tag
done
