#!/bin/bash
# Kernel-level picture of the 8-GPU operating point (per-GPU batch 512): bench lines at 512 / 1024 / 2048 + rocprofv3 kernel
# stats of the b=512 step, towers on one stream (per-kernel durations are then not inflated by the other tower's kernels) and
# on two (what the step really runs).
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
cd $ROOT
OUT=gpurun_out/${1:-b512_r3}
mkdir -p $OUT
for B in 512 1024 2048; do
  python bench.py --global-batch $B --steps 30 --warmup 5 --full --no-cpu-baseline --no-dense-compare > $OUT/bench_b$B.json 2> $OUT/bench_b$B.err; echo "b$B rc=$?"; tail -c 900 $OUT/bench_b$B.json
done
(cd /tmp && export TMPDIR=/tmp && rocprofv3 --kernel-trace --stats --output-format csv -d $ROOT/$OUT/prof_serial -- python3 $ROOT/bench.py --global-batch 512 --serial-towers --full --no-cpu-baseline --no-dense-compare --steps 20 --warmup 5 > $ROOT/$OUT/prof_serial.log 2>&1)
python scripts/kstats.py $OUT/prof_serial 27 0.05 > $OUT/kstats_serial.txt; tail -40 $OUT/kstats_serial.txt
