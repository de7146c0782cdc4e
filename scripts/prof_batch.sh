#!/bin/bash
# kernel-time breakdown of the bench step at a smaller per-GPU batch: bash scripts/prof_batch.sh 512   (results in $OUT, default bench_out/)
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${OUT:-bench_out}
mkdir -p $ROOT/$OUT
B=$1
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $ROOT/$OUT/prof_b$B -- python3 $ROOT/bench.py --global-batch $B --serial-towers --full --no-cpu-baseline --no-dense-compare --steps 10 --warmup 3 > $ROOT/$OUT/prof_b$B.log 2>&1
cd $ROOT
python scripts/kstats.py $OUT/prof_b$B 14 0.05 > $OUT/kstats_b$B.txt
tail -c 400 $OUT/prof_b$B.log | head -c 400; echo
awk '$(NF-3)+0 > 0.05' $OUT/kstats_b$B.txt | head -30; tail -1 $OUT/kstats_b$B.txt
