#!/bin/bash
# Kernel-level picture of config 5 (ViT-H/14, fp8_mfma) at per-GPU batch 128: rocprofv3 kernel stats, towers on one stream.
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
cd $ROOT
OUT=gpurun_out/${1:-h14_fp8_prof}
mkdir -p $OUT
for P in fp8_mfma bf16; do
(cd /tmp && export TMPDIR=/tmp && rocprofv3 --kernel-trace --stats --output-format csv -d $ROOT/$OUT/prof_$P -- python3 $ROOT/bench.py --model ViT-H-14 --global-batch 128 --precision $P --serial-towers --full --no-cpu-baseline --no-dense-compare --steps 6 --warmup 2 > $ROOT/$OUT/prof_$P.log 2>&1)
python scripts/kstats.py $OUT/prof_$P 9 0.5 > $OUT/kstats_$P.txt; tail -45 $OUT/kstats_$P.txt
done
