#!/bin/bash
# The fork's own operating point: ViT-B-16-colxlip + ColClipLoss, 512 pairs on one GPU (reference src/colxlip.sh:38,52).  Bench line,
# the loss alone at N = 256 / 512, and rocprofv3 kernel stats of the whole step with the towers on one stream.
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
cd $ROOT
OUT=gpurun_out/${1:-colxlip_r4}
mkdir -p $OUT
python bench.py --model ViT-B-16-colxlip --global-batch 512 --steps 20 --warmup 5 --full --no-cpu-baseline --no-dense-compare > $OUT/bench_colxlip_b512.json 2> $OUT/bench_colxlip_b512.err; echo "rc=$?"; tail -c 1500 $OUT/bench_colxlip_b512.json; tail -3 $OUT/bench_colxlip_b512.err
python scripts/bench_colclip.py 256 512 2>&1 | grep -v amdgpu.ids | tee $OUT/colclip.txt
(cd /tmp && export TMPDIR=/tmp && rocprofv3 --kernel-trace --stats --output-format csv -d $ROOT/$OUT/prof_serial -- python3 $ROOT/bench.py --model ViT-B-16-colxlip --global-batch 512 --serial-towers --full --no-cpu-baseline --no-dense-compare --steps 10 --warmup 3 > $ROOT/$OUT/prof_serial.log 2>&1)
python scripts/kstats.py $OUT/prof_serial 15 0.05 > $OUT/kstats_serial.txt; tail -45 $OUT/kstats_serial.txt
