#!/bin/bash
# Kernel-level evidence for the OTHER BASELINE configs at their stated per-GPU batch (3: ViT-B/16 512; 4: ViT-L/14-336 1024,
# grad-checkpointed; 5: ViT-H/14 2048, fp8 MFMA, grad-checkpointed) and for the fork's own ColXLIP step (ViT-B-16-colxlip, 512): a
# bench line each + rocprofv3 kernel stats with the towers on one stream.  scripts/save_evidence.py copies the results to profiles/.
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
cd $ROOT
export ROUND=${ROUND:-r04}
F=gpurun_out/final_$ROUND
mkdir -p $F
prof_cfg() {   # tag, steps profiled, bench flags...
  local tag=$1 n=$2; shift 2
  python bench.py "$@" --steps $n --warmup 1 --full --no-cpu-baseline --no-dense-compare > $F/bench_$tag.json 2> $F/bench_$tag.err; echo "$tag rc=$?"; tail -c 600 $F/bench_$tag.json
  (cd /tmp && export TMPDIR=/tmp && rocprofv3 --kernel-trace --stats --output-format csv -d $ROOT/$F/prof_$tag -- python3 $ROOT/bench.py "$@" --serial-towers --steps $n --warmup 1 --full --no-cpu-baseline --no-dense-compare > $ROOT/$F/prof_$tag.log 2>&1)
  python scripts/kstats.py $F/prof_$tag $((n + 2)) 0.05 > $F/kstats_$tag.txt; head -12 $F/kstats_$tag.txt
}
prof_cfg b16_b512 10 --model ViT-B-16 --global-batch 512
prof_cfg l14_336_b1024_ckpt 3 --model ViT-L-14-336 --global-batch 1024 --grad-checkpointing
prof_cfg h14_b2048_fp8_mfma_ckpt 2 --model ViT-H-14 --global-batch 2048 --precision fp8_mfma --grad-checkpointing
prof_cfg colxlip_b16_b512 10 --model ViT-B-16-colxlip --global-batch 512
ls $F | head -50
