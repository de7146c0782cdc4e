#!/bin/bash
# End-of-round evidence on the GPU box (one gpurun call, ~15 min): bench lines (default, per-GPU batch 2048 / 1024 / 512, one-rank
# RCCL rehearsal, ViT-H/14 in bf16 / fp8 / fp8_mfma), rocprofv3 kernel stats of the serial-towers bench, a kernel trace of the
# default two-stream bench (what overlaps what), PMC passes (MFMA utilisation, FETCH, WRITE), per-shape GEMM / epilogue / attention
# micro-benchmarks.  (scripts/collect_configs.sh: kernel-stat tables of BASELINE configs 3-5 and of the ColXLIP step -- a call of its own,
# one gpurun call is capped at 20 minutes.)
# ROUND=r04 names the outputs; scripts/save_evidence.py copies them into profiles/.
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
cd $ROOT
export ROUND=${ROUND:-r04}
F=gpurun_out/final_$ROUND
mkdir -p $F
python bench.py --full > $F/bench_default.json 2> $F/bench_default.err; echo "bench rc=$?"; tail -c 2600 $F/bench_default.json
for B in 2048 1024 512; do
  python bench.py --global-batch $B --steps 30 --warmup 5 --full --no-cpu-baseline --no-dense-compare > $F/bench_b$B.json 2> $F/bench_b$B.err; echo "b$B rc=$?"
done
python bench.py --force-dist --steps 6 --warmup 2 --full --no-cpu-baseline --no-dense-compare > $F/bench_forcedist.json 2> $F/bench_forcedist.err; echo "force-dist rc=$?"
for P in bf16 fp8 fp8_mfma; do
  python bench.py --model ViT-H-14 --global-batch 128 --precision $P --steps 6 --warmup 2 --full --no-cpu-baseline --no-dense-compare > $F/bench_h14_${P}_b128.json 2> $F/bench_h14_$P.err; echo "h14 $P rc=$?"
done
(cd /tmp && export TMPDIR=/tmp && rocprofv3 --kernel-trace --stats --output-format csv -d $ROOT/$F/prof -- python3 $ROOT/bench.py --serial-towers --full --no-cpu-baseline --no-dense-compare --steps 8 --warmup 3 > $ROOT/$F/prof.log 2>&1)
python scripts/kstats.py $F/prof 12 > $F/kstats.txt; tail -28 $F/kstats.txt
(cd /tmp && export TMPDIR=/tmp && rocprofv3 --kernel-trace --output-format csv -d $ROOT/$F/trace2 -- python3 $ROOT/bench.py --full --no-cpu-baseline --no-dense-compare --steps 5 --warmup 3 > $ROOT/$F/trace2.log 2>&1)
python scripts/timeline_gaps.py $F/trace2 20 > $F/timeline_two_streams.txt 2>&1; head -20 $F/timeline_two_streams.txt
(cd /tmp && export TMPDIR=/tmp && rocprofv3 --kernel-trace --stats --output-format csv -d $ROOT/$F/prof512 -- python3 $ROOT/bench.py --global-batch 512 --serial-towers --full --no-cpu-baseline --no-dense-compare --steps 20 --warmup 5 > $ROOT/$F/prof512.log 2>&1)
python scripts/kstats.py $F/prof512 27 0.05 > $F/kstats_b512.txt
bash scripts/collect_pmc.sh > $F/pmc.log 2>&1; head -12 gpurun_out/pmc_${ROUND}_traffic_entry.json
python scripts/bench_gemm.py > $F/gemm_vs_hipblaslt.txt 2>&1; tail -4 $F/gemm_vs_hipblaslt.txt
python scripts/bench_epi.py > $F/epilogue_variants.txt 2>&1
python scripts/bench_attn.py > $F/attention.txt 2>&1; tail -2 $F/attention.txt
python scripts/bench_colclip.py 256 512 > $F/colclip.txt 2>&1; tail -4 $F/colclip.txt
for S in h14 long b16; do python scripts/bench_attn.py 256 $S > $F/attention_$S.txt 2>&1; done; mv $F/attention_long.txt $F/attention_l14.txt
python bench.py --model ViT-B-16 --global-batch 512 --steps 10 --warmup 3 --full --no-cpu-baseline --no-dense-compare > $F/bench_b16_b512.json 2> $F/bench_b16.err; echo "b16 rc=$?"
ls $F
