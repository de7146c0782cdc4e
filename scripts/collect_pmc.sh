#!/bin/bash
# PMC evidence for the shipping kernels (run on the GPU box from the repo root):
#   bash scripts/collect_pmc.sh [extra bench flags]
# Three separate rocprofv3 passes of the same one-step bench command (counters must not be combined with trace domains
# other than --kernel-trace; FETCH_SIZE and WRITE_SIZE do not fit one pass: MI355X_MICROARCH.md, rocprofv3 PMC slots):
#   sq     SQ_VALU_MFMA_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY GRBM_GUI_ACTIVE
#   fetch  FETCH_SIZE        write  WRITE_SIZE
# Output: gpurun_out/pmc_$ROUND/{sq,fetch,write}/... and the summaries gpurun_out/pmc_${ROUND}_{sq,fetch,write}.txt (ROUND defaults to r04)
set -u
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
R=${ROUND:-r04}
OUT=$ROOT/gpurun_out/pmc_$R
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
BENCH="python3 $ROOT/bench.py --serial-towers --steps 1 --warmup 1 --full --no-cpu-baseline --no-dense-compare $*"
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY GRBM_GUI_ACTIVE \
          --kernel-trace --output-format csv -d $OUT/sq -- $BENCH > $OUT/sq.log 2>&1
echo "sq pass rc=$?"
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/fetch -- $BENCH > $OUT/fetch.log 2>&1
echo "fetch pass rc=$?"
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/write -- $BENCH > $OUT/write.log 2>&1
echo "write pass rc=$?"
cd $ROOT
for p in sq fetch write; do python3 scripts/pmc_summary.py $OUT/$p > gpurun_out/pmc_${R}_$p.txt 2>&1; done
python3 scripts/pmc_traffic_entry.py $OUT > gpurun_out/pmc_${R}_traffic_entry.json
tail -n 5 $OUT/sq.log | cut -c1-3000
