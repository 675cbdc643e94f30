#!/bin/bash
# rocprofv3 kernel stats, then counters in runs of their own, for the workspace network integrator against the LDS kernel on the
# S = 1 000 synthetic network (tools/gpu_bench_network_ws.py s1000).  Usage: bash tools/profile_network_ws.sh [TAG]  (from the repo root;
# output under build/profile/TAG, which git ignores)
set -u
TAG=${1:-network_ws}
REPO=$PWD
OUT=$REPO/build/profile/$TAG
mkdir -p $OUT
CMD="python3 $REPO/tools/gpu_bench_network_ws.py s1000"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/stats -- $CMD > $OUT/stats.log 2>&1 || { echo "rocprof stats failed"; tail -5 $OUT/stats.log; exit 1; }
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch -- $CMD > $OUT/pmc_fetch.log 2>&1 || { echo "pmc fetch failed"; tail -5 $OUT/pmc_fetch.log; exit 1; }
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write -- $CMD > $OUT/pmc_write.log 2>&1 || { echo "pmc write failed"; tail -5 $OUT/pmc_write.log; exit 1; }
timeout -k 10 300 rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_VMEM SQ_WAVE_CYCLES SQ_BUSY_CYCLES --output-format csv -d $OUT/pmc_sq -- $CMD > $OUT/pmc_sq.log 2>&1 || { echo "pmc sq failed"; tail -5 $OUT/pmc_sq.log; exit 1; }
timeout -k 10 300 rocprofv3 --pmc SQ_INSTS_VALU_FMA_F64 SQ_INSTS_VALU_ADD_F64 SQ_INSTS_VALU_MUL_F64 SQ_INSTS_VALU_TRANS_F64 --output-format csv -d $OUT/pmc_f64 -- $CMD > $OUT/pmc_f64.log 2>&1 || { echo "pmc f64 failed"; tail -3 $OUT/pmc_f64.log; }
python3 tools/summarize_prof.py $OUT | grep -E "net_solve|==" | tee $OUT/summary.txt
