#!/bin/bash
# usage (GPU box): tools/profile_round3.sh NAME ["extra bench.py args"]
# The default bench.py command under rocprofv3: kernel trace + stats, then the PMC passes (each in its own run, never
# together with a trace), then the FETCH_SIZE / WRITE_SIZE calibrations.  tools/summarize_round3.py turns the CSVs into
# profiles/<NAME>.md, profiles/<NAME>_kernel_stats.csv and the PMC json bench.py reads for `traffic`.
R=${GRAFT_REPO_ROOT:-/root/repo}; NAME=$1; EXTRA=$2
OUT=$R/gpurun_out/$NAME; mkdir -p $OUT; cd /tmp; export TMPDIR=/tmp
B="python $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-extras $EXTRA"
python $R/bench.py --full $EXTRA > $OUT/bench.json 2> $OUT/bench.err
rocprofv3 --kernel-trace --stats -f csv -d $OUT/stats -- $B > $OUT/stats.log 2>&1
rocprofv3 --pmc FETCH_SIZE -f csv -d $OUT/fetch -- $B > $OUT/fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE -f csv -d $OUT/write -- $B > $OUT/write.log 2>&1
rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_INSTS_LDS SQ_INSTS_SMEM SQ_INSTS_BRANCH -f csv -d $OUT/sq1 -- $B > $OUT/sq1.log 2>&1
rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS -f csv -d $OUT/sq2 -- $B > $OUT/sq2.log 2>&1
rocprofv3 --pmc SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT GRBM_GUI_ACTIVE -f csv -d $OUT/lds -- $B > $OUT/lds.log 2>&1
rocprofv3 --pmc FETCH_SIZE -f csv -d $OUT/calib -- python $R/tools/calib_fetch.py > $OUT/calib.log 2>&1
rocprofv3 --pmc WRITE_SIZE -f csv -d $OUT/calibw -- python $R/tools/calib_fetch.py > $OUT/calibw.log 2>&1
python $R/tools/summarize_round3.py $NAME $OUT "$EXTRA" > $OUT/summary.md 2> $OUT/summary.err
cp $OUT/stats/*/*_kernel_stats.csv $OUT/kernel_stats.csv 2>/dev/null
tail -40 $OUT/summary.md; tail -3 $OUT/summary.err
