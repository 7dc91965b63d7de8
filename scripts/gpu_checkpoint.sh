# checkpoint run on the GPU box (OUT=<dir> bash scripts/gpu_checkpoint.sh TAG; OUT defaults to results/): full GPU test-suite, smoke, bench --full (+cpu baseline), rocprofv3 kernel trace, PMC passes. args: tag
cd "$(dirname "$0")/.."; TAG=${1:-e}; R=$PWD; OUT=$(realpath -m "${OUT:-results}"); mkdir -p $OUT
timeout 1500 python -m pytest tests -m gpu -q --tb=short -p no:cacheprovider > $OUT/pytest_$TAG.log 2>&1; echo "pytest rc=$?" >> $OUT/pytest_$TAG.log
tail -5 $OUT/pytest_$TAG.log
timeout 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/smoke_$TAG.log 2>&1; tail -2 $OUT/smoke_$TAG.log
timeout 900 python bench.py --full > $OUT/bench_$TAG.log 2>&1; echo "rc=$?" >> $OUT/bench_$TAG.log; tail -3 $OUT/bench_$TAG.log
cd /tmp && export TMPDIR=/tmp
B="python $R/bench.py --steps 4 --warmup 1 --no-cpu-baseline"
timeout 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_r1$TAG -o r1$TAG -- $B > $OUT/prof_$TAG.log 2>&1
timeout 600 rocprofv3 --kernel-trace --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_WAVES -d $OUT/pmc1_$TAG -o p1 --output-format csv -- $B > $OUT/pmc1_$TAG.log 2>&1
timeout 600 rocprofv3 --kernel-trace --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_WAIT_INST_LDS SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VALU -d $OUT/pmc2_$TAG -o p2 --output-format csv -- $B > $OUT/pmc2_$TAG.log 2>&1
timeout 600 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $OUT/pmc3_$TAG -o p3 --output-format csv -- $B > $OUT/pmc3_$TAG.log 2>&1
timeout 600 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $OUT/pmc4_$TAG -o p4 --output-format csv -- $B > $OUT/pmc4_$TAG.log 2>&1
cd $R; ls $OUT/prof_r1$TAG $OUT/pmc1_$TAG | head
