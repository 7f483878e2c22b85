#!/bin/bash
# Round-3 profiles (run on the GPU box through gpurun): the default bench, a kernel trace of the same command, the two
# HBM-traffic PMC passes, the SQ instruction counters of one search batch, the issue-rate microbenchmark, the per-row
# measurements.  Summaries: python scripts/rocpd_summary.py gpurun_out/prof_r03 profiles r03
ROOT=${GRAFT_REPO_ROOT:-/root/repo}
OUT=$ROOT/gpurun_out/prof_r03
rm -rf $OUT; mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
python3 $ROOT/bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err
python3 $ROOT/bench.py --full --steps 20 --warmup 5 --no-cpu > $OUT/bench_driver_command.json 2> /dev/null
timeout 600 rocprofv3 --kernel-trace --stats -d $OUT/trace -o bench -- python3 $ROOT/bench.py --full --no-cpu > $OUT/bench_under_rocprof.log 2>&1
timeout 900 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $OUT/pmc_fetch -o fetch -- python3 $ROOT/bench.py --full --steps 2 --warmup 1 --no-cpu > $OUT/pmc_fetch.log 2>&1
timeout 900 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $OUT/pmc_write -o write -- python3 $ROOT/bench.py --full --steps 2 --warmup 1 --no-cpu > $OUT/pmc_write.log 2>&1
timeout 600 rocprofv3 --kernel-trace --stats -d $OUT/trace_rows -o rows -- python3 $ROOT/scripts/bench_rows.py > $OUT/rows.json 2> $OUT/rows.log
python3 $ROOT/scripts/timeline2.py $OUT/trace/*/*bench_results.db > $OUT/engine_timeline.txt 2>&1 || python3 $ROOT/scripts/timeline2.py $(find $OUT/trace -name "*.db" | head -1) > $OUT/engine_timeline.txt 2>&1
bash $ROOT/scripts/pmc_astar_sq.sh 96000 > $OUT/sq_counters.txt 2>&1
hipcc --offload-arch=gfx950 -O3 -Wno-unused-value $ROOT/scripts/ubench_valu.hip -o /tmp/ubench_valu && timeout 120 /tmp/ubench_valu > $OUT/ubench_valu.txt 2>&1
cd $ROOT && python3 scripts/rocpd_summary.py gpurun_out/prof_r03 gpurun_out/prof_r03/summaries r03 > $OUT/summary_stdout.txt 2>&1
# the trace databases are large: keep the summaries only
find $OUT -name "*.db" -size +20M -delete
tail -c 600 $OUT/bench_default.json | head -c 300; echo; head -12 $OUT/summaries/r03_kernel_stats_trace.txt
