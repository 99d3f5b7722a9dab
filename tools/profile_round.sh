#!/bin/bash
# The round's measurement artefacts (run from the repo root on a machine with the GPU; copy the
# results into profiles/ under the round's tag).  OUT is the output folder (default bench_out):
#   1. the bench line of bench.py --full (with its live PMC passes and the CPU baseline)
#        -> $OUT/${TAG}_bench.json, PMC CSVs under $OUT/${TAG}_pmc/
#   2. rocprofv3 --kernel-trace --stats of the same workload with one frame in flight (the
#      kernels alone: what the roofline prices) -> $OUT/${TAG}_alone_kernel_stats.csv
#   3. the same with the default frames in flight -> $OUT/${TAG}_kernel_stats.csv
#   4. tools/roofline_check.py: the line's frac recomputed from 1 + 2
TAG=${TAG:-r04}
R=$PWD
OUT=${OUT:-bench_out}
set -o pipefail
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 500 python -u bench.py --full --pmc-dir $R/$OUT/${TAG}_pmc > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err \
  || { echo "bench failed"; tail $OUT/${TAG}_bench.err; exit 1; }
python3 tools/line_summary.py $OUT/${TAG}_bench.json bench
cd /tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $R/$OUT/${TAG}_alone -o run --output-format csv -- \
  python3 $R/bench.py --full --no-cpu --no-pmc --frames-in-flight 1 > $R/$OUT/${TAG}_alone.log 2>&1 || { echo "kernel trace (alone) failed"; exit 1; }
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $R/$OUT/${TAG}_prof -o run --output-format csv -- \
  python3 $R/bench.py --full --no-cpu --no-pmc > $R/$OUT/${TAG}_prof.log 2>&1 || { echo "kernel trace failed"; exit 1; }
cd $R
cp $OUT/${TAG}_alone/run_kernel_stats.csv $OUT/${TAG}_alone_kernel_stats.csv
cp $OUT/${TAG}_prof/run_kernel_stats.csv $OUT/${TAG}_kernel_stats.csv
python3 tools/roofline_check.py $OUT/${TAG}_bench.json $OUT/${TAG}_alone_kernel_stats.csv
