#!/bin/bash
# GPU box: the --full bench line, then the plain command under rocprofv3 (kernel trace + stats).
# Results under $OUT (profile_out/ by default); the summaries worth keeping are copied into profiles/ by hand.
#   bash tools/profile_bench.sh [WORKLOAD]     (C3 by default; C5, C2, "C4 --genes 1")
set -e
W=${1:-C3}
TAG=$(echo $W | tr -d " -" | tr 'A-Z' 'a-z')
OUT=${OUT:-profile_out}
mkdir -p $OUT
python bench.py --workload $W --full > $OUT/bench_default_$TAG.json 2> $OUT/bench_default_$TAG.err || { tail -5 $OUT/bench_default_$TAG.err; exit 1; }
tail -1 $OUT/bench_default_$TAG.json | cut -c1-600
export TMPDIR=/tmp
# rocprofv3 itself has crashed now and then on this workload (SIGSEGV inside its interception of a HIP call,
# about one profiled run out of ten, never without the profiler): such a run is reported, not repeated
rm -rf $OUT/prof_bench
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_bench -o bench -- python3 bench.py --workload $W --steps 5 --warmup 1 > $OUT/bench_under_rocprof_$TAG.json 2> $OUT/rocprof.err || { tail -3 $OUT/rocprof.err; exit 1; }
find $OUT/prof_bench -name '*kernel_stats.csv' | while read f; do cp "$f" $OUT/bench_kernel_stats_$TAG.csv; done
find $OUT/prof_bench -name '*kernel_trace.csv' -delete
head -12 $OUT/bench_kernel_stats_$TAG.csv
