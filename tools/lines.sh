#!/bin/bash
# The bench lines of a round: the default command with every leg (--full), then C3 / C4 / C2x (and C5
# with `c5`) with their CPU baselines, each under its own time limit; logs in $OUT/line_<w>.log
# (OUT defaults to bench_out; copy to profiles/<round>_runs).
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 400 python -u bench.py --full > $OUT/line_c2.log 2> $OUT/line_c2.err || { tail -20 $OUT/line_c2.err; exit 1; }
tail -1 $OUT/line_c2.log | cut -c1-300
for w in c3 c4 c2x; do
  timeout -k 10 400 python -u bench.py --full --workload $w > $OUT/line_$w.log 2> $OUT/line_$w.err || { tail -20 $OUT/line_$w.err; exit 1; }
  tail -1 $OUT/line_$w.log | cut -c1-300
done
if [ "$1" = c5 ]; then
  timeout -k 10 900 python -u bench.py --full --workload c5 > $OUT/line_c5.log 2> $OUT/line_c5.err || { tail -20 $OUT/line_c5.err; exit 1; }
  tail -1 $OUT/line_c5.log | cut -c1-300
fi
