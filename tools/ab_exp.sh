#!/bin/bash
# A/B of alternative library builds on the C2 expansion leg (64K-event pushes: normal-mode placement,
# poll_device and the compact leg): tools/ab_exp.sh ab/lib_x.so [...]   (logs in $OUT, default bench_out)
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p $OUT
run() {
  timeout -k 10 300 python -u bench.py --full --steps 1 --warmup 1 --no-calibrate --no-cpu-baseline --no-ingest --no-latency ${AB_ARGS:-} > $OUT/ab.log 2> $OUT/ab.err || { tail -20 $OUT/ab.err; exit 1; }
  echo "$1: $(python3 -c "import json; d=json.loads(open('$OUT/ab.log').read().strip().splitlines()[-1]); x=d['expansion']; print(round(x['push_ms_per_step'],3), round(x['poll_ms_per_step'],3), round(x['compact']['ms_per_step'],3))")"
}
run default
for lib in "$@"; do SIDDHI_HIP_LIB=$PWD/$lib run $lib; done
run default
