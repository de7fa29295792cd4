#!/bin/bash
# GPU box helper: parity tests, bench line (--full), rocprofv3 kernel stats of the same command; results in $OUT (default out/)
set -o pipefail
OUT=${OUT:-out}
mkdir -p $OUT
export TMPDIR=/tmp
if [ "${SKIP_TESTS:-0}" != "1" ]; then
  python -m pytest tests -x -q -m gpu 2>&1 | tail -15 > $OUT/parity.log; rc=$?
  cat $OUT/parity.log
  [ $rc -ne 0 ] && exit $rc
fi
python bench.py --full --steps ${STEPS:-30} --warmup 3 ${BENCH_ARGS:-} > $OUT/bench.json 2> $OUT/bench.err; rc=$?
tail -5 $OUT/bench.err; cat $OUT/bench.json
[ $rc -ne 0 ] && exit $rc
if [ "${SKIP_PROF:-0}" != "1" ]; then
  rm -rf $OUT/prof && mkdir -p $OUT/prof
  # (--no-feed: the host-fed measurement behind the timed region launches the same kernels on 32 MiB buffers; they would
  # be averaged into demod_tiles' row of the stats file)
  rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o stats -- python3 bench.py --full --steps 20 --warmup 5 --no-feed > $OUT/prof_bench.json 2> $OUT/prof.err; rc=$?
  tail -3 $OUT/prof.err
  f=$(find $OUT/prof -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && head -8 "$f"
fi
exit $rc
