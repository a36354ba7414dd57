#!/bin/bash
# One GPU-box session: parity tests, then (unless the tests hung) the full bench.  Logs go to $OUT (default: logs/).
set -u
OUT=${OUT:-logs}
mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 ${TEST_TIMEOUT:-700} python -m pytest tests -m gpu -q -x --durations=15 > "$OUT/gpu_tests.log" 2>&1
rc=$?
echo "pytest rc=$rc" | tee -a "$OUT/gpu_tests.log"
tail -n 25 "$OUT/gpu_tests.log"
if [ $rc -eq 124 ] || [ $rc -eq 137 ]; then echo "tests hung: not starting the bench"; exit $rc; fi
timeout -k 10 ${BENCH_TIMEOUT:-400} python bench.py --steps ${STEPS:-20} --warmup 3 --full > "$OUT/bench.log" 2> "$OUT/bench.err"
brc=$?
echo "bench rc=$brc"; tail -n 5 "$OUT/bench.err"; cat "$OUT/bench.log"
exit $(( rc != 0 ? rc : brc ))
