#!/bin/bash
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
OUT=${PROF_OUT:-prof_out/tr}
mkdir -p $OUT
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT -o run --output-format csv -- python3 bench.py ${BENCH_ARGS:---full --steps 3 --warmup 1 --no-cpu-baseline} > $OUT/log 2>&1 || { echo "rc=$?"; tail -5 $OUT/log; exit 1; }
tail -1 $OUT/log
