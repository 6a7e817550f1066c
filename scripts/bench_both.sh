#!/bin/bash
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
O=${BENCH_OUT:-bench_out}
mkdir -p $O
timeout -k 10 600 python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --precision 64 > $O/bench64.log 2>&1 || { echo "bench64 rc=$?"; tail -5 $O/bench64.log; exit 1; }
tail -1 $O/bench64.log
timeout -k 10 600 python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --precision 32 > $O/bench32.log 2>&1 || { echo "bench32 rc=$?"; tail -5 $O/bench32.log; exit 1; }
tail -1 $O/bench32.log
