#!/bin/bash
# rocprofv3 kernel trace + stats, then HBM byte counters in separate passes.
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
OUT=${PROF_OUT:-gpurun_out/prof}
mkdir -p $OUT
ARGS=${BENCH_ARGS:---full --steps 3 --warmup 1 --no-cpu-baseline}
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/trace -o run --output-format csv -- \
  python3 bench.py $ARGS > $OUT/trace.log 2>&1 || { echo "trace rc=$?"; exit 1; }
echo trace ok
timeout -k 10 600 rocprofv3 --pmc FETCH_SIZE -d $OUT/pmc_fetch -o run --output-format csv -- \
  python3 bench.py $ARGS > $OUT/pmc_fetch.log 2>&1 || { echo "fetch rc=$?"; exit 1; }
echo fetch ok
timeout -k 10 600 rocprofv3 --pmc WRITE_SIZE -d $OUT/pmc_write -o run --output-format csv -- \
  python3 bench.py $ARGS > $OUT/pmc_write.log 2>&1 || { echo "write rc=$?"; exit 1; }
echo write ok
find $OUT -name "*.csv" | head -20
