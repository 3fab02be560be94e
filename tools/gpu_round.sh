#!/bin/bash
# One GPU session: smoke, GPU parity tests, bench, rocprof kernel trace.
# Every GPU step is time-limited and chained with &&.
set -o pipefail
cd "${GRAFT_REPO_ROOT:-/root/repo}"
mkdir -p gpurun_out
export TMPDIR=/tmp
STEP=${1:-all}
if [[ $STEP == all || $STEP == smoke ]]; then
  timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > gpurun_out/smoke.log 2>&1 || { echo "smoke failed rc=$?"; tail -30 gpurun_out/smoke.log; exit 1; }
  tail -2 gpurun_out/smoke.log
fi
if [[ $STEP == all || $STEP == test ]]; then
  timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > gpurun_out/pytest_gpu.log 2>&1 || { echo "pytest gpu failed rc=$?"; tail -40 gpurun_out/pytest_gpu.log; exit 1; }
  tail -3 gpurun_out/pytest_gpu.log
fi
# the bench and profile steps write under $OUT_DIR (default build/evidence)
O=${OUT_DIR:-build/evidence}
mkdir -p "$O"
if [[ $STEP == all || $STEP == bench ]]; then
  timeout -k 10 600 python bench.py --steps 10 --warmup 3 --full > $O/bench.log 2>&1 || { echo "bench failed rc=$?"; tail -30 $O/bench.log; exit 1; }
  tail -1 $O/bench.log
fi
if [[ $STEP == all || $STEP == prof ]]; then
  timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $O/prof -o run --output-format csv -- python3 bench.py --steps 10 --warmup 3 --full --no-cpu-baseline > $O/prof.log 2>&1 || { echo "rocprof failed rc=$?"; tail -30 $O/prof.log; exit 1; }
  find $O/prof -name "*kernel_stats.csv" | head -3
  for f in $(find $O/prof -name "*kernel_stats.csv"); do head -5 "$f"; done
fi
