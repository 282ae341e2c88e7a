#!/bin/bash
# Round-end pass 2: the full bench command (bench.py --full) under rocprofv3 --kernel-trace --stats (+ the timed
# window's per-launch averages; outputs under $OUT, default out/ in the repository), then the PMC traffic passes over
# the timed window.  Usage: gpu_final2.sh TAG
set -o pipefail
T=${1:-r6f}
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}
cd $R && mkdir -p $OUT
export TMPDIR=/tmp PYTHONUNBUFFERED=1
cd /tmp
timeout -k 10 700 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${T}_prof -o run -- \
  python3 $R/bench.py --full > $OUT/${T}_bench_under_rocprof.json 2> $OUT/${T}_bench_under_rocprof.err || exit $?
cd $R && python3 tools/rocprof_window.py $OUT/${T}_prof $OUT/${T}_bench_under_rocprof.json \
  > $OUT/${T}_window_kernel_stats.csv || exit $?
cat $OUT/${T}_window_kernel_stats.csv
bash tools/pmc_traffic.sh ${T} || exit $?
head -c 1500 gpurun_out/${T}_pmc_traffic.json
