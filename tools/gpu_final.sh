#!/bin/bash
# Round-end pass 1: the whole GPU suite, smoke(), the full bench line (outputs under $OUT, default out/ in the
# repository).  Usage: gpu_final.sh TAG
set -o pipefail
T=${1:-r6f}
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}
cd $R && mkdir -p $OUT
export PYTHONUNBUFFERED=1 TMPDIR=/tmp
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread -p no:cacheprovider \
  > $OUT/${T}_gpu_tests.log 2>&1 || { tail -40 $OUT/${T}_gpu_tests.log; exit 1; }
tail -2 $OUT/${T}_gpu_tests.log
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke(); print('smoke OK')" > $OUT/${T}_smoke.log 2>&1 || { tail -20 $OUT/${T}_smoke.log; exit 1; }
tail -1 $OUT/${T}_smoke.log
timeout -k 10 600 python -u bench.py --full > $OUT/${T}_bench.json 2> $OUT/${T}_bench.err || { tail -30 $OUT/${T}_bench.err; exit 1; }
tail -c 3000 $OUT/${T}_bench.json
