#!/bin/bash
# round 6: the whole GPU suite, smoke and the default bench line with this
# round's changes so far
set -o pipefail
export TMPDIR=/tmp
R=$(pwd)
O=$R/gpurun_out/r06o
mkdir -p $O
step() { echo "== $1 $(date +%T)"; }
step pytest
timeout -k 10 1000 python -u -m pytest tests -m gpu -x -v --timeout 400 --timeout-method thread > $O/pytest_gpu.log 2>&1 || { tail -30 $O/pytest_gpu.log; exit 1; }
tail -1 $O/pytest_gpu.log
step smoke
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1 || { tail -5 $O/smoke.log; exit 1; }
tail -1 $O/smoke.log
step bench
timeout -k 10 600 python bench.py --full > $O/bench_c3.log 2>&1 || { tail -5 $O/bench_c3.log; exit 1; }
tail -1 $O/bench_c3.log | cut -c1-400
step done
