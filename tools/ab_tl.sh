#!/bin/bash
# tools/ab_tl.sh "benchargs" FIRSTKERNEL NAME...: kernel timeline of one bench step per lib/var_NAME.so
set -o pipefail
O=${BIC_OUT_DIR:-bench_out}; mkdir -p $O  # where the logs go
export TMPDIR=/tmp
ARGS=$1; FK=$2; shift 2
for n in "$@"; do
  BIC_LIB_PATH=binary-image-compression_amd/lib/var_$n.so timeout -k 10 120 rocprofv3 --kernel-trace -d $O/abtl_$n -o run --output-format csv -- python3 bench.py --full --no-cpu --no-check --steps 10 $ARGS > $O/abtl_$n.log 2>&1 || { echo "$n failed"; tail -3 $O/abtl_$n.log; exit 1; }
  echo "== $n"; python3 tools/timeline.py $O/abtl_$n/run_kernel_trace.csv $FK
done
