set -o pipefail
O=${BIC_OUT_DIR:-bench_out}; mkdir -p $O  # where the logs go
export TMPDIR=/tmp
timeout -k 10 300 python -u bench.py --full --steps 40 --warmup 6 --inflight 2 --no-cpu > $O/if2b.log 2>&1 || exit $?
timeout -k 10 300 python -u bench.py --full --steps 40 --warmup 6 --no-cpu > $O/if1b.log 2>&1 || exit $?
