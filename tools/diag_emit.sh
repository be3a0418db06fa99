set -o pipefail
O=${BIC_OUT_DIR:-bench_out}; mkdir -p $O  # where the logs go
cd $GRAFT_REPO_ROOT
for d in 0 1 2 4 6 7; do
  BIC_LIB_PATH=binary-image-compression_amd/lib/libbic_stamps.so BIC_EMIT_DBG=$d timeout -k 10 120 python3 bench.py --full --no-cpu --no-check --steps 10 > $O/dbg_$d.log 2>&1 || { echo "dbg $d failed"; tail -5 $O/dbg_$d.log; exit 1; }
  python3 -c "
import json
l=[x for x in open('$O/dbg_$d.log') if x.startswith('{')][-1]; j=json.loads(l)
print('dbg $d', j['ms_per_step'], {k:round(v['avg_us'],1) for k,v in j['kernels'].items()})"
done
timeout -k 10 120 python3 tools/emit_stamps.py > $O/emit_stamps.log 2>&1 && cat $O/emit_stamps.log
export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/aux -o run --output-format csv -- python3 tools/time_aux.py --reps 3 > $O/aux.log 2>&1 || { echo aux failed; tail -5 $O/aux.log; exit 1; }
grep '^{' $O/aux.log
