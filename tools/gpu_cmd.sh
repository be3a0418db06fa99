set -o pipefail
O=${BIC_OUT_DIR:-bench_out}; mkdir -p $O  # where the logs go
export TMPDIR=/tmp
timeout -k 10 900 python -u -m pytest -x -q --timeout 300 --timeout-method thread -m gpu tests/ > $O/t_all.log 2>&1; rc=$?
[ $rc -eq 0 ] || [ $rc -eq 1 ] || exit $rc
: > $O/ab8.log
for a in "--eg-source-mode 1" "--eg-source-mode 2" "--eg-source-mode 1 --one-stream"; do
  timeout -k 10 240 python -u bench.py --full --steps 20 --warmup 3 --no-cpu $a > $O/b8.json 2>> $O/ab8.err || exit $?
  python3 -c "
import json
j=json.loads([l for l in open('$O/b8.json') if l.startswith('{')][-1])
print('$a |', j['ms_per_step'], j.get('bit_exact_check'), {k: round(v['avg_us'],1) for k, v in j['kernels'].items()}, j['predictor_pass']['in_step']['frac'] if j.get('predictor_pass') else None)" >> $O/ab8.log
done
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof8 -o run --output-format csv -- python3 bench.py --full --steps 10 --no-cpu --no-check > $O/prof8.log 2>&1
