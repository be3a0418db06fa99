#!/bin/bash
# quick GPU check: staged-encoder parity tests, then the default bench line
set -o pipefail
O=${BIC_OUT_DIR:-bench_out}; mkdir -p $O  # where the logs go
timeout -k 10 300 python -u -m pytest tests/test_gpu_fused.py tests/test_gpu_fullsize.py -x -q --timeout 200 --timeout-method thread -k "${QK:-fused or c3 or c4}" > $O/quick_test.log 2>&1 || { tail -30 $O/quick_test.log; exit 1; }
tail -2 $O/quick_test.log
timeout -k 10 200 python bench.py --full --no-cpu "$@" > $O/quick_bench.log 2>&1 || { tail -20 $O/quick_bench.log; exit 1; }
python3 -c "
import json
l=[x for x in open('$O/quick_bench.log') if x.startswith('{')][-1]; j=json.loads(l)
print(j['ms_per_step'], j.get('bit_exact_check'), j['roofline']['avg_launch_us'], j['roofline']['frac'], {k:round(v['avg_us'],1) for k,v in j['kernels'].items()})"
