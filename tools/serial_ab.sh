#!/bin/bash
# stage times with every kernel alone on the GPU (ORBX_SERIAL=1, eager): variants given as env assignments, e.g. tools/serial_ab.sh "" ORBX_FAST_V4=1 ORBX_FAST_V3=1
log=$(mktemp -d)
for v in "$@"; do
  env ORBX_SERIAL=1 $v python bench.py --full --steps 10 --warmup 3 --cpu-sample 0 --launch eager > $log/serial.log 2>$log/serial.err
  tail -1 $log/serial.log | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('[$v]', 'fps', round(d['value']), {k: round(v,3) for k,v in d['stage_ms_per_step'].items() if k in ('fast','pyramid_fast_span','total')})" || tail -3 $log/serial.err
done
