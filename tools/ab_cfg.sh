#!/bin/bash
# A/B of another library / environment against the current build on the C5, C3, C4 bench lines: tools/ab_cfg.sh <lib-or-""> [ENV=VAL ...]
lib=$1; shift
log=$(mktemp -d)
for c in c5 c3 c4; do
  python bench.py --full --config $c --steps 20 --warmup 5 --cpu-sample 0 > $log/x_$c.log 2>$log/x_$c.err
  env ${lib:+ORB_LIB=$lib} "$@" python bench.py --full --config $c --steps 20 --warmup 5 --cpu-sample 0 > $log/y_$c.log 2>$log/y_$c.err
  python - <<PY
import json
for side in ("x", "y"):
    d = json.loads(open("$log/%s_$c.log" % side).read().strip().splitlines()[-1]); s = d["stage_ms_per_step"]
    print("$c", side, round(d["value"]), round(d["value_device_resident"]), round(s["orient_desc"], 4), round(s["blur"], 4), round(s["total"], 4))
PY
done
