#!/bin/bash
# development: bench.py --full with each fused-kernel mode given on the command line, per-size pair rates side by side
out=${AB_OUT:-build/ab}
mkdir -p "$out"
for m in "$@"; do
  VKFFT_MI355X_FUSED_MODE=$m timeout 250 python bench.py --full 2>/dev/null | tail -1 > "$out/bench_m$m.json"
  python -c "
import json
d=json.load(open('$out/bench_m$m.json'))
print('mode $m', d['value'], d['ms_per_step'])
ps=d.get('per_size')
print(ps if not isinstance(ps,dict) else {k:(round(v['alg_GBps']) if isinstance(v,dict) else v) for k,v in ps.items()})
"
done
