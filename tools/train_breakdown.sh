#!/bin/bash
# tools/train_breakdown.sh [bench args]   e.g. --train-dtype f16x2   (per-launch lines on stderr: redirect 2> to keep them)
python bench.py --full --mode train --steps 10 --warmup 3 --per-layer "$@" | python -c "
import json,sys
d=json.loads(sys.stdin.read()); print(d['ms_per_step'], d['value'], d['dtype'])
for k,v in sorted(d['kernels'].items(), key=lambda kv:-kv[1]['ms_per_step']): print(k, v)"
