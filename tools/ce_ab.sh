#!/bin/bash
# config2 bench lines under runtime copy-engine settings
OUT=$(mktemp -d)
for E in "X=0" "GPU_FORCE_BLIT_COPY_SIZE=0" "GPU_BLIT_ENGINE_TYPE=2" "GPU_BLIT_ENGINE_TYPE=1"; do
  env $E timeout -k 10 120 python3 bench.py --full --no-cpu-baseline --no-north-star --no-config3 --no-check > $OUT/ce.json 2> $OUT/ce.err || { echo "$E failed"; tail -3 $OUT/ce.err; exit 1; }
  python3 -c "import json; d=json.load(open('$OUT/ce.json')); print('$E', d['value'], d['ms_per_step'], d.get('render_call_ms'))"
done
