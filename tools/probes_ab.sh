#!/bin/bash
# same-box, same-session A/B of the unarmed paths against a built checkout of the parent commit:
# tools/probes_ab.sh <parent checkout> [rounds]     alternates parent / this: bench.py at 8192^2, unarmed resident runs
parent=$1; rounds=${2:-3}; here=$(cd "$(dirname "$0")/.." && pwd)
for i in $(seq $rounds); do
  for tree in "$parent" "$here"; do
    if [ "$tree" = "$here" ]; then echo "== this round $i"; else echo "== parent round $i"; fi
    (cd "$tree" && timeout -k 10 200 python3 bench.py --gpus 1 --steps 20 --warmup 5 2>/dev/null) | python3 -c "
import json,sys
l=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('bench', l.get('grid', ''), l['value'], l.get('unit', ''), l['ms_per_step'], 'ms/step')" || exit 1
    timeout -k 10 200 python3 "$here/tools/resident_unarmed.py" "$tree" || exit 1
  done
done
