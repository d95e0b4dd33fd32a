#!/bin/bash
# same-box, same-session A/B of the order-1 mean fields against a built checkout of the parent commit (whose MEAN forms
# of resident_band have no order to read): tools/mean_ab.sh <parent checkout> [rounds]     alternates parent / this
parent=$1; rounds=${2:-3}; here=$(cd "$(dirname "$0")/.." && pwd)
for i in $(seq $rounds); do
  for tree in "$parent" "$here"; do
    if [ "$tree" = "$here" ]; then echo "== this round $i"; else echo "== parent round $i"; fi
    timeout -k 10 200 python3 "$here/tools/mean_order1.py" "$tree" || exit 1
  done
done
