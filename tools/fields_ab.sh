#!/bin/bash
# same-box, same-session A/B of the unarmed resident path against a built checkout of the parent commit:
# tools/fields_ab.sh <parent checkout> [rounds]     alternates parent / this: unarmed resident runs at 128^2 and 1024^2
parent=$1; rounds=${2:-3}; here=$(cd "$(dirname "$0")/.." && pwd)
for i in $(seq $rounds); do
  for tree in "$parent" "$here"; do
    if [ "$tree" = "$here" ]; then echo "== this round $i"; else echo "== parent round $i"; fi
    timeout -k 10 200 python3 "$here/tools/resident_unarmed.py" "$tree" || exit 1
  done
done
