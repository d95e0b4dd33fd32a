#!/bin/bash
# A/B of the command line against the parent's host program, both on this tree's liblbm_hip.so:
#   tools/cli_ab.sh <parent commit | the parent's built d2q9-bgk> [runs]
# Every case of tests/cli_case.py (malformed values, valid values, the 21 pairs of the option table) goes through both
# programs: exit status and stderr must agree.  The first line of a message, "Error at line N of file F:", names the source
# line and is compared as a constant.  LBM_ANIMATION with LBM_STEADY or LBM_PROBES may differ: the parent refuses them only
# after it has created the context, which on a box without a device fails first.
# With "runs" (needs a device): 128x128 runs of every mode for 300 and for 0 steps, LBM_GPUS=2 and LBM_OUTPUT=none: every
# file written and stdout without its "Elapsed" lines must be byte-identical.  Stops at the first run that does not end well.
here=$(cd "$(dirname "$0")/.." && pwd); lib=$here/lbm-asynchronous_amd; work=$(mktemp -d)
trap 'rm -rf "$work"' EXIT
unset LBM_PRECISION LBM_STEADY LBM_PROBES LBM_ANIMATION LBM_MEAN LBM_STATES LBM_FORCES LBM_TILE LBM_MEAN_ORDER \
      LBM_PRESSURE_BIN LBM_GPUS LBM_MATH LBM_OUTPUT
if [ -x "$1" ]; then parent=$(realpath "$1"); else
  mkdir -p "$work/src/lbm-asynchronous_amd/host" "$work/src/include"
  for f in lbm-asynchronous_amd/host/d2q9-bgk.c lbm-asynchronous_amd/host/lbm_io.c lbm-asynchronous_amd/host/lbm_io.h include/lbm_hip.h; do
    git -C "$here" show "$1:$f" > "$work/src/$f" || exit 1
  done
  parent=$work/d2q9-bgk.parent
  gcc -std=c99 -O3 -fopenmp -D_POSIX_C_SOURCE=200809L -D_DEFAULT_SOURCE "$work"/src/lbm-asynchronous_amd/host/*.c -o "$parent" \
      -L"$lib" -llbm_hip -lm -Wl,-rpath,"$lib" -Wl,-rpath,/opt/rocm/lib || exit 1
fi
inputs=$here/tests/golden/inputs; bad=0

# run <label> <dir> <program> NAME=VALUE...: status, stdout and stderr into <dir>.status / .out / .err
run() {
  local label=$1 dir=$2 prog=$3; shift 3
  mkdir -p "$dir"
  (cd "$dir" && timeout -k 10 120 env "$@" "$prog" ../input.params "$inputs/obstacles_128x128.dat" > "../$label.out" 2> "../$label.err")
  local status=$?; echo $status > "$dir/../$label.status"
  case $status in 124|134|137|139) echo "STOP: $label, '$*': exit status $status"; cat "$dir/../$label.err"; exit 1;; esac
  sed -E -i 's/^Error at line [0-9]+ of file .*:$/Error at line N of file F:/' "$dir/../$label.err"
}

echo "== options: $(python3 "$here/tests/cli_case.py" | wc -l) cases, parent = $1"
sed '3s/.*/10/' "$inputs/input_128x128.params" > "$work/input.params"
n=0
while IFS= read -r line; do
  n=$((n + 1)); IFS=$'\t' read -r -a vars <<< "$line"
  for side in parent this; do
    rm -rf "$work/$side"
    if [ $side = parent ]; then run $side "$work/$side" "$parent" "${vars[@]}"; else run $side "$work/$side" "$lib/d2q9-bgk" "${vars[@]}"; fi
  done
  shown=$(echo "$line" | cut -c1-70 | tr '\t' ' ')
  if cmp -s "$work/parent.status" "$work/this.status" && cmp -s "$work/parent.err" "$work/this.err" && diff -r "$work/parent" "$work/this" > /dev/null; then
    echo "same      status $(cat "$work/this.status")  $shown"
  elif [[ "$line" == *LBM_ANIMATION=100 ]] && [[ "$line" == LBM_STEADY* || "$line" == LBM_PROBES* ]] && grep -q "no HIP device" "$work/parent.err"; then
    echo "intended  status $(cat "$work/parent.status") / $(cat "$work/this.status")  $shown: parent '$(tail -1 "$work/parent.err" | cut -c1-40)...', this '$(tail -1 "$work/this.err")'"
  else
    echo "DIFFERENT status $(cat "$work/parent.status") / $(cat "$work/this.status")  $shown"; diff "$work/parent.err" "$work/this.err"; bad=1
  fi
done < <(python3 "$here/tests/cli_case.py")
[ "$2" = runs ] || { echo "== options: $n cases, $([ $bad = 0 ] && echo all as expected || echo DIFFERENCES)"; exit $bad; }

echo "== runs: 128x128, every mode for 300 and for 0 steps"
for steps in 300 0; do
  sed "3s/.*/$steps/" "$inputs/input_128x128.params" > "$work/input.params"
  for vars in "" LBM_ANIMATION=100 LBM_STATES=100:3,2,40,30 "LBM_PROBES=64,64;10,126:7" "LBM_MEAN=10:50 LBM_MEAN_ORDER=2" LBM_FORCES=50 \
              LBM_STEADY=1e-6:64 LBM_PRECISION=double LBM_GPUS=2 LBM_OUTPUT=none; do
    if [ $steps = 0 ] && [[ "$vars" == LBM_GPUS* || "$vars" == LBM_OUTPUT* ]]; then continue; fi
    for side in parent this; do
      rm -rf "$work/$side"
      if [ $side = parent ]; then run $side "$work/$side" "$parent" $vars; else run $side "$work/$side" "$lib/d2q9-bgk" $vars; fi
      if [ "$(cat "$work/$side.status")" != 0 ]; then
        echo "STOP: $side, $steps steps, '$vars': exit status $(cat "$work/$side.status")"; cat "$work/$side.err"; exit 1
      fi
      grep -v "^Elapsed " "$work/$side.out" > "$work/$side.report"
    done
    files=$(cd "$work/this" && find . -type f | wc -l)
    if cmp -s "$work/parent.report" "$work/this.report" && cmp -s "$work/parent.err" "$work/this.err" && diff -r "$work/parent" "$work/this" > /dev/null; then
      echo "same      $steps steps  ${vars:-plain}: $files files, $(wc -l < "$work/this.report") lines of stdout"
    else
      echo "DIFFERENT $steps steps  ${vars:-plain}"; diff "$work/parent.report" "$work/this.report"; diff -rq "$work/parent" "$work/this"; bad=1
    fi
  done
done
echo "== $([ $bad = 0 ] && echo all as expected || echo DIFFERENCES)"
exit $bad
