#!/bin/bash
# bench.py under several settings of one environment variable, alternated on ONE box.
# usage: scripts/env_sweep.sh VAR "v1 v2 v3" [reps] [extra bench flags]  -> $OUT/env_sweep.txt (OUT defaults to bench_out)
VAR=$1; VALS=$2; REPS=${3:-2}; shift 3 || shift $#
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
: > "$OUT/env_sweep.txt"
for rep in $(seq $REPS); do
  for val in $VALS; do
    env "$VAR=$val" python3 bench.py --full --no-cpu-baseline --steps 20 "$@" 2>> "$OUT/env_sweep.err" | python3 -c "
import json,sys
d=json.loads(sys.stdin.read())
print('$VAR=$val', 'Msamples_s', d['value'], 'ms_per_step', d['ms_per_step'], 'single_view_ms', d['single_view_ms'])" >> "$OUT/env_sweep.txt"
  done
done
cat "$OUT/env_sweep.txt"
