#!/bin/bash
# bench.py's two orders of the set-up: a = prepare_run first, then the warm-up steps; b = the warm-up steps first (the default)
B="--steps 20 --warmup 5 --no-cpu-baseline --no-extras --profile-steps 0"
py="import json,sys; d=json.loads(sys.stdin.read().strip().split(chr(10))[-1]); print(round(d['ms_per_step']*1e3,2), round(d['config']['device_ms_per_step']*1e3,2))"
for i in 1 2 3 4; do
  a=$(BFMMM_BENCH_PREPARE_FIRST=1 python bench.py $B 2>/dev/null | python -c "$py")
  b=$(python bench.py $B 2>/dev/null | python -c "$py")
  echo "prepare-then-warmup: $a | warmup-then-prepare: $b   [us/step wall, device]"
done
