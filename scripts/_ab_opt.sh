#!/bin/bash
# same-node A/B of one library option on the headline step: bash scripts/_ab_opt.sh BCOS_OPT_H2_TILE=2 [pairs]
OPT=$1; PAIRS=${2:-3}
run() { env $1 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline 2>/dev/null | python -c "import json,sys; r=json.loads(sys.stdin.read()); print('$2', r['value'], r['step_times']['sub_batch_stream_steps']['median'], r['roofline']['kernel_ms_per_step'], r['roofline']['by_bound']['mfma']['ms_per_step'], r['roofline']['by_bound']['hbm']['ms_per_step'], r['roofline']['by_bound']['hbm']['frac'])"; }
for i in $(seq 1 $PAIRS); do
  run "BCOS_NOOP=1" default
  run "$OPT" "$OPT"
done
