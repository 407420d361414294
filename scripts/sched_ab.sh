#!/bin/bash
# A/B of the step schedule on one box: prefetch of the next batch's backbone (behind the levels' forward) on and off, at the runtime's
# default hardware-queue count (raising GPU_MAX_HW_QUEUES is not done on shared machines).
cd $GRAFT_REPO_ROOT
run() { # label, env..., -- bench args
  label=$1; shift
  out=$(env "$@" timeout -k 10 200 python bench.py --steps 20 --warmup 3 --no-cpu-baseline --no-config4 --no-config5 --no-alt-dtype --no-kernel-timing --no-forward-only $EXTRA 2>/dev/null | python -c "import json,sys; d=json.loads(sys.stdin.read()); print('%.3f ms  %.1f img/s' % (d['ms_per_step'], d['value']))")
  echo "$label: $out"
}
for rep in 1 2; do
EXTRA="" run "base  lanes3 q4" CMPC_STREAMS=3
EXTRA="--prefetch"            run "pref  lanes3 q4" CMPC_STREAMS=3
done
