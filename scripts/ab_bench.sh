#!/bin/bash
# same-box A/B of library builds / switches, alternating: each argument is "tag[:lib.so][:ENV=VAL...]" (default: prev = build/libcmpc_prev.so
# against the in-tree build).  Prints ms_per_step of bench.py per variant and round.  Every bench run has its own time limit, and the first
# run that does not exit 0 ends the script with status 1: nothing more is started on the GPU behind a failed run.
VARS=("$@"); [ ${#VARS[@]} -eq 0 ] && VARS=("prev:build/libcmpc_prev.so" "cur")
OUT=$(mktemp)
for i in $(seq 1 ${ROUNDS:-3}); do
  for v in "${VARS[@]}"; do
    IFS=: read -r tag lib envs <<< "$v"
    ( [ -n "$lib" ] && export CMPC_LIB_PATH=$PWD/$lib; for e in ${envs//,/ }; do export $e; done
      timeout -k 10 300 python bench.py --steps ${STEPS:-30} --warmup 3 --no-cpu-baseline --no-alt-dtype --no-kernel-timing --no-forward-only > $OUT 2>/dev/null )
    rc=$?
    if [ $rc -ne 0 ]; then echo "$tag: bench.py exited with $rc; stopping"; rm -f $OUT; exit 1; fi
    echo "$tag $(tail -1 $OUT | python -c "import sys,json; print(json.loads(sys.stdin.read())['ms_per_step'])")"
  done
done
rm -f $OUT
