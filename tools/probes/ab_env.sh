#!/bin/bash
# dev: one library, several environments (e.g. RC_ENTRY_CULL), interleaved on one GPU box:
#   tools/probes/ab_env.sh "RC_ENTRY_CULL=1 RC_ENTRY_CULL=0" [perf_probe args...]
ES=$1; shift
for round in 1 2; do
  for e in $ES; do
    echo "== $e (round $round)"; env $e RC_PROBE_REPS=${RC_PROBE_REPS:-8} python3 tools/perf_probe.py "$@" 2>&1 | grep "Mrays"
  done
done
