#!/bin/bash
# One GPU job: what to run is selected by the arguments (tests | probe | bench | prof ...); outputs go to $OUT (default job_out/ in the repository root).
set -u
cd "$(dirname "$0")/.."
OUT=${OUT:-job_out}
mkdir -p "$OUT"
for what in "$@"; do
  case "$what" in
    tests) timeout 2400 python -m pytest tests -m gpu -x -q 2>&1 | tail -40 > "$OUT/tests.log"; tail -5 "$OUT/tests.log" ;;
    tests_all) timeout 2400 python -m pytest tests -m gpu -q 2>&1 | tail -60 > "$OUT/tests.log"; tail -15 "$OUT/tests.log" ;;
    probe) for cfg in 2 4; do CFG=$cfg VIL_LIB=tools/_exp/libvilsolve_stamps.so timeout 300 python tools/probe_step.py > "$OUT/probe_c$cfg.log" 2>&1; cat "$OUT/probe_c$cfg.log"; done ;;
    probe_plain) for cfg in 2 3 4; do CFG=$cfg timeout 300 python tools/probe_step.py 2>&1 | head -1 | tee "$OUT/probe_plain_c$cfg.log"; done ;;
    bench) timeout 900 python bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err"; cat "$OUT/bench.json" ;;
    *) echo "unknown job $what" ;;
  esac
done
