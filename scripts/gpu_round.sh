#!/bin/bash
# One GPU-box visit: parity tests, bench (--full), rocprof kernel stats.  Everything lands in $OUT (default build/gpu_round/).
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${OUT:-$R/build/gpu_round}
cd "$R"; mkdir -p "$OUT"
export PYTHONDONTWRITEBYTECODE=1
echo "== nproc $(nproc) ; $(rocm-smi --showproductname 2>/dev/null | grep -m1 -i 'card series' )" > "$OUT"/info.txt
( timeout ${T_TESTS:-900} python -m pytest tests -m gpu -q --maxfail=30 -p no:cacheprovider ${PYTEST_ARGS:-} > "$OUT"/pytest.log 2>&1; echo "pytest exit $?" >> "$OUT"/pytest.log )
tail -n 40 "$OUT"/pytest.log
if [ -z "$SKIP_BENCH" ]; then
  ( timeout ${T_BENCH:-600} python bench.py --full --steps ${STEPS:-3} --warmup 1 > "$OUT"/bench.json 2> "$OUT"/bench.err; echo "bench exit $?" >> "$OUT"/bench.err )
  cat "$OUT"/bench.json; tail -n 5 "$OUT"/bench.err
fi
if [ -z "$SKIP_PROF" ]; then
  ( cd /tmp && export TMPDIR=/tmp && timeout ${T_PROF:-600} rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o bench -- python "$R/bench.py" --full --steps 2 --warmup 1 --no-cpu-baseline > "$OUT/bench_prof.json" 2> "$OUT/bench_prof.err"; echo "prof exit $?" >> "$OUT/bench_prof.err" )
  find "$OUT"/prof -name "*kernel_stats*" | head -3
  f=$(find "$OUT"/prof -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && head -n 30 "$f"
  if [ -n "$DO_PMC" ]; then
    for c in FETCH_SIZE WRITE_SIZE; do
      ( cd /tmp && export TMPDIR=/tmp && timeout 300 rocprofv3 --pmc $c --kernel-trace -d "$OUT/pmc_$c" -o pmc -- python "$R/scripts/gauss_only.py" > "$OUT/pmc_$c.log" 2>&1; echo "pmc $c exit $?" >> "$OUT/pmc_$c.log" )
      tail -n 2 "$OUT/pmc_$c.log"
    done
  fi
  # keep the merge small: drop the raw per-dispatch trace
  find "$OUT"/prof -name "*kernel_trace.csv" -size +20M -delete
fi
