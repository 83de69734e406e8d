#!/bin/bash
# GPU parity tests, then a short bench with per-kernel stats.  Stops at the first failure.
cd "$GRAFT_REPO_ROOT"
export TMPDIR=/tmp
export OUT=${OUT:-bench_out}
mkdir -p $OUT
TAG=${TAG:-dev}
timeout -k 10 900 python -m pytest tests -m gpu -q -x -p no:cacheprovider > $OUT/tests_${TAG}.log 2>&1
rc=$?; tail -15 $OUT/tests_${TAG}.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python bench.py --full --no-cpu-baseline > $OUT/bench_${TAG}.json 2> $OUT/bench_${TAG}.err || { tail -20 $OUT/bench_${TAG}.err; exit 1; }
cat $OUT/bench_${TAG}.json; grep stage $OUT/bench_${TAG}.err
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${TAG} -o run -- python3 bench.py --steps 20 --warmup 3 --full --no-cpu-baseline > $OUT/prof_${TAG}.log 2>&1 || { tail -30 $OUT/prof_${TAG}.log; exit 1; }
python3 - <<'PY'
import csv, os, re
tag = os.environ.get("TAG", "dev")
rows = list(csv.DictReader(open(f"{os.environ['OUT']}/prof_{tag}/run_kernel_stats.csv")))
for r in rows:
    m = re.search(r"\b(k_[a-z0-9_]+)(?:<[^>(]*>)?\(", r["Name"])
    print(f"{(m.group(1) if m else r['Name'][:30]):22s} calls {r['Calls']:>5s} avg_us {float(r['AverageNs'])/1e3:9.2f} pct {float(r['Percentage']):6.2f}")
PY
