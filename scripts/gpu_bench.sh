#!/bin/bash
# One GPU session for the committed measurements of a round (TAG):
#   1. two separate rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE) -> per-kernel HBM bytes
#      (scripts/pmc_summary.py, MI355X_MICROARCH.md corrections) -> profiles/pmc_traffic.json
#   2. bench.py --full (N=1, config C3, with CPU baseline) -> the JSON line, traffic included
#   3. rocprofv3 --kernel-trace --stats of the same bench command -> per-kernel durations
# Every GPU step has its own time limit; the script stops at the first failure.
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p $OUT profiles
TAG=${TAG:-r01}
P="--steps 20 --warmup 3 --no-cpu-baseline --no-profile"
timeout -k 10 600 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch_${TAG} -o run -- python3 bench.py $P > $OUT/pmc_fetch_${TAG}.log 2>&1 || { echo "pmc fetch failed"; tail -30 $OUT/pmc_fetch_${TAG}.log; exit 1; }
timeout -k 10 600 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write_${TAG} -o run -- python3 bench.py $P > $OUT/pmc_write_${TAG}.log 2>&1 || { echo "pmc write failed"; tail -30 $OUT/pmc_write_${TAG}.log; exit 1; }
python3 scripts/pmc_summary.py "$(find $OUT/pmc_fetch_${TAG} -name '*counter_collection.csv' | head -1)" \
    "$(find $OUT/pmc_write_${TAG} -name '*counter_collection.csv' | head -1)" $OUT/pmc_traffic_${TAG}.json \
    > $OUT/pmc_traffic_${TAG}.txt || exit 1
cp $OUT/pmc_traffic_${TAG}.json profiles/pmc_traffic.json
rm -rf $OUT/pmc_fetch_${TAG} $OUT/pmc_write_${TAG}  # (raw counter CSVs: tens of MB)
cat $OUT/pmc_traffic_${TAG}.txt
timeout -k 10 600 python bench.py --full > $OUT/bench_${TAG}.json 2> $OUT/bench_${TAG}.err || { echo "bench failed"; tail -20 $OUT/bench_${TAG}.err; exit 1; }
cat $OUT/bench_${TAG}.json
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${TAG} -o run -- python3 bench.py --full --no-cpu-baseline > $OUT/prof_${TAG}.log 2>&1 || { echo "rocprof failed"; tail -30 $OUT/prof_${TAG}.log; exit 1; }
rm -f $OUT/prof_${TAG}/*kernel_trace.csv  # (one row per launch: tens of MB; the stats stay)
find $OUT/prof_${TAG} -name "*kernel_stats.csv"
