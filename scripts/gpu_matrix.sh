#!/bin/bash
# bench.py over --streams 1/2/3, each with and without the timed-region HIP-event bracket
cd "$GRAFT_REPO_ROOT"
export OUT=${OUT:-bench_out}
mkdir -p $OUT
TAG=${TAG:-m}
for s in 3 2 1; do
  timeout -k 10 300 python bench.py --streams $s --full --no-cpu-baseline > $OUT/mx_${TAG}_s${s}.json 2>/dev/null || exit 1
  timeout -k 10 300 python bench.py --streams $s --full --no-cpu-baseline --no-profile > $OUT/mx_${TAG}_s${s}_np.json 2>/dev/null || exit 1
done
python3 - <<'PY'
import json, glob, os
tag = os.environ.get("TAG", "m")
for f in sorted(glob.glob(f"{os.environ['OUT']}/mx_{tag}_*.json")):
    d = json.load(open(f))
    r = d.get("roofline") or {}
    print(f"{os.path.basename(f):24s} value {d['value']:.4f} latency {d.get('latency_ms_per_frame')} dom {r.get('kernel')} {r.get('avg_launch_us')}")
PY
