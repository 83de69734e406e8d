#!/usr/bin/env python3
"""Per-call time of InitWithFirstFrame's gates on the device (vx_init_gate_*, csrc/init_gate.hip) against
the sequential host loop of tests/cpp/frontend_driver.cpp.

For each shape: host clock around host_async + fetch and around async + fetch on device-resident inputs
(both end in the fetch's synchronisation), medians with quartiles over --reps calls after warm-up; then,
in a loop of its own, the two kernels' own durations from the library's stage events and k_init_sums'
bytes read over that time.  The yardstick and the adapter-side call time come from `frontend_driver gate`
on the same image and positions.  Prints one JSON line per shape."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visionx-slam_amd", "python"))

import torch  # noqa: E402  (before the library: tests/conftest.py)

import vxslam  # noqa: E402
from vxslam import synth  # noqa: E402

DRIVER = os.path.join(ROOT, "visionx-slam_amd", "build", "frontend_driver")


def quartiles(v):
    q = np.percentile(np.asarray(v) * 1e6, [25, 50, 75])
    return [round(float(x), 2) for x in q]


def timed(fn, reps, warmup=20):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return quartiles(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--shapes", default="640x480x2000,1280x960x4000")
    args = ap.parse_args()
    ctx = vxslam.Context(0)
    for shape in args.shapes.split(","):
        w, h, n = (int(x) for x in shape.split("x"))
        img = synth.make_frames(3, 1, h, w)[0]
        rng = np.random.default_rng(1)
        xy = np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n)], -1).astype(np.float32)
        d_img = torch.from_numpy(img).cuda()
        d_xy = torch.from_numpy(xy).cuda()
        d_n = torch.tensor([n], dtype=torch.int32).cuda()
        torch.cuda.synchronize()
        feats = (d_xy.data_ptr(), 8, d_n.data_ptr())

        def host_call():
            ctx.init_gate_host(img, xy)

        def dev_call():
            ctx.init_gate_async(d_img.data_ptr(), w, h, 3, 3 * w, feats, cap_feat=n)
            ctx.init_gate_fetch()

        rec = {"shape": shape, "reps": args.reps, "host_variant_us": timed(host_call, args.reps),
               "device_variant_us": timed(dev_call, args.reps)}
        ref = ctx.init_gate_host(img, xy)
        dev_call()
        assert ctx.init_gate_fetch().tobytes() == ref.tobytes()
        ctx.prof_enable(True, ["init_sums", "init_gate"])
        try:
            ctx.prof_read()
            for _ in range(args.reps):
                dev_call()
            p = ctx.prof_read()
        finally:
            ctx.prof_enable(False)
        sums_us = p["init_sums"][0] / p["init_sums"][1] * 1e3
        rec["kernel_us"] = {"init_sums": round(sums_us, 2), "init_gate": round(p["init_gate"][0] / p["init_gate"][1] * 1e3, 2)}
        rec["init_sums_bytes"] = w * h * 3
        rec["init_sums_GBps"] = round(w * h * 3 / (sums_us * 1e-6) / 1e9, 1)
        with tempfile.TemporaryDirectory() as tmp:
            np.array([w, h, 3, 3 * w], np.int32).tofile(os.path.join(tmp, "gate_meta.bin"))
            img.tofile(os.path.join(tmp, "img.bin"))
            xy.tofile(os.path.join(tmp, "xy.bin"))
            out = subprocess.run([DRIVER, "gate", tmp, str(args.reps)], capture_output=True, text=True, check=True, timeout=300)
            t = out.stdout.splitlines()[1].split()
            rec["driver_call_us"] = [float(x) for x in t[2:5]]
            rec["host_loop_us"] = [float(x) for x in t[6:9]]
        print(json.dumps(rec), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
