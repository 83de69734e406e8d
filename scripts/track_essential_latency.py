#!/usr/bin/env python3
"""Latency of Tracking::TrackLastFrame after the match, two ways, on one GPU:

  composed   match_fetch (2 copies, 2 synchronisations) + the distance filter, the cv::Point2f pairs
             and ComputeParallax of tracking.cpp:291-325 in vectorised numpy + essential_ransac
             (1 upload, the em_* kernels, 1 copy back, 1 synchronisation) + PoseFromRt and T_cl * T_lw
             on the host
  one-call   track_essential_async (k_track_epairs, the em_* kernels, k_track_epose) +
             track_essential_fetch (1 copy back, 1 synchronisation)

Both start from the same completed device-side match (match_device_async on resident descriptors)
of a synth.make_last_frame_scene scene; they are alternated call by call inside one process after a
warm-up, and the medians over --calls calls each are reported with their quartiles.  Needs a GPU
(there is no fallback).  Writes one JSON file.

  python scripts/track_essential_latency.py --out profiles/r11/track_essential_latency.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visionx-slam_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def gather(m, s):
    """tracking.cpp:291-304, :509-514, :548-560 vectorised (every index of the scene is in range)"""
    d = m["distance"]
    mn = min(np.float32(100.0), d.min()) if len(d) else np.float32(100.0)
    thr = max(2 * mn, np.float32(30.0))
    g = m[d <= thr]
    p1, p2 = s["last_xy"][g["query_idx"]], s["curr_xy"][g["train_idx"]]
    duv = p1.astype(np.float64) - p2.astype(np.float64)
    parallax = np.sqrt((duv * duv).sum(1)).sum() / max(len(g), 1)
    return p1, p2, parallax


def run(ctx, vxslam, synth, torch, n_feat, calls, warmup, max_iterations):
    from track_ess_ref import compose, pose_from_Rt

    s = synth.make_last_frame_scene(1000 + n_feat, n_feat, wrong_frac=0.3)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    dq, dt, dn = up(s["desc_last"]), up(s["desc_curr"]), up(np.array([n_feat], np.int32))
    dl, dc = up(s["last_xy"]), up(s["curr_xy"])
    torch.cuda.synchronize()
    ctx.match_device_async((dq.data_ptr(), dn.data_ptr(), n_feat), (dt.data_ptr(), dn.data_ptr(), n_feat))
    ctx.synchronize()
    opts = vxslam.track_essential_options(max_iterations=max_iterations)
    eo = np.array(opts["ess"], vxslam.EM_OPTIONS_DTYPE)

    def composed():
        m = ctx.match_fetch()
        p1, p2, par = gather(m, s)
        r, mask = ctx.essential_ransac(p1, p2, s["intr"], eo)
        pose = compose(pose_from_Rt(r["R"], r["t"]), s["pose_last"]) if r["ok"] else np.zeros(7)
        return r, mask, par, pose

    def one_call():
        ctx.track_essential_async((dl.data_ptr(), 8, dn.data_ptr()), (dc.data_ptr(), 8, dn.data_ptr()), s["intr"], opts,
                                  pose_last=s["pose_last"])
        return ctx.track_essential_fetch()

    ra, ma, pa, posea = composed()
    rb, _, mb = one_call()
    same = bool(ra.tobytes() == rb["ess"].tobytes() and np.array_equal(ma, mb) and
                abs(pa - rb["parallax"]) <= 1e-12 * max(pa, 1.0) and np.array_equal(posea, rb["pose"]))
    for _ in range(warmup):
        composed()
        one_call()
    ta, tb = [], []
    for _ in range(calls):  # alternated: both see the same drift of the shared host
        t0 = time.perf_counter()
        composed()
        t1 = time.perf_counter()
        one_call()
        t2 = time.perf_counter()
        ta.append(t1 - t0)
        tb.append(t2 - t1)
    q = lambda x: [round(float(v) * 1e3, 4) for v in np.percentile(x, [25, 50, 75])]
    qa, qb = q(ta), q(tb)
    return {"features": n_feat, "matches": int(rb["n_matches"]), "pairs": int(rb["n_pairs"]),
            "inliers": int(rb["ess"]["n_inliers"]), "hypotheses_run": int(rb["ess"]["hypotheses_run"]),
            "results_equal": same, "calls": calls, "warmup": warmup,
            "composed_ms_q25_q50_q75": qa, "one_call_ms_q25_q50_q75": qb,
            "ratio_composed_over_one_call": round(qa[1] / qb[1], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "track_essential_latency.json"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 300])
    ap.add_argument("--max-iterations", type=int, default=1000, help="findEssentialMat's maxIters (its default)")
    a = ap.parse_args()
    import torch

    import vxslam
    from vxslam import synth

    ctx = vxslam.Context(0)
    out = {
        "what": "host wall time from a completed device-side match to the composed pose in host memory, per call",
        "device": torch.cuda.get_device_name(0),
        "max_iterations": a.max_iterations,
        # counted from the code paths, not measured
        "per_call": {"composed": {"synchronisations": 3, "device_to_host_copies": 3, "host_to_device_copies": 1},
                     "one_call": {"synchronisations": 1, "device_to_host_copies": 1, "host_to_device_copies": 0}},
        "sizes": [run(ctx, vxslam, synth, torch, n, a.calls, a.warmup, a.max_iterations) for n in a.sizes],
    }
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
