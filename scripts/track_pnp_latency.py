#!/usr/bin/env python3
"""Latency of Tracking::TrackWithPnP after the match, two ways, on one GPU (the
TrackWithPnP section):

  composed   match_fetch (2 copies, 2 synchronisations) + the pair gather of tracking.cpp:342-400 in
             vectorised numpy + pnp_ransac (1 upload, 2 kernels, 1 copy back, 1 synchronisation)
  one-call   track_pnp_async (3 kernels) + track_pnp_fetch (1 copy back, 1 synchronisation)

Both start from the same completed device-side match (match_device_async on resident descriptors)
of a synth.make_track_scene scene; they are alternated call by call inside one process after a
warm-up, and the medians over --calls calls each are reported with their quartiles.  Needs a GPU
(there is no fallback).  Writes one JSON file.

  python scripts/track_pnp_latency.py --out profiles/r08/track_pnp_latency.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visionx-slam_amd", "python"))


def gather(m, s, order, sorted_ids):
    """tracking.cpp:342-400 vectorised (every landmark of the scene is in the map and good)"""
    d = m["distance"]
    mn = min(np.float32(100.0), d.min()) if len(d) else np.float32(100.0)
    thr = max(2 * mn, np.float32(30.0))
    g = m[d <= thr]
    q, t = g["query_idx"], g["train_idx"]
    fl = s["flags"][q]
    ok = ((fl & 1) == 1) & ((fl & 2) == 0)
    ids = s["lm_id"][q]
    pos = np.searchsorted(sorted_ids, ids)
    pos[pos >= len(sorted_ids)] = 0
    ok &= sorted_ids[pos] == ids
    p = s["lm_pos"][order[pos]]
    ok &= ~np.isnan(p).any(1) & ~(np.abs(p) > 1000).any(1)
    duv = s["kf_uv"][q] - s["curr_xy"][t].astype(np.float64)
    parallax = np.sqrt((duv * duv).sum(1)).sum() / max(len(g), 1)
    return p[ok].astype(np.float32), s["curr_xy"][t[ok]], parallax


def run(ctx, vxslam, synth, torch, n_feat, calls, warmup):
    s = synth.make_track_scene(1000 + n_feat, n_feat, wrong_frac=0.3)
    dm = vxslam.DMap(ctx)
    dm.add_landmarks(s["lm_id"], s["lm_pos"])
    dm.add_keyframe(7, s["pose"], s["intr"], True, s["kf_uv"], s["lm_id"], s["flags"])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    dq, dt, dxy, dn = up(s["desc_kf"]), up(s["desc_curr"]), up(s["curr_xy"]), up(np.array([n_feat], np.int32))
    torch.cuda.synchronize()
    ctx.match_device_async((dq.data_ptr(), dn.data_ptr(), n_feat), (dt.data_ptr(), dn.data_ptr(), n_feat))
    ctx.synchronize()
    order = np.argsort(s["lm_id"])
    sorted_ids = s["lm_id"][order]
    opts = vxslam.track_options()

    def composed():
        m = ctx.match_fetch()
        obj, img, par = gather(m, s, order, sorted_ids)
        r, mask = ctx.pnp_ransac(obj, img, s["intr"], vxslam.pnp_options(len(obj)))
        return r, mask, par

    def one_call():
        ctx.track_pnp_async(dm, 7, (dxy.data_ptr(), 8, dn.data_ptr()), s["intr"], opts)
        return ctx.track_pnp_fetch()

    ra, ma, pa = composed()
    rb, _, mb = one_call()
    same = bool(ra.tobytes() == rb["pnp"].tobytes() and np.array_equal(ma, mb) and
                abs(pa - rb["parallax"]) <= 1e-12 * max(pa, 1.0))
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
    dm.close()
    q = lambda x: [round(float(v) * 1e3, 4) for v in np.percentile(x, [25, 50, 75])]
    qa, qb = q(ta), q(tb)
    return {"features": n_feat, "matches": int(rb["n_matches"]), "pairs": int(rb["n_pairs"]),
            "inliers": int(rb["pnp"]["n_inliers"]), "results_equal": same, "calls": calls, "warmup": warmup,
            "composed_ms_q25_q50_q75": qa, "one_call_ms_q25_q50_q75": qb,
            "ratio_composed_over_one_call": round(qa[1] / qb[1], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "track_pnp_latency.json"))
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 300])
    a = ap.parse_args()
    import torch

    import vxslam
    from vxslam import synth

    ctx = vxslam.Context(0)
    out = {
        "what": "host wall time from a completed device-side match to the pose in host memory, per call",
        "device": torch.cuda.get_device_name(0),
        # counted from the code paths, not measured
        "per_call": {"composed": {"kernel_launches": 2, "synchronisations": 3, "device_to_host_copies": 3,
                                  "host_to_device_copies": 1},
                     "one_call": {"kernel_launches": 3, "synchronisations": 1, "device_to_host_copies": 1,
                                  "host_to_device_copies": 0}},
        "sizes": [run(ctx, vxslam, synth, torch, n, a.calls, a.warmup) for n in a.sizes],
    }
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
