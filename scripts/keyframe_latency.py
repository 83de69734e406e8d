#!/usr/bin/env python3
"""Latency of keyframe creation on the resident map (vx_dmap_create_keyframe*), on one GPU.

Map: C3 (50 + 2 keyframes / 20k landmarks, resident).  New frame: 2000 features, the match list to
the last keyframe, a 640x480 u16 depth image — `with_depth` (half of the features' depth pixels are
holes, so both branches are populated) and `no_depth` (Depth().empty(): triangulation only).  Warmed
and alternated in one process, medians and quartiles of:

  device    DMap.create_keyframe: positions, matches and depth already on the device
  host      DMap.create_keyframe_host: host arrays staged and uploaded in one copy
  sequence  what a caller does without the call: Context.depth_landmarks + Context.triangulate (host
            arrays up, host arrays back, one synchronisation each), then add_landmarks +
            add_observations + set_features + add_keyframe (the numpy glue between them included;
            `sequence_compute_calls` / `sequence_edit_calls` split it at the first edit call)

Every call inserts a keyframe, so each timed call gets a last keyframe of its own (a copy of the
pair's first frame, added untimed right before) in the same growing map; the three legs take turns.
Needs a GPU (there is no fallback).  Writes one JSON file.

  python scripts/keyframe_latency.py --out profiles/r10/keyframe_latency.json
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


def stats(ms):
    q = np.percentile(np.asarray(ms, np.float64), [25, 50, 75])
    return {"median_ms": float(q[1]), "q25_ms": float(q[0]), "q75_ms": float(q[2]), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "keyframe_latency.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--features", type=int, default=2000)
    a = ap.parse_args()
    import torch

    import vxslam
    from vxslam import synth

    import cull_ref
    import keyframe_ref as R

    def dev(x):
        b = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
        t = torch.from_numpy(np.concatenate([b, np.zeros(16, np.uint8)])).cuda()
        torch.cuda.synchronize()
        return t

    ctx = vxslam.Context(0)
    nk, nl, _ = synth.ba_config("C3")
    m = synth.make_cull_scene(0xC0 + nk, nk, nl, special=False)
    dm = vxslam.DMap(ctx)
    cull_ref.load(dm, m)
    next_kf, next_lm = int(m["kf_id"].max()) + 1, int(m["lm_id"].max()) + 1
    out = {"reps": a.reps, "map": {"keyframes": int(m["kf_alive"].sum()), "landmarks": nl,
                                   "observations": len(m["obs_kf_id"])}, "features": a.features, "cases": {}}
    for case in ("with_depth", "no_depth"):
        d = synth.make_keyframe_scene(0x4B46, a.features, with_depth=case == "with_depth")
        n, mt, depth = a.features, np.ascontiguousarray(d["matches"], vxslam.MATCH_DTYPE), d["depth"]
        link1 = np.where(d["has1"] > 0, 900000 + np.arange(n), 0).astype(np.uint64)
        keep = [dev(d["uv2"].astype(np.float32)), dev(np.array([n], np.int32)), dev(mt), dev(np.array([len(mt)], np.int32))]
        ddev = None
        if depth is not None:
            keep.append(dev(depth))
            ddev = (keep[-1].data_ptr(), vxslam.DEPTH_TYPES[depth.dtype], depth.shape[0], depth.shape[1], depth.strides[0])
        none = np.zeros(n, np.uint8)

        def fresh_last():
            nonlocal next_kf
            dm.add_keyframe(next_kf, d["pose1"], d["intr"], True, d["uv1"], link1, d["has1"])
            next_kf += 1
            return next_kf - 1

        def leg_device(last):
            return dm.create_keyframe(next_kf, d["pose2"], d["intr"], (keep[0].data_ptr(), 8, keep[1].data_ptr(), n),
                                      last_kf_id=last, matches=(keep[2].data_ptr(), keep[3].data_ptr(), len(mt)),
                                      depth=ddev, first_landmark_id=next_lm)["landmarks"]

        def leg_host(last):
            return dm.create_keyframe_host(next_kf, d["pose2"], d["intr"], d["uv2"], last_kf_id=last, matches=mt,
                                           depth=depth, first_landmark_id=next_lm)["landmarks"]

        def leg_sequence(last):
            ig, pg = ctx.depth_landmarks(d["uv2"], none, depth, d["intr"], d["pose2"])
            tg, tpg = ctx.triangulate(dict(d, has2=(ig >= 0).astype(np.uint8)))
            di, ti = np.nonzero(ig >= 0)[0], np.nonzero(tg >= 0)[0]
            recs = np.zeros(len(di) + len(ti), vxslam.KEYFRAME_LANDMARK_DTYPE)
            recs["lm_id"] = next_lm + np.arange(len(recs))
            recs["kind"][len(di):] = 1
            recs["feat_curr"] = np.concatenate([di, mt["train_idx"][ti]])
            recs["feat_last"] = np.concatenate([np.full(len(di), -1), mt["query_idx"][ti]])
            recs["pw"] = np.concatenate([pg.reshape(-1, 3), tpg.reshape(-1, 3)])
            t1 = time.perf_counter()
            R.apply_edits(dm, next_kf, d["pose2"], d["intr"], d["uv2"], last, recs)
            ctx.synchronize()
            split.append((1e3 * (t1 - t_leg[0]), 1e3 * (time.perf_counter() - t1)))
            return recs

        legs = {"device": leg_device, "host": leg_host, "sequence": leg_sequence}
        times = {k: [] for k in legs}
        split, t_leg = [], [0.0]  # sequence: (the two compute calls + glue, the four edit calls) per call
        made = {}
        for rep in range(-3, a.reps):  # (three warm-up rounds: code objects, pinned blocks, array growth)
            for name, leg in legs.items():
                last = fresh_last()
                ctx.synchronize()
                t0 = t_leg[0] = time.perf_counter()
                recs = leg(last)
                ctx.synchronize()
                dt = 1e3 * (time.perf_counter() - t0)
                next_kf += 1
                next_lm += len(recs)
                if rep >= 0:
                    times[name].append(dt)
                made[name] = (int((recs["kind"] == 0).sum()), int((recs["kind"] == 1).sum()))
        assert made["device"] == made["host"] == made["sequence"], made
        cfg = {"matches": len(mt), "n_depth": made["device"][0], "n_triangulated": made["device"][1]}
        cfg.update({k: stats(v) for k, v in times.items()})
        cfg["sequence_compute_calls"] = stats([x[0] for x in split[-a.reps:]])
        cfg["sequence_edit_calls"] = stats([x[1] for x in split[-a.reps:]])
        out["cases"][case] = cfg
        print(case, json.dumps(cfg), flush=True)
        del keep
    out["map_after"] = dm.counts()
    dm.close()
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
