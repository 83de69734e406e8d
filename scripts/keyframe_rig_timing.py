#!/usr/bin/env python3
"""Keyframe creation for a rig in one call (vx_dmap_create_keyframes_rig) against one
vx_dmap_create_keyframe_frame per camera, on one GPU.

Map: C3 (50 + 2 keyframes / 20k landmarks, resident) plus one last keyframe per camera (2000 features).
Cameras: resident 2000-feature frames with their match lists on the device; `with_depth` gives every
camera a 640x480 u16 host depth image whose pixel is a hole under half of the features (DESIGN §28's
case, so both branches are populated), `no_depth` none (triangulation only).

Legs, alternated round by round in one process on ONE map, warm-up rounds first, medians and quartiles:

  rig      one DMap.create_keyframes_rig over B cameras
  single   B DMap.create_keyframe_frame calls in camera order, the landmark ids carried

for B = 8, 4 and 2.  After every leg the map is restored, untimed, to the same live state: the new
keyframes and the created landmarks are removed and the last keyframes' links reset, so every call of
either leg meets the same live map, the same ids and the same decisions (storage rows of removed
entries stay behind, as they do in a running system).  `faster` is claimed only where the rig leg's
upper quartile lies below the single leg's lower quartile.  Per-stage kernel time of the rig call at
B = 8 comes from vx_prof_read over rounds of their own (the event brackets perturb the wall time).

  python scripts/keyframe_rig_timing.py --out profiles/r16/keyframe_rig_timing.json
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

STAGES = ["rig_kf_feat", "rig_kf_match", "rig_kf_count", "rig_kf_commit"]


def stats(ms):
    q = np.percentile(np.asarray(ms, np.float64), [25, 50, 75])
    return {"median_ms": float(q[1]), "q25_ms": float(q[0]), "q75_ms": float(q[2]), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "keyframe_rig_timing.json"))
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--cameras", type=int, nargs="+", default=[8, 4, 2])
    a = ap.parse_args()
    import torch

    import vxslam
    from vxslam import synth

    import cull_ref

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
    n, bmax = a.features, max(a.cameras)
    kf0, new0, first = int(m["kf_id"].max()) + 1, int(m["kf_id"].max()) + 1001, int(m["lm_id"].max()) + 1
    scenes = [synth.make_keyframe_scene(0x4B46 + i, n) for i in range(bmax)]
    for i, d in enumerate(scenes):  # one last keyframe per camera
        link1 = np.where(d["has1"] > 0, 900000 + i * n + np.arange(n), 0).astype(np.uint64)
        dm.add_keyframe(kf0 + i, d["pose1"], d["intr"], True, d["uv1"], link1, d["has1"])
    frames = [vxslam.Frame(ctx, n).upload(ctx, d["uv2"].astype(np.float32), np.zeros((n, 32), np.uint8)) for d in scenes]
    keep, lists = [], []
    for d in scenes:
        mt = np.ascontiguousarray(d["matches"], vxslam.MATCH_DTYPE)
        keep += [dev(mt), dev(np.array([len(mt)], np.int32))]
        lists.append((keep[-2].data_ptr(), keep[-1].data_ptr(), len(mt)))
    ctx.synchronize()
    live0 = dm.live_counts()
    out = {"rounds": a.rounds, "warmup": a.warmup, "features": n,
           "map": {"keyframes": live0["kf"], "landmarks": live0["lm"], "observations": live0["obs"]},
           "matches": [len(d["matches"]) for d in scenes], "cases": {}}

    def cams(b, with_depth):
        return [{"kf_id": new0 + i, "pose7": d["pose2"], "intr4": d["intr"], "frame": frames[i], "last_kf_id": kf0 + i,
                 "matches": lists[i], "depth": d["depth"] if with_depth else None} for i, d in enumerate(scenes[:b])]

    def leg_rig(args):
        g = dm.create_keyframes_rig(args, first)
        return g["results"], g["landmarks"]

    def leg_single(args):
        nxt, res, recs = first, [], []
        for k in args:
            g = dm.create_keyframe_frame(k["kf_id"], k["pose7"], k["intr4"], k["frame"], last_kf_id=k["last_kf_id"],
                                         matches=k["matches"], depth=k["depth"], first_landmark_id=nxt)
            res.append(g["result"])
            recs.append(g["landmarks"].copy())
            nxt = int(g["result"]["next_landmark_id"])
        return res, np.concatenate(recs)

    def restore(args, res, recs):
        """the live map as it was before the leg"""
        for k in args:
            dm.remove_keyframe(k["kf_id"])
        if len(recs):
            dm.remove_landmarks(recs["lm_id"])
        at = 0
        for k, r in zip(args, res):
            mine = recs[at:at + int(r["n_depth"]) + int(r["n_triangulated"])]
            at += len(mine)
            tri = mine[mine["kind"] == 1]["feat_last"]
            dm.set_features(k["last_kf_id"], tri, np.zeros(len(tri), np.uint64), np.zeros(len(tri), np.uint8))
        ctx.synchronize()
        assert dm.live_counts() == live0

    for case in ("with_depth", "no_depth"):
        out["cases"][case] = {}
        for b in a.cameras:
            args = cams(b, case == "with_depth")
            legs = {"rig": leg_rig, "single": leg_single}
            times = {k: [] for k in legs}
            blob = {}
            for rnd in range(-a.warmup, a.rounds):
                for name, leg in legs.items():
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    res, recs = leg(args)
                    ctx.synchronize()
                    dt = 1e3 * (time.perf_counter() - t0)
                    if rnd >= 0:
                        times[name].append(dt)
                    # (the storage row differs from leg to leg: removed landmarks keep theirs)
                    blob[name] = (b"".join(r.tobytes() for r in res),
                                  tuple(recs[f].tobytes() for f in ("lm_id", "kind", "feat_curr", "feat_last", "pw")))
                    made = [(int(r["n_depth"]), int(r["n_triangulated"])) for r in res]
                    restore(args, res, recs)
                assert blob["rig"] == blob["single"], "the legs disagree"
            cfg = {k: stats(v) for k, v in times.items()}
            cfg["made"] = made
            cfg["faster"] = bool(cfg["rig"]["q75_ms"] < cfg["single"]["q25_ms"])
            cfg["single_over_rig_median"] = cfg["single"]["median_ms"] / cfg["rig"]["median_ms"]
            if b == bmax:  # per-stage kernel time, rounds of their own
                ctx.prof_enable(True, STAGES)
                for _ in range(20):
                    res, recs = leg_rig(args)
                    restore(args, res, recs)
                p = ctx.prof_read()
                ctx.prof_enable(False)
                cfg["rig_stage_us_per_call"] = {s: 1e3 * p[s][0] / max(p[s][1], 1) for s in STAGES}
                cfg["rig_stage_launches_per_call"] = {s: p[s][1] / 20 for s in STAGES}
            out["cases"][case]["B%d" % b] = cfg
            print(case, b, json.dumps(cfg), flush=True)
    out["map_after"] = dm.counts()
    dm.close()
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
