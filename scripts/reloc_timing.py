#!/usr/bin/env python3
"""Relocalisation in one call (vx_relocalize_async + vx_relocalize_fetch) against what a caller
can do today, on one GPU.

Map: C3 (50 + 2 keyframes / 20k landmarks, resident) plus B candidate keyframes of `--features` features that
all see one scene's landmarks (synth.make_track_frame_scene), each through descriptors of its own (its own
Hamming distances) and its own 60 % of the landmark links.  The current frame is the scene's, resident.

Legs, alternated round by round in one process on ONE map, warm-up rounds first, medians and quartiles:

  reloc    one Context.relocalize_async + relocalize_fetch over the B candidates
  frames   B Context.track_frame_async + track_frame_fetch (without keypoints) in turn, one per candidate:
           B synchronisations, and no attempt sees more than one keyframe's landmarks
  rig      one Context.track_rig_async + track_rig_fetch with the candidates as cameras that share the
           current frame, if that call accepts it (`refused` holds its message otherwise)

for B = 4, 8 and 16.  The legs do not compute the same thing (one pooled PnP against B separate ones), so what
is compared is the time a caller waits; `faster_than_*` is claimed only where the reloc leg's upper quartile
lies below the other leg's lower quartile.  Per-stage kernel time of the reloc call at the largest B comes from
vx_prof_read over rounds of their own (the event brackets perturb the wall time).

  python scripts/reloc_timing.py --out profiles/r21/reloc_timing.json
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

STAGES = ["match_partial", "match_merge", "reloc_pairs", "reloc_pool", "pnp_hypotheses", "pnp_refine", "reloc_final"]


def stats(ms):
    q = np.percentile(np.asarray(ms, np.float64), [25, 50, 75])
    return {"median_ms": float(q[1]), "q25_ms": float(q[0]), "q75_ms": float(q[2]), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21", "reloc_timing.json"))
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--candidates", type=int, nargs="+", default=[4, 8, 16])
    a = ap.parse_args()
    import torch  # noqa: F401  (its HIP runtime first, as tests/conftest.py)

    import vxslam
    from vxslam import synth

    import cull_ref

    ctx = vxslam.Context(0)
    nk, nl, _ = synth.ba_config("C3")
    m = synth.make_cull_scene(0xC0 + nk, nk, nl, special=False)
    dm = vxslam.DMap(ctx)
    cull_ref.load(dm, m)
    n, bmax = a.features, max(a.candidates)
    s = synth.make_track_frame_scene(0x2E10C, n, wrong_frac=0.3)
    rng = np.random.default_rng(0x2E10C)
    kf0 = int(m["kf_id"].max()) + 1
    lm_id = s["lm_id"] + np.uint64(int(m["lm_id"].max()) + 1)
    dm.add_landmarks(lm_id, s["lm_pos"], None)
    curr = vxslam.Frame(ctx, n).upload(ctx, s["curr_xy"], s["desc_curr"])
    cands = []
    for c in range(bmax):
        bits = np.unpackbits(s["desc_curr"][s["train_of"]], axis=1)
        for i, f in enumerate(rng.integers(0, 25, n)):
            bits[i, rng.choice(256, int(f), replace=False)] ^= 1
        fr = vxslam.Frame(ctx, n).upload(ctx, s["kf_uv"].astype(np.float32), np.packbits(bits, axis=1))
        dm.add_keyframe(kf0 + c, s["pose"], s["intr"], True, s["kf_uv"], lm_id, (rng.random(n) < 0.6).astype(np.uint8))
        cands.append((kf0 + c, fr))
    ctx.synchronize()
    live = dm.live_counts()
    po = vxslam.track_options()
    fo = vxslam.track_frame_options()
    out = {"rounds": a.rounds, "warmup": a.warmup, "features": n,
           "map": {"keyframes": live["kf"], "landmarks": live["lm"], "observations": live["obs"]}, "cases": {}}

    def leg_reloc(sel):
        ctx.relocalize_async(dm, sel, curr, s["intr"], po)
        r = ctx.relocalize_fetch()["result"]
        return {"status": int(r["status"]), "n_pool": int(r["n_pool"]), "inliers": int(r["pnp"]["n_inliers"])}

    def leg_frames(sel):
        got = []
        for kf_id, fr in sel:
            ctx.track_frame_async(dm, kf_id, fr, None, curr, s["intr"], fo)
            r = ctx.track_frame_fetch(keypoints=False)["result"]
            got.append((int(r["status"]), int(r["pnp"]["n_pairs"]), int(r["n_inliers"])))
        return {"status": [g[0] for g in got], "n_pairs": [g[1] for g in got], "inliers": [g[2] for g in got]}

    def leg_rig(sel):
        ctx.track_rig_async(dm, [vxslam.rig_camera(curr, s["intr"], last_kf_id=k, last_kf=f) for k, f in sel], fo)
        got = ctx.track_rig_fetch(keypoints=False)
        return {"status": [int(g["result"]["status"]) for g in got], "inliers": [int(g["result"]["n_inliers"]) for g in got]}

    for b in a.candidates:
        sel = cands[:b]
        legs = {"reloc": leg_reloc, "frames": leg_frames, "rig": leg_rig}
        cfg = {}
        try:
            leg_rig(sel)
        except vxslam.VxError as e:
            cfg["rig_refused"] = str(e)
            del legs["rig"]
        times = {k: [] for k in legs}
        for rnd in range(-a.warmup, a.rounds):
            for name, leg in legs.items():
                ctx.synchronize()
                t0 = time.perf_counter()
                res = leg(sel)
                dt = 1e3 * (time.perf_counter() - t0)
                if rnd >= 0:
                    times[name].append(dt)
                cfg.setdefault("results", {})[name] = res
        for k, v in times.items():
            cfg[k] = stats(v)
        for other in ("frames", "rig"):
            if other in times:
                cfg["faster_than_" + other] = bool(cfg["reloc"]["q75_ms"] < cfg[other]["q25_ms"])
                cfg[other + "_over_reloc_median"] = cfg[other]["median_ms"] / cfg["reloc"]["median_ms"]
        if b == bmax:  # per-stage kernel time, rounds of their own
            ctx.prof_enable(True, STAGES)
            for _ in range(20):
                leg_reloc(sel)
            p = ctx.prof_read()
            ctx.prof_enable(False)
            cfg["reloc_stage_us_per_call"] = {st: 1e3 * p[st][0] / max(p[st][1], 1) for st in STAGES}
            cfg["reloc_stage_launches_per_call"] = {st: p[st][1] / 20 for st in STAGES}
        out["cases"]["B%d" % b] = cfg
        print(b, json.dumps(cfg), flush=True)
    dm.close()
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
