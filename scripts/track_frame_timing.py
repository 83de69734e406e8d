#!/usr/bin/env python3
"""Host time of one tracked frame from image hand-over to pose, the resident-frame adapters against the
default host-input adapters of the same tree, alternated in one session.

Writes a scene and runs `resident_driver timing` (tests/cpp/resident_driver.cpp) on it:

  image      one 640x480 BGR frame of synth.make_frames; the CURRENT frame of every round is extracted
             from it for real (ORBExtractor, 2000 features), in the default mode by Extract (upload,
             extraction, fetch of keypoints + descriptors) and in the resident mode by ExtractResident
  map        a C3-sized background (synth.make_ba_map: 52 keyframes, 20 000 landmarks) plus the scene's
             last keyframe, whose features are the extracted keypoints seen from a nearby pose: their
             descriptors are the current ones with up to 24 bits flipped, their landmarks the keypoints
             back-projected at a random depth (a fifth of them at a wrong place)
  last frame the same keypoints from a second nearby pose (a fifth at random pixels)

  cases      a PnP frame; a fallback frame (all but 20 landmark links cleared: FEW_PAIRS, then
             TrackLastFrame); a keyframe (the PnP frame followed by CreateKeyFrame with a depth image:
             the default mode matches on the host, the resident mode reuses the track's device list; the
             map grows by that keyframe every round, in both modes alike)
  modes      default  = ORBExtractor::Extract, FrameTracker::Track, KeyFrameLandmarks::CreateKeyFrame
             resident = ExtractResident, TrackResident, CreateKeyFrame over the track's match list
             each on a map of its own, alternated round by round; 20 warm-up + 300 timed rounds (100 for
             the keyframe case); medians with quartiles, microseconds

Prints one JSON document and, with --out, writes it."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visionx-slam_amd", "python"))

import vxslam  # noqa: E402
from vxslam import synth  # noqa: E402

DRIVER = os.path.join(ROOT, "visionx-slam_amd", "build", "resident_driver")
MAP_FILES = ("kf_id", "kf_pose", "kf_intr", "kf_has_cam", "kf_feat_ptr", "feat_uv", "feat_lm_id", "feat_flags", "lm_id",
             "lm_pos", "lm_bad", "lm_obs_ptr", "obs_kf_id", "obs_feat_idx")
W, H = 640, 480


def nearby(rng, q_cw, t_cw, pc, intr, rot_deg, baseline, noise_px):
    """the points pc (current camera frame) seen from a camera a small motion away: (pose7 of that
    camera, its pixels)"""
    fx, fy, cx, cy = intr
    q = synth.quat_from_rotvec(rng.normal(0, 1, 3) * np.deg2rad(rot_deg) / np.sqrt(3))
    R = synth.quat_to_mat(q)
    d = rng.normal(0, 1, 3)
    d[2] *= 0.3
    t = baseline * d / np.linalg.norm(d)
    p = pc @ R.T + t
    uv = np.stack([fx * p[:, 0] / p[:, 2] + cx, fy * p[:, 1] / p[:, 2] + cy], -1) + rng.normal(0, noise_px, (len(pc), 2))
    qw = synth.quat_mul(q, q_cw)
    if qw[3] < 0:
        qw = -qw
    return np.concatenate([qw, R @ t_cw + t]), uv


def write_scene(path, n_features, seed=41):
    rng = np.random.default_rng(seed)
    ctx = vxslam.Context(0)
    img = np.ascontiguousarray(synth.make_frames(seed, 1, H, W)[0])
    kp, desc = ctx.orb_extract(img, vxslam.default_orb_params(n_features=n_features))
    ctx.close()
    n = len(kp)
    intr = np.array([synth.FX, synth.FY, synth.CX, synth.CY], np.float64)
    perm = rng.permutation(n)
    xy = np.stack([kp["x"], kp["y"]], -1).astype(np.float64)[perm]   # keyframe feature i is keypoint perm[i]
    z = rng.uniform(1.0, 6.0, n)
    pc = np.stack([(xy[:, 0] - intr[2]) / intr[0] * z, (xy[:, 1] - intr[3]) / intr[1] * z, z], -1)
    q_cw = synth.quat_from_rotvec(rng.normal(0, 0.3, 3))
    if q_cw[3] < 0:
        q_cw = -q_cw
    R_cw, t_cw = synth.quat_to_mat(q_cw), rng.normal(0, 0.5, 3)
    pw = (pc - t_cw) @ R_cw
    kf_pose, kf_uv = nearby(rng, q_cw, t_cw, pc, intr, 3.0, 0.3, 0.5)
    pose_last, last_xy = nearby(rng, q_cw, t_cw, pc, intr, 2.0, 0.15, 0.5)
    wrong = rng.random(n) < 0.2
    pw[wrong] += rng.normal(0, 1.0, (int(wrong.sum()), 3))
    last_xy[wrong] = np.stack([rng.uniform(0, W, wrong.sum()), rng.uniform(0, H, wrong.sum())], -1)
    flips = rng.integers(0, 25, (2, n))
    rows = []
    for k in range(2):
        bits = np.unpackbits(desc[perm], axis=1)
        for i in range(n):
            bits[i, rng.choice(256, flips[k, i], replace=False)] ^= 1
        rows.append(np.packbits(bits, axis=1))
    few = np.zeros(n, np.uint8)
    few[np.nonzero(~wrong)[0][:20]] = 1
    bg = synth.make_ba_map(0xC3, 50, 20000)
    for k in MAP_FILES:
        np.ascontiguousarray(bg[k]).tofile(os.path.join(path, k + ".bin"))
    out = dict(image=img, depth=np.ascontiguousarray(synth.make_depth(seed, H, W)), intr=intr, scene_kf_pose=kf_pose,
               pose_last=pose_last, kf_uv=kf_uv, kf_lm_id=(10_000_000 + np.arange(n)).astype(np.uint64), kf_lm_pos=pw,
               flags_pnp=np.ones(n, np.uint8), flags_few=few, desc_kf=rows[0], desc_last=rows[1],
               last_xy=last_xy.astype(np.float32), meta=np.array([n_features], np.int32))
    for k, v in out.items():
        np.ascontiguousarray(v).tofile(os.path.join(path, k + ".bin"))
    return {"extracted_features": int(n), "background_keyframes": int(len(bg["kf_id"])), "background_landmarks": int(len(bg["lm_id"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=300)
    ap.add_argument("--keyframe-rounds", type=int, default=100)
    ap.add_argument("--out")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as path:
        doc = write_scene(path, a.features)
        r = subprocess.run([DRIVER, "timing", path, str(a.warmup), str(a.rounds), str(a.keyframe_rounds)],
                           capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.exit(r.stderr)
    doc.update(image=[W, H, 3], warmup=a.warmup, rounds=a.rounds, keyframe_rounds=a.keyframe_rounds, cases={})
    for line in r.stdout.splitlines():
        case, mode, q1, med, q3, ok, fallback, inliers, feats = line.split()
        doc["cases"].setdefault(case, {})[mode] = {"median_us": float(med), "q1_us": float(q1), "q3_us": float(q3),
                                                   "returned": int(ok), "used_fallback": int(fallback),
                                                   "inliers": int(inliers), "features": int(feats)}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
