#!/usr/bin/env python3
"""Latency of map culling on the resident map (vx_dmap_cull_*), on one GPU.

For each size (C3: 50 + 2 keyframes / 20k landmarks, C4: 100 + 2 / 50k) and two maps — `clean`
(options under which nothing is culled: the scan alone) and `noisy` (lm_sigma = 0.03, about 40 % of the
landmarks removed) — medians and quartiles of:

  device      DMap.cull_landmarks / keyframe_redundancy / cull_keyframes, each cull on a freshly loaded
              map (a cull edits its map), timed around the call (it ends in its own synchronisation)
  composed    what a caller could do before: download() + the numpy restatement (tests/cull_ref.py,
              PYTHON loops: this leg measures interpreter time, not a fair host implementation) + the
              edit calls (set_landmark_bad / set_features / remove_landmarks)
  sequential  tests/cpp/cull_driver: a plain C++ walk of tracking.cpp:652-840 over host objects and,
              alternated with it in the same process, visionx::MapCulling (the device call plus the
              write-back onto the host objects), medians over --reps fresh maps

and the algorithmic bytes of the three landmark kernels (what the algorithm must move, from the
shapes).  --profile: run only a few device calls per map (for rocprofv3 --kernel-trace --stats).
Needs a GPU (there is no fallback).  Writes one JSON file.

  python scripts/cull_latency.py --out profiles/r09/cull_latency.json
"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
DRIVER = os.path.join(ROOT, "visionx-slam_amd", "build", "cull_driver")
FILES = ("kf_id", "kf_pose", "kf_intr", "kf_has_cam", "kf_feat_ptr", "feat_uv", "feat_lm_id", "feat_flags", "lm_id",
         "lm_pos", "lm_bad", "lm_obs_ptr", "obs_kf_id", "obs_feat_idx")


def stats(ms):
    q = np.percentile(np.asarray(ms, np.float64), [25, 50, 75])
    return {"median_ms": float(q[1]), "q25_ms": float(q[0]), "q75_ms": float(q[2]), "n": len(ms)}


def algorithmic_bytes(m, n_culled, n_reset):
    """bytes the landmark kernels must read and write once: the scan reads every landmark row (CSR
    pointers, bad flag, id, position) and every observation (keyframe id, feature index, the
    feature's flags, landmark id and pixel) and writes its four per-row results; the apply kernel
    reads the per-row results and, for a culled row, its observations again, and writes the records
    and the resets"""
    nl, no = len(m["lm_id"]), len(m["obs_kf_id"])
    scan = nl * (16 + 1 + 8 + 24 + 20) + no * (8 + 8 + 1 + 8 + 16)
    apply_ = nl * 8 + n_culled * (32 + 8 + 1) + n_reset * (16 + 8 + 16 + 9)
    return {"scan": int(scan), "apply": int(apply_), "landmarks": nl, "observations": no}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "cull_latency.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", nargs="+", default=["C3", "C4"])
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    import vxslam
    from vxslam import synth

    import cull_ref

    ctx = vxslam.Context(0)
    out = {"reps": a.reps, "configs": {}}
    for name in a.sizes:
        nk, nl, _ = synth.ba_config(name)
        for kind in ("clean", "noisy"):
            m = synth.make_cull_scene(0xC0 + nk, nk, nl, special=False, lm_sigma=0.03 if kind == "noisy" else 0.01)
            o = (vxslam.cull_options(min_landmark_observations=0, landmark_max_reproj_error=1e6)
                 if kind == "clean" else vxslam.cull_options())
            if kind == "clean":
                m["lm_bad"][:] = 0
            ok = vxslam.cull_options(kf_min_shared_observations=2, min_landmark_observations=o["min_landmark_observations"],
                                     landmark_max_reproj_error=o["landmark_max_reproj_error"])

            def fresh():
                dm = vxslam.DMap(ctx)
                cull_ref.load(dm, m)
                ctx.synchronize()
                return dm

            for _ in range(2):  # warm-up: code objects, pinned blocks
                dm = fresh()
                dm.cull_landmarks(o), dm.keyframe_redundancy(ok), dm.cull_keyframes(ok)
                dm.close()
            if a.profile:
                continue
            t_dev, t_comp, t_kf, t_red = [], [], [], []
            res = None
            for rep in range(a.reps):
                dm = fresh()
                t0 = time.perf_counter()
                res = dm.cull_landmarks(o)
                t_dev.append(1e3 * (time.perf_counter() - t0))
                dm.close()
                if rep < 3:  # (the restatement's Python loops take seconds at these sizes)
                    dm = fresh()
                    ref = m.copy()
                    t0 = time.perf_counter()
                    pose, pos = dm.download()
                    ref["kf_pose"], ref["lm_pos"] = pose, pos
                    want = cull_ref.cull_landmarks(ref, o)
                    cull_ref.apply_edits(dm, want)
                    ctx.synchronize()
                    t_comp.append(1e3 * (time.perf_counter() - t0))
                    assert np.array_equal(want["landmarks"]["row"], res["landmarks"]["row"])
                    dm.close()
                dm = fresh()
                for _ in range(3):
                    t0 = time.perf_counter()
                    dm.keyframe_redundancy(ok)
                    t_red.append(1e3 * (time.perf_counter() - t0))
                t0 = time.perf_counter()
                rk = dm.cull_keyframes(ok)
                t_kf.append(1e3 * (time.perf_counter() - t0))
                dm.close()
            cfg = {"keyframes": int(m["kf_alive"].sum()), "landmarks": nl, "observations": len(m["obs_kf_id"]),
                   "culled": len(res["landmarks"]), "features_reset": len(res["features"]),
                   "device_cull_landmarks": stats(t_dev), "composed_python": stats(t_comp),
                   "device_keyframe_redundancy": stats(t_red), "device_cull_keyframes": stats(t_kf),
                   "cull_keyframes_removed": bool(rk["removed"]), "cull_keyframes_landmarks": len(rk["landmarks"]),
                   "algorithmic_bytes": algorithmic_bytes(m, len(res["landmarks"]), len(res["features"]))}
            with tempfile.TemporaryDirectory() as d:
                for k in FILES:
                    np.ascontiguousarray(m[k]).tofile(os.path.join(d, k + ".bin"))
                np.ascontiguousarray(o).tofile(os.path.join(d, "opts.bin"))
                p = subprocess.run([DRIVER, d, "landmarks", str(a.reps)], capture_output=True, text=True, timeout=600)
                if p.returncode:
                    raise SystemExit(p.stderr)
                f = p.stdout.split()
                assert int(f[0]) == int(f[1]) == len(res["landmarks"]), f
                cfg["sequential_cpp_walk_ms"] = float(f[6])
                cfg["adapter_cull_landmarks_ms"] = float(f[7])
            out["configs"][f"{name}_{kind}"] = cfg
            print(name, kind, json.dumps(cfg), flush=True)
    ctx.close()
    if a.profile:
        return
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
