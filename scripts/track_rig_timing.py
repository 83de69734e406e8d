#!/usr/bin/env python3
"""Host time of Track() for the eight cameras of a rig time step, frames already resident: the one-call rig
form against the two ways the single-camera call offers, alternated round by round in one session
(DESIGN.md §32).

  workload   eight cameras, synth.make_track_frame_scene with 2000 features each, uploaded into Frame handles
             once; ONE map: a C3-sized background (synth.make_ba_map: 52 keyframes, 20 000 landmarks) plus
             the eight last keyframes and their landmarks
  legs       a  vx_track_rig_async + vx_track_rig_fetch + eight vx_track_rig_keypoints        one context
             b  eight vx_track_frame_async + vx_track_frame_fetch in turn             one context
             c  eight contexts, one per camera: all enqueued, then all fetched         (4 hardware queues)
             every leg through the same raw ctypes calls on prebuilt arguments, every camera's keypoint rows
             copied into a user array;
             the host clock runs from the first enqueue to the end of the last fetch
  rigs       all eight PnP; all eight fallback (all but 20 landmark links cleared: FEW_PAIRS, then
             TrackLastFrame); seven PnP and one fallback
  rounds     20 warm-up + 300 timed, the legs alternated round by round; medians with quartiles, microseconds;
             the eight fetched records of the three legs are compared byte for byte
  stages     vx_prof_read of leg a over 20 further rounds per rig (per-dispatch kernel time, milliseconds a call)

Prints one JSON document and, with --out, writes it."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visionx-slam_amd", "python"))

import vxslam  # noqa: E402
from vxslam import synth  # noqa: E402

B, N = 8, 2000
KF0, LM0 = 1000000, 1 << 40


def few_flags(s):
    f = np.zeros(len(s["flags"]), np.uint8)
    f[np.nonzero(~s["wrong"])[0][:20]] = 1
    return f


def p(a):
    return C.c_void_p(a.ctypes.data)


class Rig:
    """one rig: a map of its own (the flags differ), the prebuilt arguments of the three legs"""

    def __init__(self, ctxs, scenes, frames, fallback, background):
        self.ctx = ctxs[0]
        self.dm = vxslam.DMap(self.ctx)
        vxslam.dmap_load(self.dm, background)
        assert not np.isin(KF0 + np.arange(B), background["kf_id"]).any()
        for i, s in enumerate(scenes):
            ids = s["lm_id"] + np.uint64(LM0 + i * 100000)
            self.dm.add_landmarks(ids, s["lm_pos"], None)
            self.dm.add_keyframe(KF0 + i, s["pose"], s["intr"], True, s["kf_uv"], ids, few_flags(s) if i in fallback else s["flags"])
        self.po, self.eo = (np.ascontiguousarray(o) for o in vxslam.track_frame_options())
        self.intr = [np.ascontiguousarray(s["intr"], np.float64) for s in scenes]
        self.pose = [np.ascontiguousarray(s["pose_last"], np.float64) for s in scenes]
        self.frames = frames
        self.tab = np.zeros(B, vxslam.RIG_CAMERA_DTYPE)
        for i, (kf, last, curr) in enumerate(frames):
            self.tab[i] = (KF0 + i, kf.handle.value, last.handle.value, curr.handle.value, self.pose[i].ctypes.data,
                           self.intr[i].ctypes.data)
        self.out = np.zeros(B, vxslam.TRACK_FRAME_RESULT_DTYPE)
        self.kp = np.zeros(N + 64, vxslam.KEYPOINT_DTYPE)
        self.ctxs = ctxs
        self.n = C.c_int(0)

    def leg_a(self):
        L, h = vxslam.lib(), self.ctx.handle
        t0 = time.perf_counter()
        rc = L.vx_track_rig_async(h, self.dm.handle, B, p(self.tab), C.c_float(0.8), p(self.po), p(self.eo))
        rc |= L.vx_track_rig_fetch(h, 1, p(self.out), B, None)
        for i in range(B):  # (the rows into a user array, as the single call's fetch copies them)
            rc |= L.vx_track_rig_keypoints(h, i, p(self.kp), len(self.kp), C.byref(self.n))
        t1 = time.perf_counter()
        assert rc == 0, vxslam.lib().vx_last_error(self.ctx.handle)
        return t1 - t0

    def single(self, L, h, i):
        kf, last, curr = self.frames[i]
        return L.vx_track_frame_async(h, self.dm.handle, C.c_uint64(KF0 + i), kf.handle, last.handle, curr.handle, C.c_float(0.8),
                                      p(self.pose[i]), p(self.intr[i]), p(self.po), p(self.eo))

    def fetch(self, L, h, i):
        return L.vx_track_frame_fetch(h, C.c_void_p(self.out.ctypes.data + i * self.out.itemsize), p(self.kp), len(self.kp),
                                      C.byref(self.n))

    def leg_b(self):
        L, h = vxslam.lib(), self.ctx.handle
        rc = 0
        t0 = time.perf_counter()
        for i in range(B):
            rc |= self.single(L, h, i)
            rc |= self.fetch(L, h, i)
        t1 = time.perf_counter()
        assert rc == 0, vxslam.lib().vx_last_error(self.ctx.handle)
        return t1 - t0

    def leg_c(self):
        L = vxslam.lib()
        rc = 0
        t0 = time.perf_counter()
        for i in range(B):
            rc |= self.single(L, self.ctxs[i].handle, i)
        for i in range(B):
            rc |= self.fetch(L, self.ctxs[i].handle, i)
        t1 = time.perf_counter()
        assert rc == 0
        return t1 - t0

    def paths(self):
        return [int(x) for x in self.out["path"]]

    def records(self):
        return self.out.tobytes()


def quartiles(t):
    t = np.sort(np.array(t)) * 1e6
    k = len(t)
    return {"q1": round(float(t[k // 4]), 1), "median": round(float(t[k // 2]), 1), "q3": round(float(t[(3 * k) // 4]), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=300)
    ap.add_argument("--out")
    a = ap.parse_args()
    ctxs = [vxslam.Context(0) for _ in range(B)]
    scenes = [synth.make_track_frame_scene(300 + i, N, wrong_frac=0.2) for i in range(B)]
    frames = [(vxslam.Frame(ctxs[0], N + 64).upload(ctxs[0], s["kf_uv"].astype(np.float32), s["desc_kf"]),
               vxslam.Frame(ctxs[0], N + 64).upload(ctxs[0], s["last_xy"], s["desc_last"]),
               vxslam.Frame(ctxs[0], N + 64).upload(ctxs[0], s["curr_xy"], s["desc_curr"])) for s in scenes]
    background = synth.make_ba_map(0xC3, 52, 20000)
    ctxs[0].synchronize()
    doc = {"cameras": B, "features": N, "map": {"keyframes": 52 + B, "landmarks": 20000 + B * N}, "warmup": a.warmup,
           "rounds": a.rounds, "unit": "microseconds", "rigs": {}}
    for name, fallback in (("all_pnp", ()), ("all_fallback", tuple(range(B))), ("seven_pnp_one_fallback", (3,))):
        rig = Rig(ctxs, scenes, frames, fallback, background)
        t = {"a": [], "b": [], "c": []}
        seen, recs = {}, {}
        for r in range(a.warmup + a.rounds):
            for leg in ("a", "b", "c"):
                dt = getattr(rig, "leg_" + leg)()
                seen[leg], recs[leg] = rig.paths(), rig.records()
                if r >= a.warmup:
                    t[leg].append(dt)
        assert seen["a"] == seen["b"] == seen["c"], seen
        assert recs["a"] == recs["b"] == recs["c"], "the three legs' records differ"  # (at the sizes timed)
        want = [vxslam.TRACK_PATH_ESSENTIAL if i in fallback else vxslam.TRACK_PATH_PNP for i in range(B)]
        assert seen["a"] == want, (seen["a"], want)
        rigdoc = {"paths": seen["a"],
                  "a_rig_call": quartiles(t["a"]), "b_eight_calls_one_context": quartiles(t["b"]),
                  "c_eight_contexts": quartiles(t["c"])}
        ctxs[0].prof_enable(True)
        ctxs[0].prof_read()
        for _ in range(20):
            rig.leg_a()
        prof = ctxs[0].prof_read()
        ctxs[0].prof_enable(False)
        rigdoc["a_stages_ms_per_call"] = {k: {"ms": round(v[0] / 20, 5), "launches": v[1] / 20} for k, v in prof.items() if v[1]}
        rigdoc["a_kernel_ms_per_call"] = round(sum(v[0] for v in prof.values()) / 20, 4)
        doc["rigs"][name] = rigdoc
        rig.dm.close()
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
