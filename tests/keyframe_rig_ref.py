"""vx_dmap_create_keyframes_rig restated in numpy: keyframe_ref.create_keyframe chained over the cameras
of a rig step with the landmark ids carried, all or nothing.  Every camera is decided first (on a copy
of the map that takes the cameras before it, which is where its rows and ids come from); the caller's
map is edited only when every camera passed.  What the rig call refuses on top of the single call —
a keyframe id or a last keyframe id named twice, a last keyframe that is not live before the call —
is decided here on the map as it was before the call.

A camera is a dict: kf_id, pose7, intr4, uv ((n, 2) float64), last_kf_id (None: no last keyframe),
matches (MATCH_DTYPE, None), depth (2-D image, None)."""
import numpy as np

import vxslam
from vxslam import synth

import keyframe_ref as R

ERR_ID_RANGE, ERR_RIG_REPEAT = 32, 64


def with_last_keyframes(m, scenes, first_kf_id):
    """map m (edited in place) with the first frame of every scene appended as a keyframe of its own
    (keyframe_ref.with_last_keyframe once per camera): ids first_kf_id, first_kf_id + 1, ..."""
    for i, d in enumerate(scenes):
        R.with_last_keyframe(m, d, first_kf_id + i)
    return [first_kf_id + i for i in range(len(scenes))]


def camera(d, kf_id, last_kf_id, depth=True, last=True, matches=None):
    """a camera of the rig step from a keyframe_ref scene: its second frame, with or without the depth
    image, with or without its last keyframe"""
    return {"kf_id": int(kf_id), "pose7": d["pose2"], "intr4": d["intr"], "uv": d["uv2"],
            "last_kf_id": int(last_kf_id) if last else None,
            "matches": (d["matches"] if matches is None else matches) if last else None,
            "depth": d["depth"] if depth else None}


def host_bits(m, cams, first_landmark_id, caps=None):
    """the error bits found before anything runs, per camera, on the map as it is before the call;
    caps: the frames' capacities (the id range covers their sum), default the feature counts"""
    live = R._live_kf(m)
    ids = set(int(x) for x, rm in zip(m["lm_id"], m["lm_removed"]) if not rm)
    caps = [len(np.asarray(k["uv"]).reshape(-1, 2)) for k in cams] if caps is None else caps
    hit = any((int(first_landmark_id) + i) in ids for i in range(int(sum(caps))))
    bits = []
    for i, k in enumerate(cams):
        b = ERR_ID_RANGE if hit else 0  # the range is the call's: every camera carries it
        if k["kf_id"] in live:
            b |= R.ERR_KF_LIVE
        if k["intr4"] is None:
            b |= R.ERR_NO_CAMERA
        if k["last_kf_id"] is not None:
            kl = live.get(k["last_kf_id"])
            if kl is None:
                b |= R.ERR_NO_LAST
            elif not m["kf_has_cam"][kl]:
                b |= R.ERR_NO_CAMERA
        for j, o in enumerate(cams):
            if j == i:
                continue
            if o["kf_id"] == k["kf_id"]:
                b |= ERR_RIG_REPEAT
            if k["last_kf_id"] is not None and o["last_kf_id"] == k["last_kf_id"]:
                b |= ERR_RIG_REPEAT
        bits.append(b)
    return bits


def create_keyframes_rig(m, cams, first_landmark_id=0, opts=None, caps=None):
    """Returns {"error_bits": [per camera], "cameras": [keyframe_ref.create_keyframe's dict per camera],
    "landmarks": all cameras' records in camera order (None when rejected), "first": [first landmark id
    per camera], "next_landmark_id"}.  m is edited only when every camera's error_bits is 0."""
    synth.cull_state(m)
    bits = host_bits(m, cams, first_landmark_id, caps)
    out = {"error_bits": bits, "cameras": [], "landmarks": None, "first": [], "next_landmark_id": int(first_landmark_id)}
    if any(bits):
        return out
    work = m.copy()
    first = int(first_landmark_id)
    for i, k in enumerate(cams):
        # (a camera with a fault edits nothing; the ones after it are still decided for their own bits,
        # which do not depend on where their rows would have begun)
        res = R.create_keyframe(work, k["kf_id"], k["pose7"], k["intr4"], k["uv"], k["last_kf_id"], k["matches"],
                                k["depth"], first, opts)
        out["cameras"].append(res)
        out["first"].append(first)
        bits[i] = res["error_bits"]
        first += len(res["landmarks"])
    if any(bits):
        return out
    out["landmarks"] = np.concatenate([np.zeros(0, vxslam.KEYFRAME_LANDMARK_DTYPE)] + [r["landmarks"] for r in out["cameras"]])
    out["next_landmark_id"] = first
    for k in list(work.keys()):
        m[k] = work[k]
    return out
