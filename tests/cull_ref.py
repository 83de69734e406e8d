"""Tracking::CullLandmarks, Tracking::RemoveKeyFrame and Tracking::CullKeyFrames
(core/frontend/tracking.cpp:652-840) restated over a synth.BAMap with synth.cull_state's membership
arrays: plain loops in the reference's order, the edits made in place.  The reference of
tests/test_gpu_cull.py and of the C++ adapter's test.

Rows are storage rows, as in the resident map: a removed keyframe / landmark keeps its row
(kf_alive = 0 / lm_removed = 1) and its id may live again in a later row.  A landmark's observations
are its lm_obs_ptr segment in insertion order; the walk of :680-711 goes through them in that order
(the reference's unordered_map order changes neither the outcome nor any reported number but the
count at a break)."""
import numpy as np

import vxslam
from vxslam import synth

RESET = 2  # feature flags after a reset: has_landmark false, is_outlier true


def _opt(o, k):
    return o[k].item() if hasattr(o[k], "item") else o[k]


def _live_kf(m):
    return {int(m["kf_id"][k]): int(k) for k in range(len(m["kf_id"])) if m["kf_alive"][k]}  # later rows win


def _live_lm(m):
    return {int(m["lm_id"][r]): int(r) for r in range(len(m["lm_id"])) if not m["lm_removed"][r]}


def _rot(q):
    """Eigen Quaternion::toRotationMatrix"""
    x, y, z, w = (float(v) for v in q)
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return ((1.0 - (tyy + tzz), txy - twz, txz + twy), (txy + twz, 1.0 - (txx + tzz), tyz - twx),
            (txz - twy, tyz + twx, 1.0 - (txx + tyy)))


def _obs(m, r):
    """the live (keyframe id, feature index) pairs of landmark row r, insertion order"""
    o0, o1 = int(m["lm_obs_ptr"][r]), int(m["lm_obs_ptr"][r + 1])
    return [(int(m["obs_kf_id"][o]), int(m["obs_feat_idx"][o])) for o in range(o0, o1) if m["obs_live"][o]]


def observation_count(m, r):
    return len(_obs(m, r))


def _empty():
    return {"landmarks": np.zeros(0, vxslam.CULL_LANDMARK_DTYPE), "features": np.zeros(0, vxslam.CULL_FEATURE_DTYPE)}


def cull_landmarks(m, o):
    """Tracking::CullLandmarks.  Returns {"landmarks", "features"} as DMap.cull_landmarks does."""
    synth.cull_state(m)
    lms = _live_lm(m)
    if len(lms) < _opt(o, "min_landmarks_for_culling"):                       # (:656)
        return _empty()
    kfs = _live_kf(m)
    tau = float(_opt(o, "landmark_max_reproj_error"))
    pose, intr, uv = m["kf_pose"].reshape(-1, 7), m["kf_intr"].reshape(-1, 4), m["feat_uv"].reshape(-1, 2)
    fptr = m["kf_feat_ptr"]
    rot = {}
    recs = []
    for r in sorted(lms.values()):
        lid = int(m["lm_id"][r])
        if m["lm_bad"][r]:                                                    # (:666)
            recs.append((lid, r, vxslam.CULL_ALREADY_BAD, 0, 0, 0.0))
            continue
        obs = _obs(m, r)
        if len(obs) < _opt(o, "min_landmark_observations"):                   # (:670)
            recs.append((lid, r, vxslam.CULL_FEW_OBSERVATIONS, 0, 0, 0.0))
            continue
        p = [float(v) for v in m["lm_pos"].reshape(-1, 3)[r]]
        err_sum, cnt, large = 0.0, 0, False
        for kid, fi in obs:
            k = kfs.get(kid)
            if k is None:                                                     # (:682)
                continue
            if fi >= fptr[k + 1] - fptr[k]:                                   # (:685)
                continue
            g = int(fptr[k]) + fi
            if not (m["feat_flags"][g] & 1) or int(m["feat_lm_id"][g]) != lid:  # (:689)
                continue
            if not m["kf_has_cam"][k]:                                        # (:694)
                continue
            if k not in rot:
                rot[k] = (_rot(pose[k][:4]), [float(v) for v in pose[k][4:]], [float(v) for v in intr[k]])
            R, t, c = rot[k]
            pc = [R[i][0] * p[0] + R[i][1] * p[1] + R[i][2] * p[2] + t[i] for i in range(3)]
            if pc[2] <= 1e-6:                                                 # ProjectToPixel (projection.h:17)
                continue
            inv_z = 1.0 / pc[2]
            pu, pv = c[0] * (pc[0] * inv_z) + c[2], c[1] * (pc[1] * inv_z) + c[3]
            dx, dy = float(uv[g][0]) - pu, float(uv[g][1]) - pv
            err = float(np.sqrt(dx * dx + dy * dy))
            err_sum += err
            cnt += 1
            if err > tau * 2.0:                                               # (:707)
                large = True
                break
        if cnt == 0:                                                          # (:713)
            recs.append((lid, r, vxslam.CULL_NO_PROJECTION, 0, 0, 0.0))
        elif large:
            recs.append((lid, r, vxslam.CULL_LARGE_ERROR, cnt, 0, 0.0))
        elif err_sum / cnt > tau:                                             # (:719)
            recs.append((lid, r, vxslam.CULL_MEAN_ERROR, cnt, 0, err_sum / cnt))
    feats = []
    for lid, r, *_ in recs:                                                   # (:729-747)
        m["lm_bad"][r] = 1  # SetBad (where it was not)
        for kid, fi in _obs(m, r):
            k = kfs.get(kid)
            if k is None or fi >= fptr[k + 1] - fptr[k]:
                continue
            g = int(fptr[k]) + fi
            if int(m["feat_lm_id"][g]) == lid:
                m["feat_lm_id"][g] = 0
                m["feat_flags"][g] = RESET
                feats.append((kid, k, fi))
        m["lm_removed"][r] = 1
    return {"landmarks": np.array(recs, vxslam.CULL_LANDMARK_DTYPE), "features": np.array(feats, vxslam.CULL_FEATURE_DTYPE)}


def keyframe_redundancy(m, o):
    """(total, redundant) of tracking.cpp:804-820 for every live keyframe in ascending id."""
    synth.cull_state(m)
    kfs, lms = _live_kf(m), _live_lm(m)
    ids, tot, red = [], [], []
    for kid in sorted(kfs):
        k = kfs[kid]
        total = redundant = 0
        for g in range(int(m["kf_feat_ptr"][k]), int(m["kf_feat_ptr"][k + 1])):
            if not (m["feat_flags"][g] & 1):
                continue
            total += 1
            r = lms.get(int(m["feat_lm_id"][g]))
            if r is None or m["lm_bad"][r]:
                continue
            if observation_count(m, r) >= _opt(o, "kf_min_shared_observations"):
                redundant += 1
        ids.append(kid), tot.append(total), red.append(redundant)
    return {"kf_id": np.array(ids, np.uint64), "total": np.array(tot, np.int32), "redundant": np.array(red, np.int32)}


def remove_keyframe(m, kid):
    """Tracking::RemoveKeyFrame (:752-773).  Returns (feature indices reset, landmark ids whose
    observation of the keyframe was removed)."""
    synth.cull_state(m)
    kfs, lms = _live_kf(m), _live_lm(m)
    k = kfs[int(kid)]
    reset, gone = [], []
    for g in range(int(m["kf_feat_ptr"][k]), int(m["kf_feat_ptr"][k + 1])):
        if not (m["feat_flags"][g] & 1):
            continue
        lid = int(m["feat_lm_id"][g])
        r = lms.get(lid)
        if r is None:
            continue
        for o in range(int(m["lm_obs_ptr"][r]), int(m["lm_obs_ptr"][r + 1])):
            if m["obs_live"][o] and int(m["obs_kf_id"][o]) == int(kid):
                m["obs_live"][o] = 0
                gone.append(lid)
        m["feat_lm_id"][g] = 0
        m["feat_flags"][g] = RESET
        reset.append(g - int(m["kf_feat_ptr"][k]))
    m["kf_alive"][k] = 0
    return reset, gone


def cull_keyframes(m, o, protect=()):
    """Tracking::CullKeyFrames (:775-840).  Returns what DMap.cull_keyframes does, plus "removed_obs"
    (the landmark ids RemoveKeyFrame took the keyframe's observation from) for the edit path."""
    synth.cull_state(m)
    out = {"removed": False, "kf_id": 0, "ratio": 0.0, "removed_obs": [], "kf_features": [], **_empty()}
    kfs = _live_kf(m)
    if len(kfs) <= _opt(o, "min_keyframes_for_culling"):                      # (:781)
        return out
    exceeded = _opt(o, "max_keyframes") > 0 and len(kfs) > _opt(o, "max_keyframes")
    red = keyframe_redundancy(m, o)
    for kid, total, redundant in zip(red["kf_id"], red["total"], red["redundant"]):
        if int(kid) in {int(p) for p in protect} or total == 0:
            continue
        ratio = float(redundant) / float(total)
        if ratio > _opt(o, "kf_redundant_ratio") and (exceeded or ratio > 0.95):  # (:827)
            k = kfs[int(kid)]
            reset, gone = remove_keyframe(m, kid)
            res = cull_landmarks(m, o)                                        # (:838)
            own = np.array([(int(kid), k, fi) for fi in reset], vxslam.CULL_FEATURE_DTYPE)
            return {"removed": True, "kf_id": int(kid), "ratio": ratio, "removed_obs": gone, "kf_features": reset,
                    "landmarks": res["landmarks"], "features": np.concatenate([res["features"], own])}
    return out


def apply_edits(dm, res):
    """The decisions of `res` (a result of cull_landmarks / cull_keyframes above) made on a DMap through
    the edit calls that existed before the device culling: the state it must equal."""
    if res.get("removed"):
        kid = res["kf_id"]
        gone = np.array(res["removed_obs"], np.uint64)
        dm.remove_observations(gone, np.full(len(gone), kid, np.uint64))
        fi = np.array(res["kf_features"], np.int32)
        dm.set_features(kid, fi, np.zeros(len(fi), np.uint64), np.full(len(fi), RESET, np.uint8))
        dm.remove_keyframe(kid)
    lm, ft = res["landmarks"], res["features"]
    if res.get("removed"):
        ft = ft[:len(ft) - len(res["kf_features"])]
    if len(lm):
        dm.set_landmark_bad(lm["lm_id"], np.ones(len(lm), np.uint8))
    for kid in np.unique(ft["kf_id"]):
        fi = ft["feat_idx"][ft["kf_id"] == kid]
        dm.set_features(int(kid), fi, np.zeros(len(fi), np.uint64), np.full(len(fi), RESET, np.uint8))
    if len(lm):
        dm.remove_landmarks(lm["lm_id"])


def load(dm, m):
    """Fill a DMap so that its storage rows are m's: keyframes in row order (a row whose id is held
    by an earlier, dead row is inserted after that one was removed), landmarks in row order, each
    landmark's observations in list order; then the removals m's state records."""
    synth.cull_state(m)
    pose, intr, uv = m["kf_pose"].reshape(-1, 7), m["kf_intr"].reshape(-1, 4), m["feat_uv"].reshape(-1, 2)
    in_map = {}
    for k, kid in enumerate(int(i) for i in m["kf_id"]):
        if kid in in_map:
            assert not m["kf_alive"][in_map[kid]]
            dm.remove_keyframe(kid)
        f0, f1 = m["kf_feat_ptr"][k], m["kf_feat_ptr"][k + 1]
        dm.add_keyframe(kid, pose[k], intr[k], m["kf_has_cam"][k], uv[f0:f1], m["feat_lm_id"][f0:f1], m["feat_flags"][f0:f1])
        in_map[kid] = k
    for kid, k in in_map.items():
        if not m["kf_alive"][k]:
            dm.remove_keyframe(kid)
    assert len(set(m["lm_id"].tolist())) == len(m["lm_id"]), "load: landmark ids must be unique"
    if len(m["lm_id"]):
        dm.add_landmarks(m["lm_id"], m["lm_pos"].reshape(-1, 3), m["lm_bad"])
        lm = np.repeat(np.arange(len(m["lm_id"])), np.diff(m["lm_obs_ptr"]))
        if len(lm):
            dm.add_observations(m["lm_id"][lm], m["obs_kf_id"], m["obs_feat_idx"])
            dead = np.nonzero(m["obs_live"] == 0)[0]
            if len(dead):
                dm.remove_observations(m["lm_id"][lm[dead]], m["obs_kf_id"][dead])
        gone = np.nonzero(m["lm_removed"])[0]
        if len(gone):
            dm.remove_landmarks(m["lm_id"][gone])
