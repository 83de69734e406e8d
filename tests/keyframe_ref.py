"""Tracking::CreateKeyFrame (core/frontend/tracking.cpp:577-584) restated in numpy over a synth.BAMap
with synth.cull_state's membership arrays (the dict format of cull_ref.load): CreateLandmarksFromDepth
(:586-650) over every feature, then TriangulateWithLastKeyFrame (:856-945) over the match list in
order, each marking features as it goes, then Map::InsertKeyFrame — the decision, the records and the
map edit.  The reference of tests/test_gpu_keyframe.py and of the C++ adapter's test; pinned against
the chained oracle calls by tests/test_keyframe_cpu.py.

The depth branch repeats the device's IEEE operations one by one (Eigen's quaternion rotation,
Sophus' inverse), so its points are compared bit for bit; the triangulated point comes from
numpy's SVD and is compared to 1e-9."""
import numpy as np

import vxslam
from vxslam import synth

ERR_MATCH_RANGE, ERR_DUP_QUERY, ERR_KF_LIVE, ERR_NO_LAST, ERR_NO_CAMERA = 1, 2, 4, 8, 16


def _qrot(q, v):
    """Eigen _transformVector: q * v, componentwise in its operation order (v: (n, 3) or (3,))"""
    v = np.asarray(v, np.float64)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    qx, qy, qz, qw = (float(c) for c in q)
    ux, uy, uz = qy * z - qz * y, qz * x - qx * z, qx * y - qy * x
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    cx, cy, cz = qy * uz - qz * uy, qz * ux - qx * uz, qx * uy - qy * ux
    return np.stack([x + qw * ux + cx, y + qw * uy + cy, z + qw * uz + cz], -1)


def _inv_apply(pose, p):
    """Sophus T.inverse() * p"""
    q, t = pose[:4], pose[4:]
    qc = (-q[0], -q[1], -q[2], q[3])
    ti = _qrot(qc, np.array([t[0] * -1.0, t[1] * -1.0, t[2] * -1.0]))
    return _qrot(qc, p) + ti


def _rot(q):
    """Eigen Quaternion::toRotationMatrix"""
    x, y, z, w = (float(v) for v in q)
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


def depth_points(uv, depth, intr, pose):
    """CreateLandmarksFromDepth for features without links: (feature indices, world points)"""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    if depth is None or depth.size == 0 or len(uv) == 0:
        return np.zeros(0, np.int64), np.zeros((0, 3))
    x, y = uv[:, 0], uv[:, 1]
    with np.errstate(invalid="ignore"):
        u, v = np.trunc(x + 0.5), np.trunc(y + 0.5)  # static_cast<int>
    inside = (u >= 0) & (u < depth.shape[1]) & (v >= 0) & (v < depth.shape[0])
    ui, vi = np.where(inside, u, 0).astype(np.int64), np.where(inside, v, 0).astype(np.int64)
    raw = depth[vi, ui]
    if depth.dtype == np.uint16:
        have = raw != 0
        d = raw.astype(np.float64) / 5000.0
    else:
        have = np.ones(len(raw), bool)
        d = raw.astype(np.float64)
    ok = inside & have & ~((d < 0.1) | (d > 10.0))
    idx = np.nonzero(ok)[0]
    fx, fy, cx, cy = (float(c) for c in intr)
    xn, yn, dd = (x[idx] - cx) / fx, (y[idx] - cy) / fy, d[idx]
    return idx, _inv_apply(np.asarray(pose, np.float64), np.stack([xn * dd, yn * dd, dd], -1)).reshape(-1, 3)


def _project(intr, R, t, pw):
    pc = R @ pw + t
    if pc[2] <= 1e-6:
        return None, pc[2]
    return np.array([intr[0] * (pc[0] / pc[2]) + intr[2], intr[1] * (pc[1] / pc[2]) + intr[3]]), pc[2]


def _gate(p1, p2, c1, c2, pose1, pose2, min_angle_rad, max_err, mg):
    """one match of TriangulateWithLastKeyFrame after its has_landmark tests; mg collects the margins"""
    R1, R2 = _rot(pose1[:4]), _rot(pose2[:4])
    t1, t2 = pose1[4:], pose2[4:]
    f1 = np.array([(p1[0] - c1[2]) / c1[0], (p1[1] - c1[3]) / c1[1], 1.0])
    f2 = np.array([(p2[0] - c2[2]) / c2[0], (p2[1] - c2[3]) / c2[1], 1.0])
    g1, g2 = R1.T @ (f1 / np.linalg.norm(f1)), R2.T @ (f2 / np.linalg.norm(f2))
    ang = np.arccos(np.clip(g1 @ g2 / (np.linalg.norm(g1) * np.linalg.norm(g2)), -1.0, 1.0))
    mg["angle"].append(abs(ang - min_angle_rad) / min_angle_rad)
    if ang < min_angle_rad:
        return None
    K = np.array([[c2[0], 0, c2[2]], [0, c2[1], c2[3]], [0, 0, 1.0]])  # the current camera for both (:865-868)
    P1, P2 = K @ np.column_stack([R1, t1]), K @ np.column_stack([R2, t2])
    A = np.stack([p1[0] * P1[2] - P1[0], p1[1] * P1[2] - P1[1], p2[0] * P2[2] - P2[0], p2[1] * P2[2] - P2[1]])
    X = np.linalg.svd(A)[2][-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        pw = X[:3] / X[3]
    if not np.isfinite(pw).all():
        return None
    for intr, R, t, px in ((c1, R1, t1, p1), (c2, R2, t2, p2)):
        uv, z = _project(intr, R, t, pw)
        mg["z"].append(abs(z - 1e-6) / 1e-6)
        if uv is None:
            return None
        e = float(np.hypot(uv[0] - px[0], uv[1] - px[1]))
        mg["err"].append(abs(e - max_err) / max_err)
        if e > max_err:
            return None
    return pw


def _live_kf(m):
    return {int(m["kf_id"][k]): int(k) for k in range(len(m["kf_id"])) if m["kf_alive"][k]}


def decide(m, kf_id, pose7, intr4, uv, last_kf_id, matches, depth, first_id, opts=None):
    """The chained decision on map m (not edited).  Returns {"error_bits", "landmarks":
    KEYFRAME_LANDMARK_DTYPE records in creation order (row = the landmark's row after the edit),
    "n_depth", "n_triangulated", "margins": {"angle", "err", "z"} (min relative distance of every
    compared quantity from its threshold; inf when nothing was compared)}."""
    synth.cull_state(m)
    o = vxslam.keyframe_options() if opts is None else opts
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    pose7 = np.asarray(pose7, np.float64)
    kfs = _live_kf(m)
    bits = 0
    if int(kf_id) in kfs:
        bits |= ERR_KF_LIVE
    if intr4 is None:
        bits |= ERR_NO_CAMERA
    kl = None
    if last_kf_id is not None:
        kl = kfs.get(int(last_kf_id))
        if kl is None:
            bits |= ERR_NO_LAST
        elif not m["kf_has_cam"][kl]:
            bits |= ERR_NO_CAMERA
    out = {"error_bits": bits, "landmarks": np.zeros(0, vxslam.KEYFRAME_LANDMARK_DTYPE), "n_depth": 0,
           "n_triangulated": 0, "margins": {"angle": np.inf, "err": np.inf, "z": np.inf}}
    if bits:
        return out
    n, n_lm = len(uv), len(m["lm_id"])
    recs = []
    di, dp = depth_points(uv, depth, intr4, pose7)
    has_cur = np.zeros(n, bool)
    for i, p in zip(di.tolist(), dp):
        recs.append((int(first_id) + len(recs), n_lm + len(recs), 0, i, -1, p))
        has_cur[i] = True
    nd = len(recs)
    mg = {"angle": [], "err": [], "z": []}
    if kl is not None and matches is not None and len(matches):
        f0, f1 = int(m["kf_feat_ptr"][kl]), int(m["kf_feat_ptr"][kl + 1])
        q, t = matches["query_idx"].astype(np.int64), matches["train_idx"].astype(np.int64)
        if ((q < 0) | (q >= f1 - f0) | (t < 0) | (t >= n)).any():
            bits |= ERR_MATCH_RANGE
        qin = q[(q >= 0) & (q < f1 - f0) & (t >= 0) & (t < n)]  # (the device counts a query once its match is in range)
        if len(np.unique(qin)) != len(qin):
            bits |= ERR_DUP_QUERY
        if bits:
            out["error_bits"] = bits
            return out
        uv1 = m["feat_uv"].reshape(-1, 2)[f0:f1]
        has_last = (m["feat_flags"][f0:f1] & 1).astype(bool)
        pose1, c1 = m["kf_pose"].reshape(-1, 7)[kl], m["kf_intr"].reshape(-1, 4)[kl]
        c2 = np.asarray(intr4, np.float64)
        min_ang = float(o["tri_min_angle_deg"]) * np.pi / 180.0
        max_err = float(o["tri_max_reproj_error"])
        for qi, ti in zip(q.tolist(), t.tolist()):
            if has_last[qi] or has_cur[ti]:
                continue
            pw = _gate(uv1[qi], uv[ti], c1, c2, pose1, pose7, min_ang, max_err, mg)
            if pw is None:
                continue
            recs.append((int(first_id) + len(recs), n_lm + len(recs), 1, ti, qi, pw))
            has_last[qi] = has_cur[ti] = True
    out["landmarks"] = np.array([(r[0], r[1], r[2], r[3], r[4], tuple(r[5])) for r in recs],
                                vxslam.KEYFRAME_LANDMARK_DTYPE).reshape(-1)
    out["n_depth"], out["n_triangulated"] = nd, len(recs) - nd
    out["margins"] = {k: (float(min(v)) if v else np.inf) for k, v in mg.items()}
    return out


def margins(res):
    """{"angle", "err", "z"} of a decide() / create_keyframe() result"""
    return res["margins"]


def observations(recs, kf_id, last_kf_id):
    """(landmark ids, keyframe ids, feature indices) the records add, in creation order: a depth
    landmark (kf_id, i); a triangulated one (last_kf_id, queryIdx) then (kf_id, trainIdx) (:916-917)"""
    lm, kf, fi = [], [], []
    for r in recs:
        if r["kind"] == 1:
            lm.append(r["lm_id"]), kf.append(last_kf_id), fi.append(r["feat_last"])
        lm.append(r["lm_id"]), kf.append(kf_id), fi.append(r["feat_curr"])
    return np.array(lm, np.uint64), np.array(kf, np.uint64), np.array(fi, np.uint64)


def feature_links(recs, n_feat):
    """(lm ids, flags) of the new keyframe's features after the call: unlinked = (0, 0)"""
    lm, fl = np.zeros(n_feat, np.uint64), np.zeros(n_feat, np.uint8)
    lm[recs["feat_curr"]] = recs["lm_id"]
    fl[recs["feat_curr"]] = 1
    return lm, fl


def apply(m, kf_id, pose7, intr4, uv, last_kf_id, recs):
    """the map edit of the records on the dict m, in place (new rows at the end of every table)"""
    synth.cull_state(m)
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    n = len(uv)
    tri = recs[recs["kind"] == 1]
    if len(tri):
        kl = _live_kf(m)[int(last_kf_id)]
        g = int(m["kf_feat_ptr"][kl]) + tri["feat_last"]
        m["feat_lm_id"][g] = tri["lm_id"]
        m["feat_flags"][g] = 1
    lm, fl = feature_links(recs, n)
    ol, ok, of = observations(recs, kf_id, last_kf_id)
    cnt = np.where(recs["kind"] == 1, 2, 1)
    m["lm_id"] = np.concatenate([m["lm_id"], recs["lm_id"]]).astype(np.uint64)
    m["lm_pos"] = np.concatenate([m["lm_pos"].reshape(-1, 3), recs["pw"].reshape(-1, 3)])
    m["lm_bad"] = np.concatenate([m["lm_bad"], np.zeros(len(recs), np.uint8)])
    m["lm_removed"] = np.concatenate([m["lm_removed"], np.zeros(len(recs), np.uint8)])
    m["lm_obs_ptr"] = np.concatenate([m["lm_obs_ptr"], m["lm_obs_ptr"][-1] + np.cumsum(cnt)]).astype(np.int64)
    m["obs_kf_id"] = np.concatenate([m["obs_kf_id"], ok]).astype(np.uint64)
    m["obs_feat_idx"] = np.concatenate([m["obs_feat_idx"], of]).astype(np.uint64)
    m["obs_live"] = np.concatenate([m["obs_live"], np.ones(len(ok), np.uint8)])
    m["kf_id"] = np.concatenate([m["kf_id"], [kf_id]]).astype(np.uint64)
    m["kf_pose"] = np.concatenate([m["kf_pose"].reshape(-1, 7), np.asarray(pose7, np.float64).reshape(1, 7)])
    m["kf_intr"] = np.concatenate([m["kf_intr"].reshape(-1, 4), np.asarray(intr4, np.float64).reshape(1, 4)])
    m["kf_has_cam"] = np.concatenate([m["kf_has_cam"], np.ones(1, np.uint8)])
    m["kf_alive"] = np.concatenate([m["kf_alive"], np.ones(1, np.uint8)])
    m["kf_feat_ptr"] = np.concatenate([m["kf_feat_ptr"], [m["kf_feat_ptr"][-1] + n]]).astype(np.int64)
    m["feat_uv"] = np.concatenate([m["feat_uv"].reshape(-1, 2), uv])
    m["feat_lm_id"] = np.concatenate([m["feat_lm_id"], lm]).astype(np.uint64)
    m["feat_flags"] = np.concatenate([m["feat_flags"], fl]).astype(np.uint8)
    return m


def create_keyframe(m, kf_id, pose7, intr4, uv, last_kf_id=None, matches=None, depth=None, first_landmark_id=0,
                    opts=None):
    """decide() then apply(): what DMap.create_keyframe* must return and leave.  A rejected call
    (error_bits != 0) leaves m as it was."""
    res = decide(m, kf_id, pose7, intr4, uv, last_kf_id, matches, depth, first_landmark_id, opts)
    if not res["error_bits"]:
        apply(m, kf_id, pose7, intr4, uv, last_kf_id, res["landmarks"])
    return res


def apply_edits(dm, kf_id, pose7, intr4, uv, last_kf_id, recs):
    """The records made on a DMap through the four edit calls that existed before the one call
    (INTEGRATION.md §3): the state it must equal."""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    dm.add_landmarks(recs["lm_id"], recs["pw"].reshape(-1, 3), np.zeros(len(recs), np.uint8))
    dm.add_observations(*observations(recs, kf_id, last_kf_id))
    tri = recs[recs["kind"] == 1]
    if last_kf_id is not None:
        dm.set_features(last_kf_id, tri["feat_last"], tri["lm_id"], np.ones(len(tri), np.uint8))
    lm, fl = feature_links(recs, len(uv))
    dm.add_keyframe(kf_id, pose7, intr4, 1, uv, lm, fl)


LAST_KF_ID = 7


def scene_map(d, last_kf_id=LAST_KF_ID):
    """a synth.make_keyframe_scene dict's first frame as a one-keyframe map: its linked features
    (has1) name ids that are not in the map, as features of culled landmarks do"""
    n = len(d["uv1"])
    m = synth.BAMap()
    m["kf_id"] = np.array([last_kf_id], np.uint64)
    m["kf_pose"] = np.asarray(d["pose1"], np.float64).reshape(1, 7).copy()
    m["kf_intr"] = np.asarray(d["intr"], np.float64).reshape(1, 4).copy()
    m["kf_has_cam"] = np.ones(1, np.uint8)
    m["kf_feat_ptr"] = np.array([0, n], np.int64)
    m["feat_uv"] = np.asarray(d["uv1"], np.float64).reshape(-1, 2).copy()
    m["feat_lm_id"] = np.where(d["has1"] > 0, 900000 + np.arange(n), 0).astype(np.uint64)
    m["feat_flags"] = d["has1"].astype(np.uint8).copy()
    m["lm_id"] = np.zeros(0, np.uint64)
    m["lm_pos"] = np.zeros((0, 3))
    m["lm_bad"] = np.zeros(0, np.uint8)
    m["lm_obs_ptr"] = np.zeros(1, np.int64)
    m["obs_kf_id"] = np.zeros(0, np.uint64)
    m["obs_feat_idx"] = np.zeros(0, np.uint64)
    return synth.cull_state(m)


# the scenes of tests/test_gpu_keyframe.py: (seed, n features, with depth); B = the commit workgroup
def scene_sizes(block):
    return [0, 1, 63, 64, 65, block - 1, block, block + 1, 2 * block + 3, 2000]


_scenes = {}


def scene(n, with_depth):
    """the shared scene of a size (built once, never changed: callers copy what they edit)"""
    key = (int(n), bool(with_depth))
    if key not in _scenes:
        d = synth.make_keyframe_scene(5100 + n, max(n, 1), with_depth=with_depth)
        if n == 0:  # a frame without features and without matches against a last keyframe with one feature
            d["uv2"], d["has2"], d["matches"] = d["uv2"][:0], d["has2"][:0], d["matches"][:0]
        _scenes[key] = d
    return _scenes[key]


def with_last_keyframe(m, d, kf_id=LAST_KF_ID):
    """map m (edited in place) with the scene's first frame appended as its newest keyframe"""
    one = scene_map(d, kf_id)
    synth.cull_state(m)
    n = len(d["uv1"])
    for k, w in (("kf_id", None), ("kf_pose", 7), ("kf_intr", 4), ("kf_has_cam", None), ("kf_alive", None),
                 ("feat_uv", 2), ("feat_lm_id", None), ("feat_flags", None)):
        a, b = (m[k], one[k]) if w is None else (m[k].reshape(-1, w), one[k].reshape(-1, w))
        m[k] = np.concatenate([a, b]).astype(m[k].dtype)
    m["kf_feat_ptr"] = np.concatenate([m["kf_feat_ptr"], [m["kf_feat_ptr"][-1] + n]]).astype(np.int64)
    return m


def edit_scene(seed=61):
    """6 keyframes / 300 landmarks (synth.make_cull_scene) with the first frame of a 300-feature pair
    as the newest keyframe: (map, pair, last keyframe id, new keyframe id, first free landmark id)"""
    d = synth.make_keyframe_scene(seed, 300)
    m = synth.make_cull_scene(seed, 6, 300, special=False)
    last = int(m["kf_id"].max()) + 1
    with_last_keyframe(m, d, last)
    return m, d, last, last + 1, int(m["lm_id"].max()) + 1
