"""numpy restatement of Tracking::TrackLastFrame between Match() and SetPose
(core/frontend/tracking.cpp:291-325, :509-514, :539-541, :548-560; InitWithSecondFrame :211-245 is the
same with T_lw = identity), the specification of vx_track_essential_async (csrc/track_ess.hip): the
distance filter, the cv::Point2f pairs, ComputeParallax over the float positions, and
Sophus::SE3d(R, t) * T_lw restated as Shepperd's quaternion, the Hamilton product, Sophus's
first-order renormalisation and the rotated translation.  Plain sequential loops and scalar IEEE
double arithmetic in the order the kernel and visionx::SE3d use; pinned on hand-written cases by
tests/test_track_ess_cpu.py.  (findEssentialMat + recoverPose themselves: oracle.essential_ransac.)"""
import math

import numpy as np


def pose_from_Rt(R, t):
    """PoseFromRt (host/src/geometry.cpp): Eigen::Quaterniond(Matrix3d) by Shepperd's method, normalised.
    R: 9 doubles row-major.  Returns [qx qy qz qw tx ty tz]."""
    R = [float(v) for v in np.asarray(R, np.float64).reshape(9)]
    tr = R[0] + R[4] + R[8]
    if tr > 0.0:
        s = math.sqrt(tr + 1.0) * 2.0
        w = 0.25 * s; x = (R[7] - R[5]) / s; y = (R[2] - R[6]) / s; z = (R[3] - R[1]) / s
    elif R[0] > R[4] and R[0] > R[8]:
        s = math.sqrt(1.0 + R[0] - R[4] - R[8]) * 2.0
        w = (R[7] - R[5]) / s; x = 0.25 * s; y = (R[1] + R[3]) / s; z = (R[2] + R[6]) / s
    elif R[4] > R[8]:
        s = math.sqrt(1.0 + R[4] - R[0] - R[8]) * 2.0
        w = (R[2] - R[6]) / s; x = (R[1] + R[3]) / s; y = 0.25 * s; z = (R[5] + R[7]) / s
    else:
        s = math.sqrt(1.0 + R[8] - R[0] - R[4]) * 2.0
        w = (R[3] - R[1]) / s; x = (R[2] + R[6]) / s; y = (R[5] + R[7]) / s; z = 0.25 * s
    inv = 1.0 / math.sqrt(x * x + y * y + z * z + w * w)
    return np.array([x * inv, y * inv, z * inv, w * inv, float(t[0]), float(t[1]), float(t[2])], np.float64)


def compose(T_cl, T_lw):
    """Sophus::SE3d T_cl * T_lw on [qx qy qz qw tx ty tz]: q = q_cl (x) q_lw (Eigen's coefficient
    order), q *= 2 / (1 + |q|^2) when |q|^2 != 1, t = R(q_cl) t_lw + t_cl (Eigen's _transformVector)."""
    ax, ay, az, aw, atx, aty, atz = (float(v) for v in T_cl)
    bx, by, bz, bw, px, py, pz = (float(v) for v in T_lw)
    qw = aw * bw - ax * bx - ay * by - az * bz
    qx = aw * bx + ax * bw + ay * bz - az * by
    qy = aw * by + ay * bw + az * bx - ax * bz
    qz = aw * bz + az * bw + ax * by - ay * bx
    n2 = qx * qx + qy * qy + qz * qz + qw * qw
    if n2 != 1.0:
        sc = 2.0 / (1.0 + n2)
        qx *= sc; qy *= sc; qz *= sc; qw *= sc
    ux = ay * pz - az * py; uy = az * px - ax * pz; uz = ax * py - ay * px
    vx = 2 * ux; vy = 2 * uy; vz = 2 * uz
    return np.array([qx, qy, qz, qw,
                     px + aw * vx + (ay * vz - az * vy) + atx,
                     py + aw * vy + (az * vx - ax * vz) + aty,
                     pz + aw * vz + (ax * vy - ay * vx) + atz], np.float64)


def track_ess_ref(matches, last_xy, curr_xy, min_matches=50):
    """matches: records with query_idx / train_idx / distance (query = last frame feature, train =
    current frame feature); last_xy / curr_xy (n x 2 float32): the frames' positions as cv::Point2f.

    Returns a dict: n_matches, min_distance, thr (float32), good (indices into matches of the kept
    ones, in order), n_good_matches, n_bad_index, pair_match (indices into matches of the pairs, in
    order), pts_last / pts_curr (k x 2 float32), n_pairs, parallax (float64), gate (0 pass,
    1 FEW_MATCHES)."""
    last_xy = np.asarray(last_xy, np.float32).reshape(-1, 2)
    curr_xy = np.asarray(curr_xy, np.float32).reshape(-1, 2)
    dist = np.asarray(matches["distance"], np.float32)
    min_dist = np.float32(100.0)                           # :294
    for d in dist:
        if d < min_dist:
            min_dist = d
    thr = max(np.float32(2) * min_dist, np.float32(30.0))  # :299
    good = [i for i, d in enumerate(dist) if d <= thr]
    n_good = len(good)
    n_bad = 0
    pair_match, p1, p2 = [], [], []
    par = 0.0
    for i in good:
        q, t = int(matches["query_idx"][i]), int(matches["train_idx"][i])
        if not (0 <= q < len(last_xy) and 0 <= t < len(curr_xy)):
            n_bad += 1                                     # (the reference would index out of bounds)
            continue
        dx = float(last_xy[q, 0]) - float(curr_xy[t, 0])   # ComputeParallax: (p1 - p2).norm()
        dy = float(last_xy[q, 1]) - float(curr_xy[t, 1])
        par += math.sqrt(dx * dx + dy * dy)
        pair_match.append(i)
        p1.append(last_xy[q])                              # cv::Point2f (:512-513)
        p2.append(curr_xy[t])
    enough = n_good >= min_matches
    return {
        "n_matches": len(dist), "min_distance": np.float32(min_dist), "thr": np.float32(thr),
        "good": np.array(good, np.int32), "n_good_matches": n_good, "n_bad_index": n_bad,
        "pair_match": np.array(pair_match, np.int32),
        "pts_last": np.array(p1, np.float32).reshape(-1, 2), "pts_curr": np.array(p2, np.float32).reshape(-1, 2),
        "n_pairs": len(pair_match), "parallax": (par / n_good if enough and n_good else 0.0),
        "gate": 0 if enough else 1,
    }
