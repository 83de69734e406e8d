"""numpy restatement of the part of Tracking::TrackWithPnP between Match() and solvePnPRansac
(core/frontend/tracking.cpp:342-400) and of ComputeParallax (:548-560), the reference of
vx_track_pnp_async's pair gather (csrc/track.hip).  Plain sequential loops in the reference's order;
pinned on hand-written cases by tests/test_track_cpu.py."""
import numpy as np


def track_ref(matches, kf_uv, kf_lm_id, kf_flags, curr_xy, landmarks, min_matches=50, min_inliers=30,
              max_iterations=-1):
    """matches: records with query_idx / train_idx / distance (query = last keyframe feature, train =
    current frame feature); kf_uv (n x 2 float64), kf_lm_id, kf_flags (bit0 has_landmark, bit1
    is_outlier): the last keyframe's features; curr_xy (m x 2 float32): the current frame's positions;
    landmarks: {id: (position (3,) float64, bad flag)} of the landmarks Map::GetLandmark finds.

    Returns a dict: n_matches, min_distance, thr (float32), good (indices into matches of the kept
    ones, in order), n_good_matches, n_bad_index, pair_match (indices into matches of the pairs, in
    order), obj (k x 3 float32), img (k x 2 float32), n_pairs, parallax (float64), gate (0 pass,
    1 FEW_MATCHES, 2 FEW_PAIRS) and max_iterations (the budget solvePnPRansac gets, :421)."""
    kf_uv = np.asarray(kf_uv, np.float64).reshape(-1, 2)
    curr_xy = np.asarray(curr_xy, np.float32).reshape(-1, 2)
    dist = np.asarray(matches["distance"], np.float32)
    min_dist = np.float32(100.0)                       # :345
    for d in dist:
        if d < min_dist:
            min_dist = d
    thr = max(np.float32(2) * min_dist, np.float32(30.0))  # :350
    good = [i for i, d in enumerate(dist) if d <= thr]
    n_good = len(good)
    n_bad = 0
    pair_match, obj, img = [], [], []
    par = 0.0
    for i in good:
        q, t = int(matches["query_idx"][i]), int(matches["train_idx"][i])
        if not (0 <= q < len(kf_uv) and 0 <= t < len(curr_xy)):
            n_bad += 1                                 # (the reference would index out of bounds)
            continue
        dx = kf_uv[q, 0] - np.float64(curr_xy[t, 0])   # ComputeParallax: (p1 - p2).norm()
        dy = kf_uv[q, 1] - np.float64(curr_xy[t, 1])
        par += np.sqrt(dx * dx + dy * dy)
        fl = int(kf_flags[q])
        if not (fl & 1) or (fl & 2):                   # :375
            continue
        lm = landmarks.get(int(kf_lm_id[q]))           # :378
        if lm is None:
            continue
        p, bad = lm
        if bad:                                        # :382
            continue
        p = np.asarray(p, np.float64)
        if np.isnan(p).any():                          # :388
            continue
        if (np.abs(p) > 1000).any():                   # :391
            continue
        pair_match.append(i)
        obj.append(p.astype(np.float32))               # cv::Point3f
        img.append(curr_xy[t])
    enough = n_good >= min_matches
    n_pairs = len(pair_match)
    gate = 1 if not enough else (2 if n_pairs < min_inliers else 0)
    return {
        "n_matches": len(dist), "min_distance": np.float32(min_dist), "thr": np.float32(thr),
        "good": np.array(good, np.int32), "n_good_matches": n_good, "n_bad_index": n_bad,
        "pair_match": np.array(pair_match, np.int32),
        "obj": np.array(obj, np.float32).reshape(-1, 3), "img": np.array(img, np.float32).reshape(-1, 2),
        "n_pairs": n_pairs, "parallax": (par / n_good if enough and n_good else 0.0), "gate": gate,
        "max_iterations": min(100, 2 * n_pairs) if max_iterations < 0 else max_iterations,
    }
