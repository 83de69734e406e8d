"""Seeded synthetic workloads shaped like the reference's inputs.

The TUM RGB-D sequences and real keyframe maps are not available offline, so every bench line
and parity test runs on data generated here:

* ``make_texture`` / ``make_frames`` — 640x480 (or any size) BGR8 frames cut from one textured
  plane with a small per-frame camera shift, uint16 depth (metres x 5000, tracking.cpp:603).
* ``make_ba_map`` — a flattened snapshot of ``visionx::Map`` (core/map/map.h:13-34,
  landmark.h:12-68, frame.h:16-64) holding a sliding BA window: keyframe poses ``T_cw`` on a
  smooth arc, landmarks observed by 2..5 consecutive keyframes, observations = true projection
  + N(0, 0.5 px) truncated at 1.5 px, poses perturbed by ~0.2 deg / 1 cm and landmarks by 1 cm.
  It also plants the corner cases LocalBA::Optimize handles (local_ba.cpp:66-249): older
  keyframes outside the window, single-observation landmarks (used by the pose stage only),
  bad landmarks, outlier features and features without a landmark.

Intrinsics default to 520.9/521.0/325.1/249.7 (apps/mono_demo.cpp:26-27).
"""
from __future__ import annotations

import numpy as np

FX, FY, CX, CY = 520.9, 521.0, 325.1, 249.7


# --------------------------------------------------------------------------- images
def _value_noise(rng, h, w, cell):
    gh, gw = h // cell + 3, w // cell + 3
    g = rng.random((gh, gw)).astype(np.float32)
    ys = np.arange(h, dtype=np.float32) / cell
    xs = np.arange(w, dtype=np.float32) / cell
    y0 = ys.astype(np.int64)
    x0 = xs.astype(np.int64)
    fy = (ys - y0)[:, None]
    fx = (xs - x0)[None, :]
    fy = fy * fy * (3 - 2 * fy)
    fx = fx * fx * (3 - 2 * fx)
    a = g[y0][:, x0]
    b = g[y0][:, x0 + 1]
    c = g[y0 + 1][:, x0]
    d = g[y0 + 1][:, x0 + 1]
    return (a * (1 - fx) + b * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy


def make_texture(seed: int, h: int, w: int, n_rects: int | None = None) -> np.ndarray:
    """Gray uint8 texture: multi-octave value noise plus random rectangles (strong corners)."""
    rng = np.random.default_rng(seed)
    t = np.zeros((h, w), np.float32)
    for cell, amp in ((64, 0.45), (24, 0.3), (9, 0.2), (4, 0.12)):
        t += amp * _value_noise(rng, h, w, cell)
    t = (t - t.mean()) / (t.std() + 1e-6) * 38.0 + 110.0
    if n_rects is None:
        n_rects = max(8, (h * w) // 1500)
    for _ in range(n_rects):
        rh, rw = rng.integers(4, 40, size=2)
        y, x = rng.integers(0, h - rh), rng.integers(0, w - rw)
        t[y:y + rh, x:x + rw] += rng.choice([-1.0, 1.0]) * rng.uniform(35, 90)
    return np.clip(t, 0, 255).astype(np.uint8)


def make_frames(seed: int, n: int, h: int = 480, w: int = 640, step=(3, 2)) -> np.ndarray:
    """n BGR8 frames (n, h, w, 3) cut from one texture, shifted by ``step`` px per frame, with
    per-channel tint and per-frame noise."""
    rng = np.random.default_rng(seed + 1)
    sy, sx = step
    tex = make_texture(seed, h + abs(sy) * n + 8, w + abs(sx) * n + 8)
    out = np.empty((n, h, w, 3), np.uint8)
    for i in range(n):
        y0 = 4 + (sy * i if sy >= 0 else abs(sy) * (n - i))
        x0 = 4 + (sx * i if sx >= 0 else abs(sx) * (n - i))
        g = tex[y0:y0 + h, x0:x0 + w].astype(np.int16)
        noise = rng.integers(-2, 3, size=(h, w), dtype=np.int16)
        for c, tint in enumerate((-6, 0, 9)):
            out[i, :, :, c] = np.clip(g + noise + tint, 0, 255).astype(np.uint8)
    return out


def make_depth(seed: int, h: int = 480, w: int = 640) -> np.ndarray:
    """uint16 depth image, metres x 5000 in [0.5, 4] m (tracking.cpp:603 scale)."""
    rng = np.random.default_rng(seed + 7)
    d = 0.5 + 3.5 * _value_noise(rng, h, w, 80)
    return (d * 5000).astype(np.uint16)


# --------------------------------------------------------------------------- BA maps
def quat_from_rotvec(v):
    v = np.asarray(v, np.float64)
    th = np.linalg.norm(v, axis=-1, keepdims=True)
    half = 0.5 * th
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.where(th > 1e-12, np.sin(half) / th, 0.5)
    return np.concatenate([v * k, np.cos(half)], axis=-1)  # x y z w


def quat_to_mat(q):
    x, y, z, w = np.moveaxis(np.asarray(q, np.float64), -1, 0)
    return np.stack([
        np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
        np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
        np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1),
    ], -2)


def quat_mul(a, b):
    ax, ay, az, aw = np.moveaxis(a, -1, 0)
    bx, by, bz, bw = np.moveaxis(b, -1, 0)
    return np.stack([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz], -1)


class BAMap(dict):
    """Flattened visionx::Map snapshot: a dict of numpy arrays plus scalars."""

    @property
    def n_kf(self):
        return int(self["kf_id"].shape[0])

    @property
    def n_lm(self):
        return int(self["lm_id"].shape[0])

    @property
    def n_obs(self):
        return int(self["obs_kf_id"].shape[0])

    def copy(self):
        return BAMap({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in self.items()})


def make_ba_map(seed: int, n_kf: int = 10, n_lm: int = 2000, *, n_old_kf: int = 2,
                extra_feats_per_kf: int = 40, frac_single: float = 0.03, frac_bad: float = 0.01,
                frac_outlier: float = 0.01, noise_px: float = 0.5, noise_clip: float = 1.5,
                rot_deg: float = 0.2, trans_m: float = 0.01, lm_sigma: float = 0.01,
                width: int = 640, height: int = 480, intr=(FX, FY, CX, CY),
                n_streams: int = 1, cross_frac: float = 0.0) -> BAMap:
    """A BA window of ``n_kf`` keyframes (+ ``n_old_kf`` older keyframes outside the window) and
    ``n_lm`` landmarks.  ``n_streams`` > 1 builds a multi-camera rig (configs C5): keyframes are
    split into streams, each stream observing its own landmark subset.  ``cross_frac`` > 0 makes
    the rig one body: that fraction of the landmarks lies in the field of view the stream shares
    with its neighbour (the next camera, 360 / n_streams degrees further round the rig) and is
    observed by both, so the streams' keyframes form ONE covisibility component (config C5's
    global window; with 0 every stream is a component of its own).

    Returns a BAMap with the vx_map_view / orc_map_view fields.  Landmark ids are random uint64,
    keyframe ids increase with time but are not contiguous."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = intr
    K_all = n_kf + n_old_kf
    per_stream = K_all // n_streams
    assert per_stream * n_streams == K_all, "n_kf + n_old_kf must divide by n_streams"

    # ---- ground-truth camera trajectory (camera-to-world), per stream an offset arc
    idx = np.arange(K_all)
    stream = idx % n_streams
    tpos = idx // n_streams  # time index inside a stream
    yaw = np.deg2rad(0.35) * tpos + stream * (2 * np.pi / max(n_streams, 1))
    centres = np.stack([0.04 * tpos * np.cos(yaw) + 0.3 * stream,
                        0.01 * np.sin(tpos / 5.0),
                        0.04 * tpos * np.sin(yaw) * 0.2], -1)
    q_wc = quat_from_rotvec(np.stack([np.deg2rad(0.1) * np.sin(tpos / 7.0), yaw, np.zeros(K_all)], -1))
    R_wc = quat_to_mat(q_wc)
    R_cw = np.transpose(R_wc, (0, 2, 1))
    t_cw = -np.einsum("kij,kj->ki", R_cw, centres)
    q_cw = q_wc * np.array([-1, -1, -1, 1.0])

    # ---- landmarks: each observed by L in {2..5} consecutive KFs of one stream
    lm_stream = rng.integers(0, n_streams, size=n_lm)
    L = np.minimum(rng.integers(2, 6, size=n_lm), per_stream)
    n_single = int(round(frac_single * n_lm))
    L[:n_single] = 1  # depth landmarks observed once (pose stage only)
    start = rng.integers(0, per_stream, size=n_lm)
    start = np.minimum(start, per_stream - L)
    start = np.maximum(start, 0)
    anchor_t = start + L // 2
    anchor = anchor_t * n_streams + lm_stream
    u = rng.uniform(20, width - 20, size=n_lm)
    v = rng.uniform(20, height - 20, size=n_lm)
    z = rng.uniform(1.0, 5.0, size=n_lm)
    pc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], -1)
    p_true = np.einsum("nij,nj->ni", R_wc[anchor], pc) + centres[anchor]

    # observations
    obs_lm = np.repeat(np.arange(n_lm), L)
    within = np.arange(obs_lm.shape[0]) - np.repeat(np.cumsum(L) - L, L)
    obs_t = start[obs_lm] + within
    obs_kf = obs_t * n_streams + lm_stream[obs_lm]
    if cross_frac > 0 and n_streams > 1:
        # shared landmarks: 15-28 degrees off the anchor camera's axis towards the next camera
        # (its yaw is 360 / n_streams degrees larger), 2-5 m deep, observed by that camera too at
        # the same times wherever the point projects inside its image (separate generator, so the
        # maps of cross_frac = 0 are unchanged)
        rc = np.random.default_rng(seed ^ 0xC5C5C5)
        cand = np.nonzero(L >= 2)[0]
        sh = np.sort(rc.choice(cand, size=min(len(cand), int(round(cross_frac * n_lm))), replace=False))
        th = np.deg2rad(rc.uniform(15.0, 28.0, size=len(sh)))
        zs = rc.uniform(2.0, 5.0, size=len(sh))
        u[sh] = cx + np.tan(th) * fx
        v[sh] = rc.uniform(60, height - 60, size=len(sh))
        z[sh] = zs
        pcs_a = np.stack([(u[sh] - cx) / fx * zs, (v[sh] - cy) / fy * zs, zs], -1)
        p_true[sh] = np.einsum("nij,nj->ni", R_wc[anchor[sh]], pcs_a) + centres[anchor[sh]]
        x_lm = np.repeat(sh, L[sh])
        x_t = start[x_lm] + (np.arange(len(x_lm)) - np.repeat(np.cumsum(L[sh]) - L[sh], L[sh]))
        x_kf = x_t * n_streams + (lm_stream[x_lm] + 1) % n_streams
        pc2 = np.einsum("oij,oj->oi", R_cw[x_kf], p_true[x_lm]) + t_cw[x_kf]
        z2 = np.where(pc2[:, 2] > 0.3, pc2[:, 2], 1.0)
        u2, v2 = fx * pc2[:, 0] / z2 + cx, fy * pc2[:, 1] / z2 + cy
        vis = (pc2[:, 2] > 0.3) & (u2 > 20) & (u2 < width - 20) & (v2 > 20) & (v2 < height - 20)
        obs_lm = np.concatenate([obs_lm, x_lm[vis]])
        obs_t = np.concatenate([obs_t, x_t[vis]])
        obs_kf = np.concatenate([obs_kf, x_kf[vis]])
        L = np.bincount(obs_lm, minlength=n_lm)
    pcs = np.einsum("oij,oj->oi", R_cw[obs_kf], p_true[obs_lm]) + t_cw[obs_kf]
    uv = np.stack([fx * pcs[:, 0] / pcs[:, 2] + cx, fy * pcs[:, 1] / pcs[:, 2] + cy], -1)
    nz = np.clip(rng.normal(0, noise_px, size=uv.shape), -noise_clip, noise_clip)
    uv = uv + nz

    # ---- features per KF: observations (shuffled) + features without a landmark
    n_obs = obs_lm.shape[0]
    order = np.lexsort((rng.random(n_obs), obs_kf))
    feat_kf = obs_kf[order]
    feat_uv = uv[order]
    feat_lm = obs_lm[order]
    counts = np.bincount(feat_kf, minlength=K_all)
    extra = np.full(K_all, extra_feats_per_kf)
    # interleave: per KF, obs features then extra features
    tot = counts + extra
    feat_ptr = np.zeros(K_all + 1, np.int64)
    feat_ptr[1:] = np.cumsum(tot)
    nf = int(feat_ptr[-1])
    f_uv = rng.uniform([0, 0], [width, height], size=(nf, 2))
    f_lm_idx = np.full(nf, -1, np.int64)
    obs_start = np.zeros(K_all + 1, np.int64)
    obs_start[1:] = np.cumsum(counts)
    pos_in_kf = np.arange(n_obs) - obs_start[feat_kf]
    fpos = feat_ptr[feat_kf] + pos_in_kf
    f_uv[fpos] = feat_uv
    f_lm_idx[fpos] = feat_lm
    flags = (f_lm_idx >= 0).astype(np.uint8)
    n_out = int(round(frac_outlier * n_obs))
    if n_out:
        flags[rng.choice(fpos, size=n_out, replace=False)] |= 2
    # a few features pointing at ids that are not in the map (GetLandmark -> nullptr)
    lm_ids = rng.choice(np.iinfo(np.int64).max, size=n_lm + 16, replace=False).astype(np.uint64)
    missing_ids = lm_ids[n_lm:]
    lm_ids = lm_ids[:n_lm]
    f_lm_id = np.zeros(nf, np.uint64)
    f_lm_id[fpos] = lm_ids[feat_lm]
    no_lm = np.nonzero(f_lm_idx < 0)[0]
    if no_lm.size >= 8:
        ghosts = rng.choice(no_lm, size=8, replace=False)
        flags[ghosts] = 1
        f_lm_id[ghosts] = missing_ids[:8]

    # landmark observation lists (kf_id, feature idx) — ordered by KF
    kf_ids = (np.arange(K_all, dtype=np.uint64) * 3 + 7).astype(np.uint64)
    lm_order = np.lexsort((obs_kf, obs_lm))
    o_lm = obs_lm[lm_order]
    o_kf = obs_kf[lm_order]
    # feature index of each (lm, kf) observation
    inv = np.empty(n_obs, np.int64)
    inv[order] = np.arange(n_obs)  # obs -> position in sorted feature order
    o_feat = pos_in_kf[inv[lm_order]]
    lm_obs_ptr = np.zeros(n_lm + 1, np.int64)
    lm_obs_ptr[1:] = np.cumsum(L)

    lm_bad = np.zeros(n_lm, np.uint8)
    n_bad = int(round(frac_bad * n_lm))
    if n_bad:
        lm_bad[rng.choice(n_lm, size=n_bad, replace=False)] = 1

    # ---- perturbed initial state
    dq = quat_from_rotvec(rng.normal(0, np.deg2rad(rot_deg) / np.sqrt(3), size=(K_all, 3)))
    q0 = quat_mul(dq, q_cw)
    q0 /= np.linalg.norm(q0, axis=-1, keepdims=True)
    t0 = t_cw + rng.normal(0, trans_m / np.sqrt(3), size=(K_all, 3))
    p0 = p_true + rng.normal(0, lm_sigma / np.sqrt(3), size=(n_lm, 3))

    m = BAMap()
    m["kf_id"] = kf_ids
    m["kf_pose"] = np.ascontiguousarray(np.concatenate([q0, t0], -1))
    m["kf_intr"] = np.tile(np.array(intr, np.float64), (K_all, 1))
    m["kf_has_cam"] = np.ones(K_all, np.uint8)
    m["kf_feat_ptr"] = feat_ptr
    m["feat_uv"] = np.ascontiguousarray(f_uv)
    m["feat_lm_id"] = f_lm_id
    m["feat_flags"] = flags
    m["lm_id"] = lm_ids
    m["lm_pos"] = np.ascontiguousarray(p0)
    m["lm_bad"] = lm_bad
    m["lm_obs_ptr"] = lm_obs_ptr
    m["obs_kf_id"] = kf_ids[o_kf].astype(np.uint64)
    m["obs_feat_idx"] = o_feat.astype(np.uint64)
    m["ref_kf_id"] = int(kf_ids[-1])
    m["window"] = n_kf
    return m


def ba_config(name: str):
    """(n_kf, n_lm, n_streams) of the BASELINE.json configs."""
    return {"C2": (10, 2000, 1), "C3": (50, 20000, 1), "C4": (100, 50000, 1),
            "C5": (200, 100000, 8)}[name]


def make_keyframe_pair(seed: int, n: int = 2000, *, width: int = 640, height: int = 480, intr=(FX, FY, CX, CY),
                       baseline_m: float = 0.08, yaw_deg: float = 1.5, noise_px: float = 0.3,
                       frac_has: float = 0.1, frac_bad_match: float = 0.1, frac_dup_train: float = 0.03,
                       depth_type: str = "u16"):
    """Two keyframes seeing a common set of points, for Tracking::CreateKeyFrame's landmark
    creation (tracking.cpp:577-580): per frame Feature positions and has_landmark flags, T_cw poses,
    a depth image of the second frame (TUM u16 metres * 5000, with holes and out-of-range pixels)
    and the match list Match(last, curr) would return (query = last frame, unique queries; some
    wrong / duplicated train indices).  Returns a dict of numpy arrays."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = intr
    # points in front of camera 1
    u = rng.uniform(5, width - 5, n)
    v = rng.uniform(5, height - 5, n)
    z = rng.uniform(0.6, 6.0, n)
    pc1 = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], -1)
    q1 = quat_from_rotvec(rng.normal(0, 0.02, 3))
    t1 = rng.normal(0, 0.1, 3)
    R1 = quat_to_mat(q1)
    pw = (pc1 - t1) @ R1  # R1^T (pc - t)
    q12 = quat_from_rotvec(np.array([0.0, np.deg2rad(yaw_deg), 0.0]))
    q2 = quat_mul(q12, q1)
    q2 /= np.linalg.norm(q2)
    R2 = quat_to_mat(q2)
    c1w = -R1.T @ t1
    c2w = c1w + np.array([baseline_m, 0.01, 0.005])
    t2 = -R2 @ c2w
    pc2 = pw @ R2.T + t2
    uv1 = np.stack([fx * pc1[:, 0] / pc1[:, 2] + cx, fy * pc1[:, 1] / pc1[:, 2] + cy], -1)
    uv2 = np.stack([fx * pc2[:, 0] / pc2[:, 2] + cx, fy * pc2[:, 1] / pc2[:, 2] + cy], -1)
    uv1 += rng.normal(0, noise_px, uv1.shape)
    uv2 += rng.normal(0, noise_px, uv2.shape)
    # frame 2 feature order is a permutation of frame 1's
    perm = rng.permutation(n)
    uv2 = uv2[perm]
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)  # point i is feature inv[i] of frame 2
    has1 = (rng.random(n) < frac_has).astype(np.uint8)
    has2 = (rng.random(n) < frac_has).astype(np.uint8)
    q_idx = np.sort(rng.choice(n, size=int(0.8 * n), replace=False))
    t_idx = inv[q_idx].copy()
    bad = rng.random(q_idx.size) < frac_bad_match
    t_idx[bad] = rng.integers(0, n, bad.sum())
    dup = rng.random(q_idx.size) < frac_dup_train
    dup_src = rng.integers(0, q_idx.size, dup.sum())
    t_idx[dup] = t_idx[dup_src]
    matches = np.zeros(q_idx.size, np.dtype([("query_idx", "<i4"), ("train_idx", "<i4"), ("distance", "<f4")]))
    matches["query_idx"] = q_idx
    matches["train_idx"] = t_idx
    matches["distance"] = rng.integers(0, 64, q_idx.size)
    # depth image of frame 2: smooth field, holes (0) and out-of-range pixels
    yy, xx = np.mgrid[0:height, 0:width]
    dm = 2.5 + 1.5 * np.sin(xx / 57.0) * np.cos(yy / 43.0) + 0.002 * xx
    dm[rng.random(dm.shape) < 0.05] = 0.0
    dm[rng.random(dm.shape) < 0.02] = 0.05
    dm[rng.random(dm.shape) < 0.02] = 12.0
    if depth_type == "u16":
        depth = np.round(dm * 5000.0).clip(0, 65535).astype(np.uint16)
    elif depth_type == "f32":
        depth = dm.astype(np.float32)
    else:
        depth = dm.astype(np.float64)
    pose1 = np.concatenate([q1, t1])
    pose2 = np.concatenate([q2, t2])
    return {"uv1": np.ascontiguousarray(uv1), "has1": has1, "uv2": np.ascontiguousarray(uv2), "has2": has2,
            "intr": np.array(intr, np.float64), "pose1": pose1, "pose2": pose2, "matches": matches,
            "depth": np.ascontiguousarray(depth), "pw_true": pw, "inv": inv}


def make_keyframe_scene(seed: int, n: int = 2000, *, depth_hole_frac: float = 0.5, with_depth: bool = True, **pair_kw):
    """make_keyframe_pair shaped for Tracking::CreateKeyFrame as a whole (tracking.cpp:577-584): the
    positions of both frames are float-representable (Feature::position comes from cv::KeyPoint::pt),
    the new keyframe (frame 2) arrives without links (has2 = 0), and the depth pixel of a share
    `depth_hole_frac` of its features is a hole, so that CreateLandmarksFromDepth leaves features for
    TriangulateWithLastKeyFrame (with the pair's own depth image only ~4 % of the features reach it).
    `with_depth=False`: no depth image at all (d["depth"] is None).  Otherwise the dict of
    make_keyframe_pair."""
    d = make_keyframe_pair(seed, n, **pair_kw)
    d["uv1"] = np.ascontiguousarray(d["uv1"].astype(np.float32).astype(np.float64))
    d["uv2"] = np.ascontiguousarray(d["uv2"].astype(np.float32).astype(np.float64))
    d["has2"] = np.zeros(n, np.uint8)
    if not with_depth:
        d["depth"] = None
        return d
    rng = np.random.default_rng(seed ^ 0xD0117)
    depth = d["depth"]
    px = (d["uv2"] + 0.5).astype(np.int64)  # the pixel CreateLandmarksFromDepth reads (tracking.cpp:596-597)
    inside = (px[:, 0] >= 0) & (px[:, 0] < depth.shape[1]) & (px[:, 1] >= 0) & (px[:, 1] < depth.shape[0])
    hole = inside & (rng.random(n) < depth_hole_frac)
    depth[px[hole, 1], px[hole, 0]] = 0
    return d


def _pnp_geometry(rng, n, outlier_frac, noise_px, width, height, intr, z_range):
    """World points (float64) seen at pixels uv by a camera at a random T_cw = (q | R, t), pixel noise,
    a fraction `outlier_frac` of the pixels replaced by random ones (flags in `out`)."""
    fx, fy, cx, cy = intr
    u = rng.uniform(0, width, n)
    v = rng.uniform(0, height, n)
    z = rng.uniform(z_range[0], z_range[1], n)
    pc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], -1)
    q = quat_from_rotvec(rng.normal(0, 0.3, 3))
    R = quat_to_mat(q)
    t = rng.normal(0, 0.5, 3)
    pw = (pc - t) @ R  # R^T (pc - t)
    uv = np.stack([u, v], -1) + rng.normal(0, noise_px, (n, 2))
    out = rng.random(n) < outlier_frac
    uv[out] = np.stack([rng.uniform(0, width, out.sum()), rng.uniform(0, height, out.sum())], -1)
    return pw, uv, out, q, R, t


def make_pnp_problem(seed: int, n: int = 1000, *, outlier_frac: float = 0.3, noise_px: float = 0.5,
                     width: int = 640, height: int = 480, intr=(FX, FY, CX, CY), z_range=(1.0, 6.0)):
    """3D-2D correspondences as Tracking::TrackWithPnP builds them (tracking.cpp:364-401:
    cv::Point3f landmark positions, cv::Point2f current-frame feature positions): points seen by a
    camera at a random T_cw, pixel noise, a fraction of wrong matches (random pixels).  Returns a
    dict: obj (n x 3 float32), img (n x 2 float32), intr, pose (T_cw qx qy qz qw tx ty tz),
    R, t, outlier (bool per correspondence)."""
    rng = np.random.default_rng(seed)
    pw, uv, out, q, R, t = _pnp_geometry(rng, n, outlier_frac, noise_px, width, height, intr, z_range)
    if q[3] < 0:
        q = -q
    return {"obj": pw.astype(np.float32), "img": uv.astype(np.float32), "intr": np.array(intr, np.float64),
            "pose": np.concatenate([q, t]), "R": R, "t": t, "outlier": out}


def make_track_scene(seed: int, n_feat: int = 300, *, wrong_frac: float = 0.3, noise_px: float = 0.5,
                     max_flips: int = 24, kf_shift_px: float = 6.0, width: int = 640, height: int = 480,
                     intr=(FX, FY, CX, CY), z_range=(1.0, 6.0)):
    """What Tracking::TrackWithPnP (tracking.cpp:332-455) reads, on make_pnp_problem's geometry: a last
    keyframe of n_feat features, each holding a landmark, and a current frame that sees the same
    landmarks from the true pose T_cw, its keypoints stored in a permuted order.  A fraction
    `wrong_frac` of the features is matched to a keypoint at a random pixel (a wrong match).

    Descriptors (32 bytes): the current frame's are random; keyframe feature i's is its keypoint's with
    flips[i] (0..max_flips) bits flipped, so the best Hamming distance of feature i is flips[i] and the
    second best that of an unrelated random row (about 128 - 3 * 8 at the least): the ratio test passes
    and Match(last_keyframe, curr) returns `matches` (query i, train train_of[i], distance flips[i]).

    Returns a dict: kf_uv (n x 2 float64, the keyframe's own pixels: the current ones shifted by a
    few px, so the parallax is known), lm_id (uint64), flags (uint8: has_landmark), lm_pos (n x 3
    float64, not float-representable), curr_xy (n x 2 float32, permuted), train_of (int32: the keypoint
    of feature i), desc_kf / desc_curr (n x 32 uint8), flips, matches (MATCH_DTYPE-compatible record
    array), wrong (bool), intr, pose (T_cw qx qy qz qw tx ty tz), R, t."""
    rng = np.random.default_rng(seed)
    pw, uv, wrong, q, R, t = _pnp_geometry(rng, n_feat, wrong_frac, noise_px, width, height, intr, z_range)
    if q[3] < 0:
        q = -q
    perm = rng.permutation(n_feat).astype(np.int32)
    curr_xy = np.zeros((n_feat, 2), np.float32)
    curr_xy[perm] = uv.astype(np.float32)
    kf_uv = uv + rng.normal(0, kf_shift_px, (n_feat, 2))
    desc_curr = rng.integers(0, 256, (n_feat, 32), dtype=np.uint8)
    flips = rng.integers(0, max_flips + 1, n_feat).astype(np.int32)
    bits = np.unpackbits(desc_curr[perm], axis=1)
    for i in range(n_feat):
        bits[i, rng.choice(256, flips[i], replace=False)] ^= 1
    desc_kf = np.packbits(bits, axis=1)
    matches = np.zeros(n_feat, [("query_idx", "<i4"), ("train_idx", "<i4"), ("distance", "<f4")])
    matches["query_idx"] = np.arange(n_feat)
    matches["train_idx"] = perm
    matches["distance"] = flips
    return {"kf_uv": kf_uv, "lm_id": (1000 + 7 * np.arange(n_feat)).astype(np.uint64),
            "flags": np.ones(n_feat, np.uint8), "lm_pos": pw, "curr_xy": curr_xy, "train_of": perm,
            "desc_kf": desc_kf, "desc_curr": desc_curr, "flips": flips, "matches": matches, "wrong": wrong,
            "intr": np.array(intr, np.float64), "pose": np.concatenate([q, t]), "R": R, "t": t}


def make_two_view(seed: int, n: int = 1000, *, outlier_frac: float = 0.3, noise_px: float = 0.5,
                  width: int = 640, height: int = 480, intr=(FX, FY, CX, CY), baseline_m: float = 0.15,
                  rot_deg: float = 3.0, z_range=(1.0, 6.0)):
    """Matched pixel pairs as Tracking::EstimatePoseByEssential builds them (tracking.cpp:506-514:
    cv::Point2f of the last and the current frame's features): points seen by both cameras, pixel
    noise, a fraction of wrong matches.  Returns pts_last, pts_curr (n x 2 float32), intr, the true
    T_cl (R, t with x_curr = R x_last + t; t unit-normalised copy in t_dir) and the outlier flags."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = intr
    q = quat_from_rotvec(rng.normal(0, 1, 3) * np.deg2rad(rot_deg) / np.sqrt(3))
    R = quat_to_mat(q)
    d = rng.normal(0, 1, 3)
    d[2] *= 0.3
    t = baseline_m * d / np.linalg.norm(d)
    pts_last, pts_curr = [], []
    while not pts_last or sum(len(a) for a in pts_last) < n:
        u = rng.uniform(0, width, 2 * n)
        v = rng.uniform(0, height, 2 * n)
        z = rng.uniform(z_range[0], z_range[1], 2 * n)
        p1 = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], -1)
        p2 = p1 @ R.T + t
        u2 = fx * p2[:, 0] / p2[:, 2] + cx
        v2 = fy * p2[:, 1] / p2[:, 2] + cy
        ok = (p2[:, 2] > 0.1) & (u2 >= 0) & (u2 < width) & (v2 >= 0) & (v2 < height)
        pts_last.append(np.stack([u, v], -1)[ok])
        pts_curr.append(np.stack([u2, v2], -1)[ok])
    a = np.concatenate(pts_last)[:n] + rng.normal(0, noise_px, (n, 2))
    b = np.concatenate(pts_curr)[:n] + rng.normal(0, noise_px, (n, 2))
    out = rng.random(n) < outlier_frac
    b[out] = np.stack([rng.uniform(0, width, out.sum()), rng.uniform(0, height, out.sum())], -1)
    return {"pts_last": a.astype(np.float32), "pts_curr": b.astype(np.float32), "intr": np.array(intr, np.float64),
            "R": R, "t": t, "t_dir": t / np.linalg.norm(t), "outlier": out}


def make_last_frame_scene(seed: int, n_feat: int = 300, *, wrong_frac: float = 0.3, noise_px: float = 0.5,
                          max_flips: int = 24, width: int = 640, height: int = 480, intr=(FX, FY, CX, CY),
                          baseline_m: float = 0.15, rot_deg: float = 3.0, z_range=(1.0, 6.0)):
    """What Tracking::TrackLastFrame (tracking.cpp:281-330) reads: make_two_view's geometry (points seen
    by the last and the current camera, pixel noise, a fraction `wrong_frac` of the current pixels
    replaced by random ones) with make_track_scene's descriptor construction (the current frame's
    keypoints stored in a permuted order, its descriptors random, last feature i's its keypoint's
    with flips[i] bits flipped), so Match(last, curr) returns `matches` (query i, train train_of[i],
    distance flips[i]).

    Returns a dict: last_xy, curr_xy (n x 2 float32; curr permuted), train_of (int32), desc_last /
    desc_curr (n x 32 uint8), flips, matches (MATCH_DTYPE-compatible record array), wrong (bool), intr,
    the true T_cl (R, t with x_curr = R x_last + t; t_dir = t / |t|), pose_last (a non-trivial T_lw,
    qx qy qz qw tx ty tz, qw > 0) and R_cw (the rotation of T_cl * T_lw)."""
    tv = make_two_view(seed, n_feat, outlier_frac=wrong_frac, noise_px=noise_px, width=width, height=height,
                       intr=intr, baseline_m=baseline_m, rot_deg=rot_deg, z_range=z_range)
    rng = np.random.default_rng([seed, 0x7E55])
    perm = rng.permutation(n_feat).astype(np.int32)
    curr_xy = np.zeros((n_feat, 2), np.float32)
    curr_xy[perm] = tv["pts_curr"]
    desc_curr = rng.integers(0, 256, (n_feat, 32), dtype=np.uint8)
    flips = rng.integers(0, max_flips + 1, n_feat).astype(np.int32)
    bits = np.unpackbits(desc_curr[perm], axis=1)
    for i in range(n_feat):
        bits[i, rng.choice(256, flips[i], replace=False)] ^= 1
    desc_last = np.packbits(bits, axis=1)
    matches = np.zeros(n_feat, [("query_idx", "<i4"), ("train_idx", "<i4"), ("distance", "<f4")])
    matches["query_idx"] = np.arange(n_feat)
    matches["train_idx"] = perm
    matches["distance"] = flips
    q_lw = quat_from_rotvec(rng.normal(0, 0.4, 3))
    if q_lw[3] < 0:
        q_lw = -q_lw
    pose_last = np.concatenate([q_lw, rng.normal(0, 0.7, 3)])
    return {"last_xy": tv["pts_last"], "curr_xy": curr_xy, "train_of": perm, "desc_last": desc_last,
            "desc_curr": desc_curr, "flips": flips, "matches": matches, "wrong": tv["outlier"], "intr": tv["intr"],
            "R": tv["R"], "t": tv["t"], "t_dir": tv["t_dir"], "pose_last": pose_last,
            "R_cw": tv["R"] @ quat_to_mat(q_lw)}


def make_track_frame_scene(seed: int, n_feat: int = 300, *, wrong_frac: float = 0.3, noise_px: float = 0.5,
                           max_flips: int = 24, baseline_m: float = 0.15, rot_deg: float = 3.0, **track_kw):
    """What Tracking::Track (tracking.cpp:267-279) reads: make_track_scene's last keyframe, landmarks and
    current frame, plus a LAST FRAME that sees the same landmarks from T_lw = T_cl^-1 * T_cw (T_cl a
    rotation of about rot_deg and a baseline of baseline_m), with make_last_frame_scene's descriptor
    construction: last feature i's descriptor is the current keypoint train_of[i]'s with flips_last[i]
    bits flipped, so Match(last, curr) returns `matches_last` (query i, train train_of[i]).  The current
    pixels of the `wrong` features are random, so they are outliers of both paths (wrong_frac = 1.0:
    both fail); whether PnP passes is the caller's to steer (flags, min_matches, min_inliers).

    Returns make_track_scene's dict plus last_xy (n x 2 float32), desc_last, flips_last, matches_last,
    pose_last (T_lw: qx qy qz qw tx ty tz, qw > 0), R_cl, t_cl."""
    s = make_track_scene(seed, n_feat, wrong_frac=wrong_frac, noise_px=noise_px, max_flips=max_flips, **track_kw)
    rng = np.random.default_rng([seed, 0x7F2A])
    fx, fy, cx, cy = s["intr"]
    q_cl = quat_from_rotvec(rng.normal(0, 1, 3) * np.deg2rad(rot_deg) / np.sqrt(3))
    R_cl = quat_to_mat(q_cl)
    d = rng.normal(0, 1, 3)
    d[2] *= 0.3
    t_cl = baseline_m * d / np.linalg.norm(d)
    R_lw = R_cl.T @ s["R"]
    t_lw = R_cl.T @ (s["t"] - t_cl)
    pl = s["lm_pos"] @ R_lw.T + t_lw
    last_xy = np.stack([fx * pl[:, 0] / pl[:, 2] + cx, fy * pl[:, 1] / pl[:, 2] + cy], -1) + rng.normal(0, noise_px, (n_feat, 2))
    perm = s["train_of"]
    flips = rng.integers(0, max_flips + 1, n_feat).astype(np.int32)
    bits = np.unpackbits(s["desc_curr"][perm], axis=1)
    for i in range(n_feat):
        bits[i, rng.choice(256, flips[i], replace=False)] ^= 1
    matches = np.zeros(n_feat, [("query_idx", "<i4"), ("train_idx", "<i4"), ("distance", "<f4")])
    matches["query_idx"] = np.arange(n_feat)
    matches["train_idx"] = perm
    matches["distance"] = flips
    # R -> quaternion through the rotation vector of R_lw's own quaternion product (qw > 0)
    q_cw = s["pose"][:4]
    q_lw = quat_mul(np.array([-q_cl[0], -q_cl[1], -q_cl[2], q_cl[3]]), q_cw)
    if q_lw[3] < 0:
        q_lw = -q_lw
    return dict(s, last_xy=last_xy.astype(np.float32), desc_last=np.packbits(bits, axis=1), flips_last=flips,
                matches_last=matches, pose_last=np.concatenate([q_lw, t_lw]), R_cl=R_cl, t_cl=t_cl)


def make_sequence(seed: int, n_frames: int = 14, n_pts: int = 350, *, width: int = 640, height: int = 480,
                  intr=(FX, FY, CX, CY), step_m: float = 1.0, yaw_deg: float = 0.25, z_range=(5.0, 9.5),
                  depth_share: float = 0.5, noise_px: float = 0.3, max_flips: int = 10, garbage=(), dark=()):
    """What Tracking::ProcessFrame (tracking.cpp:39-89) reads frame after frame: world points seen by a
    camera that moves along a straight line with a slowly growing yaw, about `n_pts` of them in view of
    every frame.

    The camera centres are exactly `step_m` apart.  The default is 1: InitWithSecondFrame takes the
    unit translation recoverPose returns (:528-541) while CreateLandmarksFromDepth places points at
    their metric depth (:626-640), so the two only agree in a world whose first baseline is 1 (the
    TrackLastFrame fallback composes unit steps in the same way).  With fx = 520 and z in `z_range`
    that is a displacement of 55-105 px a frame.

    Per frame i (frames[i], a dict): xy (n_i x 2 float32: true projection + noise, in a permuted order),
    desc (n_i x 32 uint8: the point's base row with up to `max_flips` bits flipped, make_track_scene's
    construction, so two views of a point are at most 2 * max_flips apart and unrelated rows about
    128), point (int64: the world point behind each feature), depth (height x width uint16:
    round(z * 5000) at the pixel CreateLandmarksFromDepth reads, (int)(x + 0.5), (int)(y + 0.5), for a
    share `depth_share` of the features, 0 elsewhere and where two features share a pixel), img
    (height x width x 3 uint8, a make_frames frame: it passes the quality gate), pose (true T_cw, qx
    qy qz qw tx ty tz, relative to frame 0).
    `garbage`: frames whose positions and descriptors are replaced by random ones (nothing matches);
    `dark`: frames whose image is all zero (only InitWithFirstFrame looks at the image).
    Returns {"frames", "intr", "width", "height", "points"}."""
    rng = np.random.default_rng([seed, 0x5E0])
    fx, fy, cx, cy = intr
    z0, z1 = z_range
    d = np.array([0.99, 0.04, 0.08])
    d /= np.linalg.norm(d)
    centres = np.arange(n_frames)[:, None] * step_m * d[None, :]
    # a slab that covers every frame's frustum, thinned until about n_pts points are in view of a frame
    x_lo, x_hi = -cx / fx * z1 - 1.0, centres[-1, 0] + (width - cx) / fx * z1 + 1.0
    cand = int(np.ceil(3 * n_pts * (x_hi - x_lo) * fx / (width * z0)))
    z = rng.uniform(z0, z1 + centres[-1, 2], cand)
    pts = np.stack([rng.uniform(x_lo, x_hi, cand),
                    (rng.uniform(-20, height + 20, cand) - cy) / fy * z + rng.uniform(0, 1, cand) * centres[-1, 1], z], -1)
    seen = 0
    for c in centres:  # (the yaw is small: the unrotated frustum is close enough for a count)
        pc = pts - c
        u, v = fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy
        seen += np.count_nonzero((pc[:, 2] < 9.9) & (u >= 2) & (u < width - 2) & (v >= 2) & (v < height - 2))
    total = min(cand, int(round(cand * n_pts * n_frames / max(seen, 1))))
    pts = pts[:total]
    base = rng.integers(0, 256, (total, 32), dtype=np.uint8)
    imgs = make_frames(seed, n_frames, height, width)
    frames = []
    for i in range(n_frames):
        q = quat_from_rotvec(np.array([0.0, np.deg2rad(yaw_deg) * i, 0.002 * i]))
        R = quat_to_mat(q)
        t = -R @ centres[i]
        pc = pts @ R.T + t
        with np.errstate(divide="ignore", invalid="ignore"):
            uv = np.stack([fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy], -1)
        uv = uv + rng.normal(0, noise_px, uv.shape)
        vis = np.flatnonzero((pc[:, 2] > 0.5) & (pc[:, 2] < 9.9) & (uv[:, 0] >= 2) & (uv[:, 0] < width - 2) &
                             (uv[:, 1] >= 2) & (uv[:, 1] < height - 2))
        vis = vis[rng.permutation(len(vis))]
        xy = uv[vis].astype(np.float32)
        bits = np.unpackbits(base[vis], axis=1)
        for k in range(len(vis)):
            bits[k, rng.choice(256, rng.integers(0, max_flips + 1), replace=False)] ^= 1
        desc = np.packbits(bits, axis=1)
        img = imgs[i].copy()
        if i in garbage:
            xy = np.stack([rng.uniform(2, width - 2, len(vis)), rng.uniform(2, height - 2, len(vis))], -1).astype(np.float32)
            desc = rng.integers(0, 256, (len(vis), 32), dtype=np.uint8)
        if i in dark:
            img[:] = 0
        depth = np.zeros((height, width), np.uint16)
        px = (xy.astype(np.float64) + 0.5).astype(np.int64)
        flat = px[:, 1] * width + px[:, 0]
        _, first, count = np.unique(flat, return_index=True, return_counts=True)
        alone = np.zeros(len(vis), bool)
        alone[first[count == 1]] = True
        has = alone & (rng.random(len(vis)) < depth_share)
        depth[px[has, 1], px[has, 0]] = np.round(pc[vis[has], 2] * 5000.0).astype(np.uint16)
        if q[3] < 0:
            q = -q
        frames.append({"xy": np.ascontiguousarray(xy), "desc": np.ascontiguousarray(desc), "point": vis, "depth": depth,
                       "img": img, "pose": np.concatenate([q, t])})
    return {"frames": frames, "intr": np.array(intr, np.float64), "width": width, "height": height, "points": pts}


# --------------------------------------------------------------------------- map culling
def _project_rows(m, lm_rows, kf_rows):
    """camera-frame points and pixels of landmark rows seen from keyframe rows (R from the quaternion
    as Eigen's toRotationMatrix, pc = R p + t, common/projection.h:16-25)"""
    pose = m["kf_pose"].reshape(-1, 7)[kf_rows]
    R = quat_to_mat(pose[:, :4])
    pc = np.einsum("oij,oj->oi", R, m["lm_pos"].reshape(-1, 3)[lm_rows]) + pose[:, 4:]
    intr = m["kf_intr"].reshape(-1, 4)[kf_rows]
    with np.errstate(divide="ignore", invalid="ignore"):
        uv = np.stack([intr[:, 0] * (pc[:, 0] / pc[:, 2]) + intr[:, 2], intr[:, 1] * (pc[:, 1] / pc[:, 2]) + intr[:, 3]], -1)
    return pc, uv


def cull_state(m):
    """The membership state Tracking's culling changes, added to a BAMap in place when absent:
    kf_alive (0 after Map::RemoveKeyFrame; a later row may hold the id again), lm_removed (1 after
    Map::RemoveLandmark), obs_live (0 after Landmark::RemoveObservation).  Rows are storage rows."""
    m.setdefault("kf_alive", np.ones(len(m["kf_id"]), np.uint8))
    m.setdefault("lm_removed", np.zeros(len(m["lm_id"]), np.uint8))
    m.setdefault("obs_live", np.ones(len(m["obs_kf_id"]), np.uint8))
    return m


def cull_margins(m, tau=5.0):
    """How far the map is from each threshold Tracking::CullLandmarks compares against
    (tracking.cpp:652-750), as relative distances over every observation the walk can project:
    {"err": min |err - 2 tau| / 2 tau, "mean": min |mean - tau| / tau over the landmarks without a
    large error, "z": min |pc.z - 1e-6| / 1e-6}.  A decision made in another rounding order is the same
    decision while these stay far above that order's error."""
    cull_state(m)
    optr = m["lm_obs_ptr"]
    lm = np.repeat(np.arange(len(m["lm_id"])), np.diff(optr))
    alive = np.nonzero(m["kf_alive"])[0]
    row_of = {int(m["kf_id"][k]): int(k) for k in alive}
    kf = np.array([row_of.get(int(i), -1) for i in m["obs_kf_id"]], np.int64)
    fi = m["obs_feat_idx"].astype(np.int64)
    nf = np.diff(m["kf_feat_ptr"])
    ok = (m["obs_live"] > 0) & (m["lm_removed"][lm] == 0) & (m["lm_bad"][lm] == 0) & (kf >= 0)
    ok &= (fi >= 0) & (fi < nf[np.maximum(kf, 0)])
    g = m["kf_feat_ptr"][np.maximum(kf, 0)] + np.where(ok, fi, 0)
    ok &= ((m["feat_flags"][g] & 1) > 0) & (m["feat_lm_id"][g] == m["lm_id"][lm]) & (m["kf_has_cam"][np.maximum(kf, 0)] > 0)
    sel = np.nonzero(ok)[0]
    out = {"err": np.inf, "mean": np.inf, "z": np.inf}
    if not len(sel):
        return out
    pc, uv = _project_rows(m, lm[sel], kf[sel])
    out["z"] = float((np.abs(pc[:, 2] - 1e-6) / 1e-6).min())
    front = pc[:, 2] > 1e-6
    err = np.hypot(*(m["feat_uv"].reshape(-1, 2)[g[sel][front]] - uv[front]).T)
    if len(err):
        out["err"] = float((np.abs(err - 2 * tau) / (2 * tau)).min())
        rows = lm[sel][front]
        s = np.bincount(rows, err, len(m["lm_id"]))
        c = np.bincount(rows, minlength=len(m["lm_id"]))
        large = np.bincount(rows, err > 2 * tau, len(m["lm_id"])) > 0
        use = (c > 0) & ~large
        if use.any():
            out["mean"] = float((np.abs(s[use] / c[use] - tau) / tau).min())
    return out


def make_cull_scene(seed: int, n_kf: int = 10, n_lm: int = 2000, *, special: bool = True, tau: float = 5.0,
                    min_margin: float = 1e-9, **ba_kw) -> BAMap:
    """A map for Tracking::CullLandmarks / CullKeyFrames (tracking.cpp:652-840): make_ba_map (bad
    landmarks, single-observation landmarks, features naming ids that are not in the map; the larger
    `lm_sigma`, the more reprojection culls) with the membership state of cull_state, plus — with
    `special` — hand-placed keyframes and landmarks that each reach one branch of the walk:

      keyframes   S0, S1 (ordinary), D (removed from the map), Y (id removed and inserted again: a dead
                  row and a live one), C (no camera), B (looks away: points lie behind it), Z (no
                  feature holds a landmark), W0..W69 (one feature each)
      landmarks   (name -> row in m["special"]) dead_kf: one observation names D (still counts towards
                  ObservationCount); reinserted / reinserted_bad: observed through Y's live row (small /
                  large error there, garbage in the dead row); oor / oor_cull: a feature index past the
                  keyframe's features; other / other_cull: the feature points at another landmark;
                  nohas_keep / nohas_cull: the feature carries the id without has_landmark (skipped by
                  the walk, reset by the removal); behind: pc.z < 0 in B; nocam: observed by C;
                  wave_cull / wave_keep: 70 observations (W0..W69), the only large error the last /
                  none; all_skipped / all_skipped_reset: every observation skipped (NO_PROJECTION; the
                  second one's features are still reset); mean: errors 4 and 8; removed: a removed
                  landmark that features of S0 and S1 still name.

    Asserts cull_margins(m, tau) > min_margin on all three."""
    m = cull_state(make_ba_map(seed, n_kf, n_lm, **ba_kw))
    if special:
        _add_cull_specials(m, np.random.default_rng(seed ^ 0xC0117))
    mg = cull_margins(m, tau)
    assert min(mg.values()) > min_margin, mg
    m["margins"] = mg
    return m


def _add_cull_specials(m, rng):
    base_pose = m["kf_pose"].reshape(-1, 7)
    nb = len(base_pose)
    intr = m["kf_intr"].reshape(-1, 4)[0]
    kfs, lms = [], []  # [id, pose, has_cam, alive, feats [(uv, lm_id, flags)]], [id, pos, bad, removed, obs [(kf_id, fi)]]

    def new_kf(kid, pose, cam=1, alive=1):
        kfs.append([kid, np.array(pose, np.float64), cam, alive, []])
        return len(kfs) - 1

    def feat(k, uv, lm_id, flags=1):
        kfs[k][4].append((np.array(uv, np.float64), int(lm_id), flags))
        return len(kfs[k][4]) - 1

    def proj(k, p):
        q, t = kfs[k][1][:4], kfs[k][1][4:]
        pc = quat_to_mat(q) @ p + t
        return np.array([intr[0] * (pc[0] / pc[2]) + intr[2], intr[1] * (pc[1] / pc[2]) + intr[3]])

    ids = iter(range(9_000_001, 9_100_000))
    names = {}

    def new_lm(name, bad=0, removed=0):
        p = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2), rng.uniform(2.5, 4.0)])
        lms.append([next(ids), p, bad, removed, []])
        names[name] = len(lms) - 1
        return len(lms) - 1

    def see(l, k, err=1.0, flags=1, lm_id=None, uv=None):
        """landmark l observed by keyframe k through a new feature `err` px (a 3-4-5 offset) off its projection"""
        if uv is None:
            uv = proj(k, lms[l][1]) + np.array([0.6, 0.8]) * err
        fi = feat(k, uv, lms[l][0] if lm_id is None else lm_id, flags)
        lms[l][4].append((kfs[k][0], fi))
        return fi

    S0 = new_kf(1000, base_pose[0])
    S1 = new_kf(1001, base_pose[min(1, nb - 1)])
    D = new_kf(1002, base_pose[0], alive=0)
    Y1 = new_kf(1003, base_pose[0], alive=0)
    C = new_kf(1004, base_pose[0], cam=0)
    flip = quat_mul(np.array([0.0, 1.0, 0.0, 0.0]), base_pose[0][:4])  # half a turn about y
    B = new_kf(1005, np.concatenate([flip, quat_to_mat(np.array([0.0, 1.0, 0.0, 0.0])) @ base_pose[0][4:]]))
    Z = new_kf(1006, base_pose[0])
    W = [new_kf(2000 + i, base_pose[i % nb]) for i in range(70)]
    Y2 = new_kf(1003, base_pose[min(1, nb - 1)])  # the id again: a later row
    for _ in range(3):
        feat(Z, rng.uniform(0, 400, 2), 0, 0)
        feat(Y1, rng.uniform(0, 400, 2), 0, 0)  # so that Y2's feature indices differ from Y1's... (Y1 holds more)

    l = new_lm("dead_kf")
    see(l, S0), see(l, D)
    for name, e in (("reinserted", 1.0), ("reinserted_bad", 30.0)):
        l = new_lm(name)
        see(l, S0)
        fi = see(l, Y2, err=e)
        while len(kfs[Y1][4]) <= fi:  # the dead row holds a feature at that index too, far off
            feat(Y1, [5000.0, 5000.0], lms[l][0], 1)
        kfs[Y1][4][fi] = (np.array([5000.0, 5000.0]), lms[l][0], 1)
    for name, e in (("oor", 1.0), ("oor_cull", 30.0)):
        l = new_lm(name)
        see(l, S0, err=e)
        lms[l][4].append((kfs[S1][0], 100_000))
    for name, e in (("other", 1.0), ("other_cull", 30.0)):
        l = new_lm(name)
        see(l, S0, err=e)
        see(l, S1, err=30.0 if e == 1.0 else 1.0, lm_id=lms[names["oor"]][0])
    l = new_lm("nohas_keep")
    see(l, S0), see(l, S1, err=30.0, flags=0)
    l = new_lm("nohas_cull")
    see(l, S0, err=30.0), see(l, S1, flags=0)
    l = new_lm("behind")
    see(l, S0), see(l, B, uv=[100.0, 100.0])
    l = new_lm("nocam")
    see(l, S0), see(l, C, uv=[100.0, 100.0])
    l = new_lm("wave_cull")
    for i, k in enumerate(W):
        see(l, k, err=30.0 if i == 69 else 0.5 + 0.01 * i)
    l = new_lm("wave_keep")
    for i, k in enumerate(W):
        see(l, k, err=0.5 + 0.01 * i)
    l = new_lm("all_skipped")
    see(l, D), lms[l][4].append((kfs[S1][0], 100_001))
    l = new_lm("all_skipped_reset")
    see(l, C, uv=[50.0, 60.0]), see(l, S1, flags=0)
    l = new_lm("mean")
    see(l, S0, err=4.0), see(l, S1, err=8.0)
    l = new_lm("removed", removed=1)
    see(l, S0), see(l, S1)
    assert len(kfs[Y1][4]) != len(kfs[Y2][4])

    # ---- append to the map's arrays (storage rows: keyframes then landmarks, in creation order)
    k0 = len(m["kf_id"])
    m["kf_id"] = np.concatenate([m["kf_id"], np.array([k[0] for k in kfs], np.uint64)])
    m["kf_pose"] = np.concatenate([m["kf_pose"].reshape(-1, 7), np.stack([k[1] for k in kfs])])
    m["kf_intr"] = np.concatenate([m["kf_intr"].reshape(-1, 4), np.tile(intr, (len(kfs), 1))])
    m["kf_has_cam"] = np.concatenate([m["kf_has_cam"], np.array([k[2] for k in kfs], np.uint8)])
    m["kf_alive"] = np.concatenate([m["kf_alive"], np.array([k[3] for k in kfs], np.uint8)])
    cnt = np.array([len(k[4]) for k in kfs], np.int64)
    m["kf_feat_ptr"] = np.concatenate([m["kf_feat_ptr"], m["kf_feat_ptr"][-1] + np.cumsum(cnt)]).astype(np.int64)
    fl = [f for k in kfs for f in k[4]]
    m["feat_uv"] = np.concatenate([m["feat_uv"].reshape(-1, 2), np.stack([f[0] for f in fl])])
    m["feat_lm_id"] = np.concatenate([m["feat_lm_id"], np.array([f[1] for f in fl], np.uint64)])
    m["feat_flags"] = np.concatenate([m["feat_flags"], np.array([f[2] for f in fl], np.uint8)])
    l0 = len(m["lm_id"])
    m["lm_id"] = np.concatenate([m["lm_id"], np.array([x[0] for x in lms], np.uint64)])
    m["lm_pos"] = np.concatenate([m["lm_pos"].reshape(-1, 3), np.stack([x[1] for x in lms])])
    m["lm_bad"] = np.concatenate([m["lm_bad"], np.array([x[2] for x in lms], np.uint8)])
    m["lm_removed"] = np.concatenate([m["lm_removed"], np.array([x[3] for x in lms], np.uint8)])
    ocnt = np.array([len(x[4]) for x in lms], np.int64)
    m["lm_obs_ptr"] = np.concatenate([m["lm_obs_ptr"], m["lm_obs_ptr"][-1] + np.cumsum(ocnt)]).astype(np.int64)
    ol = [o for x in lms for o in x[4]]
    m["obs_kf_id"] = np.concatenate([m["obs_kf_id"], np.array([o[0] for o in ol], np.uint64)])
    m["obs_feat_idx"] = np.concatenate([m["obs_feat_idx"], np.array([o[1] for o in ol], np.uint64)])
    m["obs_live"] = np.concatenate([m["obs_live"], np.ones(len(ol), np.uint8)])
    m["special"] = {n: l0 + r for n, r in names.items()}
    m["special_kf"] = {"S0": k0 + S0, "S1": k0 + S1, "D": k0 + D, "Y_dead": k0 + Y1, "Y": k0 + Y2, "C": k0 + C,
                       "B": k0 + B, "Z": k0 + Z, "W": [k0 + w for w in W]}
