"""numpy restatement of Tracking::InitWithFirstFrame's gates (core/frontend/tracking.cpp:93-139, :177-204)
as vx_init_gate_* computes them (csrc/init_gate.hip), and a pure-Python restatement of the tracking
state machine (ProcessFrame :39-89, UpdateTrackingState / HandleTracking* :459-499, NeedNewKeyFrame
:562-575) fed per-frame outcomes.  Pinned by tests/test_init_gate_cpu.py."""
import numpy as np

INIT_OK, INIT_FEW_FEATURES, INIT_POOR_DISTRIBUTION, INIT_POOR_IMAGE = range(4)

RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_features", "<i4"), ("valid_grids", "<i4"), ("grid_mask", "<u4"),
                         ("n_pixels", "<i8"), ("sum", "<u8"), ("sum_sq", "<u8"), ("mean", "<f8"), ("stddev", "<f8")])

DEFAULTS = dict(min_features=50, grid_cols=5, grid_rows=5, min_grid_frac=0.5, min_mean=30.0, max_mean=225.0,
                min_stddev=20.0)


def gray(img):
    """cvtColor BGR2GRAY in OpenCV's fixed point (B 1868, G 9617, R 4899, + 2^13, >> 14) on the first
    three channels; a 2-D (or 1-channel) image is its own gray level"""
    img = np.asarray(img)
    assert img.dtype == np.uint8
    if img.ndim == 2:
        return img
    if img.shape[2] == 1:
        return img[:, :, 0]
    assert img.shape[2] in (3, 4)
    c = img.astype(np.int64)
    return ((c[:, :, 0] * 1868 + c[:, :, 1] * 9617 + c[:, :, 2] * 4899 + (1 << 13)) >> 14).astype(np.uint8)


def sums(g):
    """(N, sum, sum of squares) of a gray image as Python integers"""
    g = np.asarray(g).astype(np.uint64)
    return int(g.size), int(g.sum(dtype=np.uint64)), int((g * g).sum(dtype=np.uint64))


def mean_stddev(n, s, q):
    """meanStdDev's arithmetic: scale = 1.0 / N, mean = sum * scale, sqrt(max(sum_sq * scale - mean *
    mean, 0)); every operation an IEEE double operation rounded on its own (numpy scalars: no fusing)"""
    scale = np.float64(1.0) / np.float64(n)
    mean = np.float64(s) * scale
    var = np.float64(q) * scale - mean * mean
    return float(mean), float(np.sqrt(max(var, np.float64(0.0))))


def grid_cells(xy, width, height, cols=5, rows=5):
    """(col, row) per keypoint as tracking.cpp:101-104: (int)((x / width) * cols) in double, truncation
    toward zero, clamped"""
    xy = np.asarray(xy, np.float32).reshape(-1, 2).astype(np.float64)
    col = np.trunc((xy[:, 0] / np.float64(width)) * np.float64(cols)).astype(np.int64)
    row = np.trunc((xy[:, 1] / np.float64(height)) * np.float64(rows)).astype(np.int64)
    return np.clip(col, 0, cols - 1), np.clip(row, 0, rows - 1)


def init_gate_ref(img, xy, **opt):
    """the whole vx_init_gate_result record (RESULT_DTYPE) for an image (H x W or H x W x C uint8) and
    float positions (n x 2)"""
    o = dict(DEFAULTS, **opt)
    g = gray(img)
    h, w = g.shape
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    cols, rows = o["grid_cols"], o["grid_rows"]
    col, row = grid_cells(xy, w, h, cols, rows)
    mask = 0
    for b in np.unique(col * rows + row):
        mask |= 1 << int(b)
    valid = bin(mask).count("1")
    n, s, q = sums(g)
    mean, std = mean_stddev(n, s, q)
    if len(xy) < o["min_features"]:
        status = INIT_FEW_FEATURES
    elif valid < np.float64(cols * rows) * np.float64(o["min_grid_frac"]):
        status = INIT_POOR_DISTRIBUTION
    elif mean < o["min_mean"] or mean > o["max_mean"] or std < o["min_stddev"]:
        status = INIT_POOR_IMAGE
    else:
        status = INIT_OK
    r = np.zeros((), RESULT_DTYPE)
    r["status"], r["n_features"], r["valid_grids"], r["grid_mask"] = status, len(xy), valid, mask
    r["n_pixels"], r["sum"], r["sum_sq"], r["mean"], r["stddev"] = n, s, q, mean, std
    return r


# ---------------------------------------------------------------------------- the state machine
INIT, TRACKING_GOOD, TRACKING_BAD, LOST = range(4)

SM_DEFAULTS = dict(min_inliers=30, min_keyframe_inliers=50, min_parallax=10.0, min_keyframe_gap=3)


class StateMachine:
    """Tracking's state and the members the state functions touch, without any geometry.  step() takes
    the frame id and the outcome of the one geometric call ProcessFrame makes in the current state:

      INIT, no init frame   {"gate": bool}                                     InitWithFirstFrame (:47)
      INIT, init frame      {"init": bool, "inliers": int, "parallax": float}  InitWithSecondFrame (:54)
      TRACKING_GOOD         {"track": bool, "inliers": int, "parallax": float} Track (:64)
      TRACKING_BAD / LOST   nothing is read                                    HandleTrackingBad / Lost

    inliers / parallax are read on success only (a failed call leaves last_inliers_ / last_parallax_
    as they were).  Returns (state after the frame, whether a keyframe was created)."""

    def __init__(self, **opt):
        self.o = dict(SM_DEFAULTS, **opt)
        self.state = INIT
        self.init_frame = self.last_frame = self.last_keyframe = None
        self.last_inliers, self.last_parallax = 0, 0.0
        self.resets = 0

    def _update(self):  # UpdateTrackingState (:459-465)
        self.state = TRACKING_GOOD if self.last_inliers >= self.o["min_inliers"] else TRACKING_BAD

    def _reset(self):  # HandleTrackingBad / HandleTrackingLost (:477-499)
        self.state = INIT
        self.init_frame = self.last_frame = self.last_keyframe = None
        self.last_inliers, self.last_parallax = 0, 0.0
        self.resets += 1

    def _need_keyframe(self, fid):  # NeedNewKeyFrame (:562-575)
        if self.state != TRACKING_GOOD or self.last_keyframe is None:
            return False
        if self.last_inliers < self.o["min_keyframe_inliers"]:
            return False
        if self.last_parallax < self.o["min_parallax"]:
            return False
        return fid - self.last_keyframe >= self.o["min_keyframe_gap"]

    def step(self, fid, out):
        just_initialized = False
        if self.state == INIT:
            if self.init_frame is None:
                if out["gate"]:
                    self.init_frame = fid
                return self.state, False
            if not out["init"]:
                return self.state, False
            self.last_keyframe = fid
            self.last_inliers, self.last_parallax = out["inliers"], out["parallax"]
            self._update()
            self.last_frame = fid
            just_initialized = True
        elif self.state == TRACKING_GOOD:
            if not out["track"]:
                self.state = TRACKING_BAD  # HandleTrackingFailure from TRACKING_GOOD (:468-469)
                return self.state, False
            self.last_inliers, self.last_parallax = out["inliers"], out["parallax"]
        else:  # TRACKING_BAD, LOST
            self._reset()
            return self.state, False
        created = False
        if not just_initialized and self._need_keyframe(fid):
            self.last_keyframe = fid
            created = True
        self._update()
        self.last_frame = fid
        return self.state, created
