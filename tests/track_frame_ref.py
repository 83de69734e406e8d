"""The decision of Tracking::Track (tracking.cpp:267-279) restated over the two paths' outcome records:
which path runs, which one sets the pose, and what vx_track_frame_fetch's head reports.  Composes the
records tests/track_ref.py (TrackWithPnP) and tests/track_ess_ref.py (TrackLastFrame) describe; the
reference of tests/test_gpu_track_frame.py, pinned by tests/test_track_frame_cpu.py."""
import numpy as np

import vxslam

OK, FEW_MATCHES, FEW_PAIRS, PNP_FAILED, BAD_ROTATION, ESSENTIAL_FAILED = 0, 1, 2, 3, 4, 5
PATH_NONE, PATH_PNP, PATH_ESSENTIAL = 0, 1, 2


def pnp_status(rec, min_matches, min_inliers):
    """the return statements of Tracking::TrackWithPnP in their order (tracking.cpp:357, :402, :425, :441)"""
    if rec["n_good_matches"] < min_matches:
        return FEW_MATCHES
    if rec["n_pairs"] < min_inliers:
        return FEW_PAIRS
    if not rec["pnp"]["ok"] or rec["pnp"]["n_inliers"] < min_inliers:
        return PNP_FAILED
    if not np.isfinite(rec["pnp"]["pose"]).all():
        return BAD_ROTATION
    return OK


def ess_status(rec, min_matches, min_inliers):
    """the return statements of Tracking::TrackLastFrame (tracking.cpp:306, :317)"""
    if rec["n_good_matches"] < min_matches:
        return FEW_MATCHES
    if not rec["ess"]["ok"] or rec["ess"]["n_inliers"] < min_inliers:
        return ESSENTIAL_FAILED
    return OK


def empty_ess_record(min_matches):
    """the counts vx_track_essential_fetch returns on an empty match list (the RANSAC record: zeros here; the
    GPU test embeds the fetched one)"""
    r = np.zeros((), vxslam.TRACK_ESS_RESULT_DTYPE)
    r["min_distance"] = 100.0
    r["status"] = ess_status(r, min_matches, 0)
    return r


def track_frame_ref(pnp, ess, pnp_opt, ess_opt, n_keypoints=0, empty_ess=None):
    """pnp: the TRACK_RESULT_DTYPE record of TrackWithPnP on (last keyframe, current), None without a last
    keyframe (:269).  ess: the TRACK_ESS_RESULT_DTYPE record TrackLastFrame on (last frame, current)
    WOULD give, None without a last frame (:282).  The status fields of the inputs are ignored: they
    are evaluated here.  empty_ess: the record to embed when the fallback does not run (default: zeros
    but min_distance = 100, as the kernels leave it).  Returns a TRACK_FRAME_RESULT_DTYPE record."""
    out = np.zeros((), vxslam.TRACK_FRAME_RESULT_DTYPE)
    out["n_keypoints"] = n_keypoints
    pnp_st = OK
    if pnp is not None:
        pnp_st = pnp_status(pnp, pnp_opt["min_matches"], pnp_opt["min_inliers"])
        out["pnp_ran"] = 1
        out["pnp"] = pnp
        out["pnp"]["status"] = pnp_st
    gate_open = pnp is None or pnp_st != OK
    out["ess_ran"] = int(gate_open and ess is not None)
    if out["ess_ran"]:
        out["ess"] = ess
    else:
        out["ess"] = empty_ess if empty_ess is not None else empty_ess_record(0)
    ess_st = ess_status(out["ess"], ess_opt["min_matches"], ess_opt["min_inliers"])
    out["ess"]["status"] = ess_st
    if pnp is not None and pnp_st == OK:
        out["path"], out["status"] = PATH_PNP, OK
        out["n_inliers"], out["parallax"], out["pose"] = pnp["pnp"]["n_inliers"], pnp["parallax"], pnp["pnp"]["pose"]
    elif out["ess_ran"]:
        out["status"] = ess_st
        if ess_st == OK:
            out["path"] = PATH_ESSENTIAL
            out["n_inliers"], out["parallax"], out["pose"] = ess["ess"]["n_inliers"], ess["parallax"], ess["pose"]
    else:
        out["status"] = pnp_st
    return out
