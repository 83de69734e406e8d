"""vx_frame_* and vx_track_frame_* (csrc/frame.hip, csrc/track_frame.hip) without a GPU: the
declarations, exports and record layouts; the decision table of Tracking::Track (tracking.cpp:267-279)
restated in tests/track_frame_ref.py, over hand-made outcome records; and the status rules' boundaries on
BOTH statements of them: the shared C++ one (csrc/track_common.hpp, what vx_track_pnp_fetch,
vx_track_essential_fetch, k_track_gate and k_track_final evaluate; run on the host through
build/track_status_check) and the numpy one the GPU tests compose."""
import os
import re
import subprocess

import numpy as np
import pytest

import vxslam
from vxslam import synth

import track_frame_ref as R
from track_frame_ref import track_frame_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "visionx-slam_amd", "build", "track_status_check")
NAMES = ["vx_frame_create", "vx_frame_destroy", "vx_frame_capture_async", "vx_frame_extract_host_async",
         "vx_frame_upload_async", "vx_frame_device", "vx_frame_fetch", "vx_frame_fetch_ex", "vx_track_frame_async",
         "vx_track_frame_fetch", "vx_track_frame_pairs", "vx_track_frame_matches"]
MM, MI = 50, 30
POSE = np.array([0.1, -0.2, 0.3, 0.9, 1.0, 2.0, 3.0])


# ---------------------------------------------------------------------------- the C surface
def test_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "vx_slam.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", vxslam.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert re.search(r" T %s$" % n, out, flags=re.M), n
        assert n in vxslam.EXPORTS, n
        assert hasattr(vxslam.lib(), n), n
    assert re.search(r"\}\s*vx_track_frame_result;", hdr) and re.search(r"typedef struct vx_frame vx_frame;", hdr)
    for k, name in enumerate(("NONE", "PNP", "ESSENTIAL")):
        assert re.search(r"#define\s+VX_TRACK_PATH_%s\s+%d\b" % (name, k), hdr)
    assert (vxslam.TRACK_PATH_NONE, vxslam.TRACK_PATH_PNP, vxslam.TRACK_PATH_ESSENTIAL) == (0, 1, 2)
    for n in ("capture", "extract_host", "upload", "device", "fetch"):
        assert hasattr(vxslam.Frame, n), n
    for n in ("track_frame_async", "track_frame_fetch", "track_frame_matches"):
        assert hasattr(vxslam.Context, n), n
    assert hasattr(vxslam, "track_frame_options")


def test_record_sizes_match_the_c_structs():
    src = open(os.path.join(ROOT, "visionx-slam_amd", "csrc", "track_frame.hip")).read()
    size = int(re.search(r"static_assert\(sizeof\(vx_track_frame_result\) == (\d+)", src).group(1))
    T = vxslam.TRACK_FRAME_RESULT_DTYPE
    assert size == T.itemsize == 552
    end = 0
    for name in T.names:  # no implicit padding
        dt, off = T.fields[name][:2]
        assert off == end, name
        end = off + dt.itemsize
    assert end == T.itemsize
    assert [T.fields[k][1] for k in ("parallax", "pose", "pnp_ran", "pnp", "ess")] == [16, 24, 80, 88, 264]
    for k, v in (("parallax", 16), ("pose", 24), ("pnp_ran", 80), ("pnp", 88), ("ess", 264)):
        assert re.search(r"offsetof\(vx_track_frame_result, %s\) == %d\b" % (k, v), src), k
    assert T.fields["pnp"][0] == vxslam.TRACK_RESULT_DTYPE and T.fields["ess"][0] == vxslam.TRACK_ESS_RESULT_DTYPE
    assert vxslam.KEYPOINT_DTYPE.itemsize == 20
    assert vxslam.TRACK_RESULT_DTYPE.itemsize == 176 and vxslam.TRACK_ESS_RESULT_DTYPE.itemsize == 288


def test_options_pair():
    po, eo = vxslam.track_frame_options(min_matches=40, min_inliers=12, pnp={"seed": 3}, ess={"max_iterations": 64})
    assert po.dtype == vxslam.TRACK_OPTIONS_DTYPE and eo.dtype == vxslam.TRACK_ESS_OPTIONS_DTYPE
    assert po["min_matches"] == eo["min_matches"] == 40 and po["min_inliers"] == eo["min_inliers"] == 12
    assert po["pnp"]["seed"] == 3 and eo["ess"]["max_iterations"] == 64
    po, eo = vxslam.track_frame_options()
    assert po.tobytes() == vxslam.track_options().tobytes() and eo.tobytes() == vxslam.track_essential_options().tobytes()


def test_null_arguments_need_no_device():
    L = vxslam.lib()
    assert L.vx_frame_create(None, 8, None) == vxslam.VX_ERR_INVALID
    assert L.vx_frame_device(None, None, None, None, None, None) == vxslam.VX_ERR_INVALID
    assert L.vx_frame_fetch(None, None, None, None, 0, None) == vxslam.VX_ERR_INVALID
    assert L.vx_track_frame_async(None, None, 0, None, None, None, 0.8, None, None, None, None) == vxslam.VX_ERR_INVALID
    assert L.vx_track_frame_fetch(None, None, None, 0, None) == vxslam.VX_ERR_INVALID
    assert L.vx_track_frame_matches(None, 0, None, None, None) == vxslam.VX_ERR_INVALID
    L.vx_frame_destroy(None)


def test_scene_helper_is_consistent():
    s = synth.make_track_frame_scene(5, 64, wrong_frac=0.25)
    assert s["last_xy"].dtype == np.float32 and s["last_xy"].shape == (64, 2) and s["desc_last"].shape == (64, 32)
    # last feature i's descriptor is flips_last[i] bits from the current keypoint train_of[i]'s
    d = np.unpackbits(s["desc_last"] ^ s["desc_curr"][s["train_of"]], axis=1).sum(1)
    assert np.array_equal(d, s["flips_last"]) and np.array_equal(s["matches_last"]["train_idx"], s["train_of"])
    # T_cl * T_lw = T_cw, and the right pixels of both frames see the landmarks
    R_lw = synth.quat_to_mat(s["pose_last"][:4])
    assert np.abs(s["R_cl"] @ R_lw - s["R"]).max() < 1e-12
    assert np.abs(s["R_cl"] @ s["pose_last"][4:] + s["t_cl"] - s["t"]).max() < 1e-12
    fx, fy, cx, cy = s["intr"]
    pl = s["lm_pos"] @ R_lw.T + s["pose_last"][4:]
    uv = np.stack([fx * pl[:, 0] / pl[:, 2] + cx, fy * pl[:, 1] / pl[:, 2] + cy], -1)
    assert (pl[:, 2] > 0.5).all() and np.abs(uv - s["last_xy"]).max() < 5.0
    a = synth.make_track_scene(5, 64, wrong_frac=0.25)
    assert all(np.array_equal(a[k], s[k]) for k in a)  # it only adds


# ---------------------------------------------------------------------------- the decision table
def pnp_rec(n_good=200, n_pairs=150, ok=1, n_inliers=120, pose=POSE, parallax=7.5):
    r = np.zeros((), vxslam.TRACK_RESULT_DTYPE)
    r["n_matches"], r["n_good_matches"], r["n_pairs"], r["min_distance"], r["parallax"] = 220, n_good, n_pairs, 3.0, parallax
    r["pnp"]["ok"], r["pnp"]["n_inliers"], r["pnp"]["pose"] = ok, n_inliers, pose
    r["status"] = 77  # ignored: evaluated by the reference
    return r


def ess_rec(n_good=180, ok=1, n_inliers=90, parallax=4.25):
    r = np.zeros((), vxslam.TRACK_ESS_RESULT_DTYPE)
    r["n_matches"], r["n_good_matches"], r["n_pairs"], r["min_distance"], r["parallax"] = 190, n_good, n_good, 2.0, parallax
    r["ess"]["ok"], r["ess"]["n_inliers"] = ok, n_inliers
    r["pose"] = POSE[::-1] if ok else 0.0
    r["status"] = 77
    return r


PNP_FAILURES = {
    R.FEW_MATCHES: dict(n_good=MM - 1),
    R.FEW_PAIRS: dict(n_pairs=MI - 1),
    R.PNP_FAILED: dict(ok=0, n_inliers=0),
    R.BAD_ROTATION: dict(pose=np.array([0.1, np.nan, 0.3, 0.9, 1.0, 2.0, 3.0])),
}
OPTS = ({"min_matches": MM, "min_inliers": MI}, {"min_matches": MM, "min_inliers": MI})


def test_pnp_ok_closes_the_gate():
    out = track_frame_ref(pnp_rec(), ess_rec(), *OPTS, n_keypoints=321)
    assert (out["path"], out["status"], out["pnp_ran"], out["ess_ran"]) == (R.PATH_PNP, R.OK, 1, 0)
    assert out["n_inliers"] == 120 and out["parallax"] == 7.5 and np.array_equal(out["pose"], POSE)
    assert out["n_keypoints"] == 321 and out["pnp"]["status"] == R.OK
    # the fallback's record is the empty one, whatever TrackLastFrame would have given
    assert out["ess"]["n_matches"] == 0 and out["ess"]["ess"]["ok"] == 0 and out["ess"]["min_distance"] == 100.0
    assert out["ess"]["status"] == R.FEW_MATCHES


@pytest.mark.parametrize("failure", sorted(PNP_FAILURES))
def test_pnp_failure_then_essential_ok(failure):
    out = track_frame_ref(pnp_rec(**PNP_FAILURES[failure]), ess_rec(), *OPTS)
    assert out["pnp"]["status"] == failure and (out["pnp_ran"], out["ess_ran"]) == (1, 1)
    assert (out["path"], out["status"]) == (R.PATH_ESSENTIAL, R.OK)
    assert out["n_inliers"] == 90 and out["parallax"] == 4.25 and np.array_equal(out["pose"], POSE[::-1])


@pytest.mark.parametrize("failure", sorted(PNP_FAILURES))
@pytest.mark.parametrize("ess_kw, ess_failure", [(dict(n_good=MM - 1), R.FEW_MATCHES), (dict(ok=0, n_inliers=0), R.ESSENTIAL_FAILED),
                                                 (dict(n_inliers=MI - 1), R.ESSENTIAL_FAILED)])
def test_pnp_failure_then_essential_failure(failure, ess_kw, ess_failure):
    out = track_frame_ref(pnp_rec(**PNP_FAILURES[failure]), ess_rec(**ess_kw), *OPTS)
    assert (out["pnp_ran"], out["ess_ran"], out["path"]) == (1, 1, R.PATH_NONE)
    assert out["status"] == ess_failure == out["ess"]["status"] and out["pnp"]["status"] == failure
    assert out["n_inliers"] == 0 and out["parallax"] == 0.0 and not out["pose"].any()


def test_no_keyframe_goes_straight_to_the_fallback():
    out = track_frame_ref(None, ess_rec(), *OPTS)
    assert (out["pnp_ran"], out["ess_ran"], out["path"], out["status"]) == (0, 1, R.PATH_ESSENTIAL, R.OK)
    assert out["pnp"].tobytes() == bytes(176)
    out = track_frame_ref(None, ess_rec(ok=0, n_inliers=0), *OPTS)
    assert (out["path"], out["status"]) == (R.PATH_NONE, R.ESSENTIAL_FAILED)


def test_no_last_frame_fails_the_fallback():
    out = track_frame_ref(pnp_rec(n_pairs=3), None, *OPTS)
    assert (out["pnp_ran"], out["ess_ran"], out["path"], out["status"]) == (1, 0, R.PATH_NONE, R.FEW_PAIRS)
    assert not out["pose"].any() and out["ess"]["n_matches"] == 0
    out = track_frame_ref(pnp_rec(), None, *OPTS)  # PnP needs no last frame
    assert (out["path"], out["status"], out["ess_ran"]) == (R.PATH_PNP, R.OK, 0)


# ---------------------------------------------------------------------------- the status rules' boundaries
PNP_CASES = [  # (n_good, n_pairs, ok, n_inliers, pose), expected
    ((MM - 1, 150, 1, 120, "finite"), R.FEW_MATCHES), ((MM, 150, 1, 120, "finite"), R.OK),
    ((200, MI - 1, 1, 120, "finite"), R.FEW_PAIRS), ((200, MI, 1, MI, "finite"), R.OK),
    ((200, 150, 1, MI - 1, "finite"), R.PNP_FAILED), ((200, 150, 1, MI, "finite"), R.OK),
    ((200, 150, 0, 120, "finite"), R.PNP_FAILED),
    ((200, 150, 1, 120, "nan"), R.BAD_ROTATION), ((200, 150, 1, 120, "inf"), R.BAD_ROTATION),
    # the order of the return statements: the earliest failing gate names the status
    ((MM - 1, MI - 1, 0, 0, "nan"), R.FEW_MATCHES), ((MM, MI - 1, 0, 0, "nan"), R.FEW_PAIRS),
    ((MM, MI, 0, 0, "nan"), R.PNP_FAILED),
]
ESS_CASES = [  # (n_good, ok, n_inliers), expected
    ((MM - 1, 1, 90), R.FEW_MATCHES), ((MM, 1, 90), R.OK), ((200, 1, MI - 1), R.ESSENTIAL_FAILED),
    ((200, 1, MI), R.OK), ((200, 0, 90), R.ESSENTIAL_FAILED), ((MM - 1, 0, 0), R.FEW_MATCHES),
]


def test_status_boundaries_on_both_statements():
    """the shared C++ rule (csrc/track_common.hpp, run on the host by build/track_status_check) and the numpy
    restatement the GPU tests compose (tests/track_frame_ref.py), on the same boundary cases"""
    for (ng, npairs, ok, ni, pose), want in PNP_CASES:
        p = POSE.copy()
        if pose == "nan":
            p[5] = np.nan
        if pose == "inf":
            p[0] = -np.inf
        assert R.pnp_status(pnp_rec(ng, npairs, ok, ni, p), MM, MI) == want, (ng, npairs, ok, ni, pose)
    for (ng, ok, ni), want in ESS_CASES:
        assert R.ess_status(ess_rec(ng, ok, ni), MM, MI) == want, (ng, ok, ni)
    assert os.path.exists(CHECK), f"{CHECK} missing: run __graft_entry__.build()"
    lines = ["pnp %d %d %d %d %s %d %d" % (*c, MM, MI) for c, _ in PNP_CASES]
    lines += ["ess %d %d %d %d %d" % (*c, MM, MI) for c, _ in ESS_CASES]
    out = subprocess.run([CHECK], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    assert [int(x) for x in out.split()] == [w for _, w in PNP_CASES + ESS_CASES]
    # and both fetches evaluate that statement, not one of their own
    for f, fn in (("track.hip", "trk::pnp_status"), ("track_ess.hip", "trk::ess_status")):
        src = open(os.path.join(ROOT, "visionx-slam_amd", "csrc", f)).read()
        assert fn in src and "out->status = VX_TRACK_FEW_MATCHES" not in src, f
