"""visionx::EssentialTracker and visionx::FrameTracker (visionx-slam_amd/host, over
vx_track_essential_host_async) driven by tests/cpp/track_ess_driver on dumped 300-feature scenes: the
pose they set, the inlier count and the parallax equal the Python path's (Context.match +
track_essential_async + track_essential_fetch) on the same scene — the same kernels on the same inputs,
so bit for bit — and the host's SE3d::operator* reproduces the device's composition."""
import os
import subprocess

import numpy as np
import pytest

import vxslam
from vxslam import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "visionx-slam_amd", "build", "track_ess_driver")


def run(cmd, tmp_path):
    if not os.path.exists(DRIVER):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "visionx-slam_amd"), "-j8"], check=True)
    out = subprocess.run([DRIVER, cmd, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return [line.split() for line in out.stdout.strip().splitlines()]


def dump(tmp_path, **arrays):
    for k, v in arrays.items():
        np.ascontiguousarray(v).tofile(os.path.join(tmp_path, k + ".bin"))


def dump_last_frame(tmp_path, s):
    dump(tmp_path, last_xy=s["last_xy"], curr_xy=s["curr_xy"], desc_last=s["desc_last"], desc_curr=s["desc_curr"],
         intr=s["intr"], pose_last=s["pose_last"])


def python_path(ctx, s, pose_last):
    """match + track_essential_async on explicit device arrays, default options"""
    import torch

    m = ctx.match(s["desc_last"], s["desc_curr"])
    assert np.array_equal(m, s["matches"].astype(vxslam.MATCH_DTYPE))
    dev = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
           for a in (s["last_xy"], s["curr_xy"], np.array([len(s["last_xy"])], np.int32), m, np.array([len(m)], np.int32))]
    torch.cuda.synchronize()
    ctx.track_essential_async((dev[0].data_ptr(), 8, dev[2].data_ptr()), (dev[1].data_ptr(), 8, dev[2].data_ptr()),
                              s["intr"], vxslam.track_essential_options(),
                              matches=(dev[3].data_ptr(), dev[4].data_ptr(), len(m)), pose_last=pose_last)
    return ctx.track_essential_fetch()[0]


@pytest.fixture(scope="module")
def scene():
    return synth.make_last_frame_scene(3, 300, wrong_frac=0.3)


def test_essential_tracker_equals_python_path(ctx, tmp_path, scene):
    s = scene
    dump_last_frame(tmp_path, s)
    (ok, inliers, parallax, host_eq), (ok2, inliers2, parallax2, host_eq2) = run("last", tmp_path)
    pose = np.fromfile(os.path.join(tmp_path, "pose.out"), np.float64)
    res = np.fromfile(os.path.join(tmp_path, "result.out"), vxslam.TRACK_ESS_RESULT_DTYPE)[0]
    py = python_path(ctx, s, s["pose_last"])
    assert py["status"] == vxslam.TRACK_OK and py["n_pairs"] == 300
    assert int(ok) == 1 and int(inliers) == py["ess"]["n_inliers"] >= 30
    assert float(parallax) == py["parallax"]
    assert res.tobytes() == py.tobytes()
    assert np.array_equal(pose, py["pose"])
    assert int(host_eq) == 1   # PoseFromRt(R, t) * last->Pose() on the host, bit for bit
    assert np.abs(synth.quat_to_mat(pose[:4]) - s["R_cw"]).max() < 0.02
    # EstimateInitialPose == the call with identity; its parallax is the reference's float
    init_pose = np.fromfile(os.path.join(tmp_path, "init_pose.out"), np.float64)
    init_res = np.fromfile(os.path.join(tmp_path, "init_result.out"), vxslam.TRACK_ESS_RESULT_DTYPE)[0]
    py0 = python_path(ctx, s, None)
    assert int(ok2) == 1 and int(inliers2) == py0["ess"]["n_inliers"] and int(host_eq2) == 1
    assert float(parallax2) == float(np.float32(py0["parallax"])) >= np.float32(np.pi / 180)
    assert init_res.tobytes() == py0.tobytes() and np.array_equal(init_pose, py0["pose"])
    assert py0["ess"].tobytes() == py["ess"].tobytes() and not np.array_equal(init_pose, pose)


def test_essential_tracker_failures(ctx, tmp_path):
    """all-outlier matches: false, the pose and the kept LastInliers / LastParallax untouched"""
    s = synth.make_last_frame_scene(8, 300, wrong_frac=1.0)
    dump_last_frame(tmp_path, s)
    (ok, inliers, parallax, _), (ok2, inliers2, parallax2, _) = run("last", tmp_path)
    assert (int(ok), int(inliers), float(parallax)) == (0, 0, 0.0)
    assert (int(ok2), int(inliers2), float(parallax2)) == (0, 0, 0.0)
    assert np.array_equal(np.fromfile(os.path.join(tmp_path, "pose.out"), np.float64), [0, 0, 0, 1, 0, 0, 0])
    res = np.fromfile(os.path.join(tmp_path, "result.out"), vxslam.TRACK_ESS_RESULT_DTYPE)[0]
    assert res["status"] == vxslam.TRACK_ESSENTIAL_FAILED
    assert res.tobytes() == python_path(ctx, s, s["pose_last"]).tobytes()


def test_frame_tracker_takes_pnp_then_the_fallback(ctx, tmp_path, scene):
    import torch

    # 1: a keyframe whose landmarks are good -> TrackWithPnP succeeds, TrackLastFrame is not run
    t = synth.make_track_scene(3, 300, wrong_frac=0.3)
    kf_files = dict(kf_uv=t["kf_uv"], lm_id=t["lm_id"], flags=t["flags"], lm_pos=t["lm_pos"],
                    lm_bad=np.zeros(300, np.uint8), desc_kf=t["desc_kf"], kf_pose=t["pose"])
    dump(tmp_path, **kf_files, last_xy=t["kf_uv"].astype(np.float32), desc_last=t["desc_kf"], curr_xy=t["curr_xy"],
         desc_curr=t["desc_curr"], intr=t["intr"], pose_last=t["pose"])
    (ok, fallback, inliers, parallax), = run("track", tmp_path)
    pose = np.fromfile(os.path.join(tmp_path, "pose.out"), np.float64)
    dm = vxslam.DMap(ctx)
    dm.add_landmarks(t["lm_id"], t["lm_pos"])
    dm.add_keyframe(7, t["pose"], t["intr"], True, t["kf_uv"], t["lm_id"], t["flags"])
    m = ctx.match(t["desc_kf"], t["desc_curr"])
    dev = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
           for a in (t["curr_xy"], np.array([300], np.int32), m, np.array([len(m)], np.int32))]
    torch.cuda.synchronize()
    ctx.track_pnp_async(dm, 7, (dev[0].data_ptr(), 8, dev[1].data_ptr()), t["intr"], vxslam.track_options(),
                        matches=(dev[2].data_ptr(), dev[3].data_ptr(), len(m)))
    py = ctx.track_pnp_fetch()[0]
    dm.close()
    assert py["status"] == vxslam.TRACK_OK
    assert (int(ok), int(fallback), int(inliers)) == (1, 0, py["pnp"]["n_inliers"]) and float(parallax) == py["parallax"]
    assert np.array_equal(pose, py["pnp"]["pose"])

    # 2: every landmark of the keyframe bad -> TrackWithPnP fails (no pairs), TrackLastFrame sets the pose
    s = scene
    dump_last_frame(tmp_path, s)
    dump(tmp_path, kf_uv=s["last_xy"].astype(np.float64), lm_id=t["lm_id"], flags=t["flags"], lm_pos=t["lm_pos"],
         lm_bad=np.ones(300, np.uint8), desc_kf=s["desc_last"], kf_pose=s["pose_last"])
    (ok, fallback, inliers, parallax), = run("track", tmp_path)
    pose = np.fromfile(os.path.join(tmp_path, "pose.out"), np.float64)
    py = python_path(ctx, s, s["pose_last"])
    assert py["status"] == vxslam.TRACK_OK
    assert (int(ok), int(fallback), int(inliers)) == (1, 1, py["ess"]["n_inliers"]) and float(parallax) == py["parallax"]
    assert np.array_equal(pose, py["pose"])
