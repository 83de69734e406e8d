"""visionx::PnPTracker::TrackWithPnP (visionx-slam_amd/host, over vx_track_pnp_host_async) driven by
tests/cpp/track_driver on a dumped 300-feature scene: the pose it sets, the inlier count and the
parallax equal the Python path's (Context.match + track_pnp_async + track_pnp_fetch) on the same
scene — the same kernels on the same inputs, so bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import vxslam
from vxslam import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "visionx-slam_amd", "build", "track_driver")


def test_pnp_tracker_equals_python_path(ctx, tmp_path):
    import torch

    if not os.path.exists(DRIVER):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "visionx-slam_amd"), "-j8"], check=True)
    s = synth.make_track_scene(3, 300, wrong_frac=0.3)
    bad = np.zeros(300, np.uint8)
    bad[[5, 111]] = 1      # Landmark::IsBad
    bad[[40, 222]] = 2     # never inserted into the map
    for k, v in (("kf_uv", s["kf_uv"]), ("lm_id", s["lm_id"]), ("flags", s["flags"]), ("lm_pos", s["lm_pos"]),
                 ("lm_bad", bad), ("desc_kf", s["desc_kf"]), ("desc_curr", s["desc_curr"]), ("curr_xy", s["curr_xy"]),
                 ("intr", s["intr"]), ("kf_pose", s["pose"])):
        np.ascontiguousarray(v).tofile(os.path.join(tmp_path, k + ".bin"))
    out = subprocess.run([DRIVER, "pnp", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    ok, inliers, parallax = out.stdout.split()
    pose = np.fromfile(os.path.join(tmp_path, "pose.out"), np.float64)
    res = np.fromfile(os.path.join(tmp_path, "result.out"), vxslam.TRACK_RESULT_DTYPE)[0]

    # the Python path on the same scene
    dm = vxslam.DMap(ctx)
    keep = bad != 2
    dm.add_landmarks(s["lm_id"][keep], s["lm_pos"][keep], bad[keep])
    dm.add_keyframe(7, s["pose"], s["intr"], True, s["kf_uv"], s["lm_id"], s["flags"])
    m = ctx.match(s["desc_kf"], s["desc_curr"])
    assert np.array_equal(m, s["matches"].astype(vxslam.MATCH_DTYPE))
    dev = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
           for a in (s["curr_xy"], np.array([300], np.int32), m, np.array([len(m)], np.int32))]
    torch.cuda.synchronize()
    ctx.track_pnp_async(dm, 7, (dev[0].data_ptr(), 8, dev[1].data_ptr()), s["intr"], vxslam.track_options(),
                        matches=(dev[2].data_ptr(), dev[3].data_ptr(), len(m)))
    py, pm, _ = ctx.track_pnp_fetch()
    dm.close()
    assert py["status"] == vxslam.TRACK_OK and py["n_pairs"] == 296 and not (set(pm.tolist()) & {5, 111, 40, 222})
    assert int(ok) == 1 and int(inliers) == py["pnp"]["n_inliers"] >= 30
    assert float(parallax) == py["parallax"]
    assert res.tobytes() == py.tobytes()
    assert np.array_equal(pose, py["pnp"]["pose"])
    assert np.abs(pose - s["pose"]).max() < 5e-3
