"""visionx::MapCulling (visionx-slam_amd/host, over vx_dmap_cull_landmarks / vx_dmap_cull_keyframes)
driven by tests/cpp/cull_driver on a dumped 6 + 2 keyframe / 300 landmark scene: the host objects the
adapter edited equal, field for field, the ones the driver's sequential walk of tracking.cpp:652-840
edited (bad flags, the three feature fields, observation maps, map membership), and both equal the
numpy restatement (tests/cull_ref.py), whose records the adapter's lists must be."""
import os
import subprocess

import numpy as np
import pytest

import vxslam
from vxslam import synth

import cull_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "visionx-slam_amd", "build", "cull_driver")
FILES = ("kf_id", "kf_pose", "kf_intr", "kf_has_cam", "kf_feat_ptr", "feat_uv", "feat_lm_id", "feat_flags", "lm_id",
         "lm_pos", "lm_bad", "lm_obs_ptr", "obs_kf_id", "obs_feat_idx")


def dump(m, o, protect, path):
    for k in FILES:
        np.ascontiguousarray(m[k]).tofile(os.path.join(path, k + ".bin"))
    np.ascontiguousarray(o).tofile(os.path.join(path, "opts.bin"))
    np.array(list(protect), np.uint64).tofile(os.path.join(path, "protect.bin"))


def state(path, x):
    rd = lambda n, t: np.fromfile(os.path.join(path, f"{x}_{n}.bin"), t)
    return {"kf_in": rd("kf_in", np.uint8), "lm_in": rd("lm_in", np.uint8), "lm_bad": rd("lm_bad", np.uint8),
            "feat_lm": rd("feat_lm", np.uint64), "feat_fl": rd("feat_fl", np.uint8), "obs": rd("obs", np.uint64).reshape(-1, 3)}


@pytest.mark.parametrize("what", ["landmarks", "keyframes"])
def test_adapter_equals_sequential_walk_and_restatement(what, tmp_path):
    if not os.path.exists(DRIVER):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "visionx-slam_amd"), "-j8"], check=True)
    m = synth.make_cull_scene(0xC012, 6, 300, special=False, lm_sigma=0.03, min_margin=1e-9)
    o = vxslam.cull_options(kf_redundant_ratio=0.5, max_keyframes=5, kf_min_shared_observations=2)
    protect = [int(m["kf_id"][0]), int(m["kf_id"][-1])]
    dump(m, o, protect, tmp_path)
    out = subprocess.run([DRIVER, str(tmp_path), what], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    n_h, n_a, rm_h, rm_a, ratio_h, ratio_a, ms_walk, ms_dev = out.stdout.split()
    print("walk", ms_walk, "ms, adapter", ms_dev, "ms (one call each, unwarmed)")
    ref = m.copy()
    if what == "landmarks":
        want = cull_ref.cull_landmarks(ref, o)
        assert np.bincount(want["landmarks"]["reason"], minlength=6)[1:].tolist() == [3, 9, 0, 60, 58]
        assert int(rm_h) == int(rm_a) == 0
    else:
        want = cull_ref.cull_keyframes(ref, o, protect)
        assert want["removed"] and want["kf_id"] == int(m["kf_id"][1]) and int(rm_h) == int(rm_a) == 1
        assert float(ratio_h) == float(ratio_a) == want["ratio"]
    assert int(n_h) == int(n_a) == len(want["landmarks"]) > 100
    h, a = state(tmp_path, "H"), state(tmp_path, "A")
    for k in h:
        assert np.array_equal(h[k], a[k]), k
    # ... and both are the restatement's map
    assert np.array_equal(a["kf_in"], ref["kf_alive"]) and np.array_equal(a["lm_in"], 1 - ref["lm_removed"])
    assert np.array_equal(a["feat_lm"], ref["feat_lm_id"]) and np.array_equal(a["feat_fl"], ref["feat_flags"])
    assert np.array_equal(a["lm_bad"], ref["lm_bad"])
    lm = np.repeat(np.arange(len(ref["lm_id"])), np.diff(ref["lm_obs_ptr"]))
    live = ref["obs_live"] > 0
    robs = np.stack([ref["lm_id"][lm[live]], ref["obs_kf_id"][live], ref["obs_feat_idx"][live]], -1)
    key = lambda x: x[np.lexsort((x[:, 1], np.searchsorted(np.sort(ref["lm_id"]), x[:, 0])))]
    assert np.array_equal(key(a["obs"]), key(robs))
    # the adapter's lists are the restatement's records
    lm_rec = np.fromfile(os.path.join(tmp_path, "A_lm_records.bin"), vxslam.CULL_LANDMARK_DTYPE)
    ft_rec = np.fromfile(os.path.join(tmp_path, "A_feat_records.bin"), vxslam.CULL_FEATURE_DTYPE)
    for k in ("lm_id", "row", "reason", "n_projected"):
        assert np.array_equal(lm_rec[k], want["landmarks"][k]), k
    assert np.all(np.abs(lm_rec["mean_err"] - want["landmarks"]["mean_err"]) <= 1e-12 * want["landmarks"]["mean_err"])
    assert np.array_equal(ft_rec, want["features"])
