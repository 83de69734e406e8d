"""visionx::KeyFrameLandmarks::CreateKeyFrame (visionx-slam_amd/host, over vx_dmap_create_keyframe_host)
driven by tests/cpp/keyframe_driver on a dumped 6 + 1 keyframe / 300 landmark map and a 300-feature
frame matched to its last keyframe: the host objects the one call left equal, field for field, the
ones the sequential host path left (landmark ids, positions, observation maps, the three feature
fields of every frame, map membership; both resident maps' counts), both equal the numpy restatement
(tests/keyframe_ref.py), and the adapter's records are the restatement's."""
import os
import subprocess

import numpy as np
import pytest

import vxslam

import keyframe_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "visionx-slam_amd", "build", "keyframe_driver")
FILES = ("kf_id", "kf_pose", "kf_intr", "kf_has_cam", "kf_feat_ptr", "feat_uv", "feat_lm_id", "feat_flags", "lm_id",
         "lm_pos", "lm_bad", "lm_obs_ptr", "obs_kf_id", "obs_feat_idx")


def state(path, x):
    rd = lambda n, t: np.fromfile(os.path.join(path, f"{x}_{n}.bin"), t)
    return {"kf_in": rd("kf_in", np.uint8), "lm_in": rd("lm_in", np.uint8), "lm_id": rd("lm_id", np.uint64),
            "lm_pos": rd("lm_pos", np.float64).reshape(-1, 3), "feat_lm": rd("feat_lm", np.uint64),
            "feat_fl": rd("feat_fl", np.uint8), "obs": rd("obs", np.uint64).reshape(-1, 3), "counts": rd("counts", np.int64)}


def test_one_call_equals_the_sequential_path_and_the_restatement(tmp_path):
    if not os.path.exists(DRIVER):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "visionx-slam_amd"), "-j8"], check=True)
    m, d, last, new, first = R.edit_scene(64)
    for k in FILES:
        np.ascontiguousarray(m[k]).tofile(os.path.join(tmp_path, k + ".bin"))
    np.array([new, last, first], np.uint64).tofile(os.path.join(tmp_path, "new_ids.bin"))
    for k, v in (("new_pose", d["pose2"]), ("new_intr", d["intr"]), ("new_uv", d["uv2"]), ("matches", d["matches"]),
                 ("depth", d["depth"]), ("opts", vxslam.keyframe_options())):
        np.ascontiguousarray(v).tofile(os.path.join(tmp_path, k + ".bin"))
    np.array([d["depth"].shape[0], d["depth"].shape[1], vxslam.DEPTH_TYPES[d["depth"].dtype], d["depth"].strides[0]],
             np.int64).tofile(os.path.join(tmp_path, "depth_shape.bin"))
    out = subprocess.run([DRIVER, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    ref = m.copy()
    want = R.create_keyframe(ref, new, d["pose2"], d["intr"], d["uv2"], last, d["matches"], d["depth"], first)
    assert min(want["margins"].values()) > 1e-9, want["margins"]
    recs = want["landmarks"]
    assert want["n_depth"] > 50 and want["n_triangulated"] > 20
    next_h, next_a = (int(x) for x in out.stdout.split())
    assert next_h == next_a == first + len(recs)
    h, a = state(tmp_path, "H"), state(tmp_path, "A")
    tri = np.concatenate([np.zeros(len(m["lm_id"]), bool), recs["kind"] == 1])
    for k in h:
        if k == "lm_pos":  # depth points and the map's own bitwise; the two triangulation calls to 1e-9
            assert np.array_equal(h[k][~tri], a[k][~tri])
            assert np.abs(h[k][tri] - a[k][tri]).max() <= 1e-9 * np.abs(h[k][tri]).max()
        else:
            assert np.array_equal(h[k], a[k]), k
    # ... and both are the restatement's map
    assert a["kf_in"].all() and a["lm_in"].all() and np.array_equal(a["lm_id"], ref["lm_id"])
    assert np.array_equal(a["feat_lm"], ref["feat_lm_id"]) and np.array_equal(a["feat_fl"], ref["feat_flags"])
    assert np.array_equal(a["lm_pos"][~tri], ref["lm_pos"].reshape(-1, 3)[~tri])
    assert np.abs(a["lm_pos"][tri] - ref["lm_pos"].reshape(-1, 3)[tri]).max() <= 1e-9 * np.abs(ref["lm_pos"].reshape(-1, 3)[tri]).max()
    lm = np.repeat(np.arange(len(ref["lm_id"])), np.diff(ref["lm_obs_ptr"]))
    robs = np.stack([ref["lm_id"][lm], ref["obs_kf_id"], ref["obs_feat_idx"]], -1)
    key = lambda x: x[np.lexsort((x[:, 1], np.searchsorted(np.sort(ref["lm_id"]), x[:, 0])))]
    assert np.array_equal(key(a["obs"]), key(robs))
    assert a["counts"].tolist() == [len(ref["kf_id"]), int(ref["kf_feat_ptr"][-1]), len(ref["lm_id"]), len(robs),
                                    len(ref["kf_id"]), len(ref["lm_id"]), len(robs), 0]
    # the adapter's records are the restatement's
    rec = np.fromfile(os.path.join(tmp_path, "A_records.bin"), vxslam.KEYFRAME_LANDMARK_DTYPE)
    for k in ("lm_id", "row", "kind", "feat_curr", "feat_last"):
        assert np.array_equal(rec[k], recs[k]), k
    dep = recs["kind"] == 0
    assert np.array_equal(rec["pw"][dep], recs["pw"][dep])
    assert np.abs(rec["pw"][~dep] - recs["pw"][~dep]).max() <= 1e-9 * np.abs(recs["pw"][~dep]).max()
