"""vx_track_essential_* (csrc/track_ess.hip) without a GPU: the declarations, exports and record
layouts, argument checks that need no device, and the numpy restatement of tracking.cpp:291-325 /
:539-541 (tests/track_ess_ref.py, the reference of tests/test_gpu_track_essential.py) pinned on
hand-written cases."""
import os
import re
import subprocess

import numpy as np

import vxslam
from vxslam import synth

from track_ess_ref import compose, pose_from_Rt, track_ess_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["vx_track_essential_default_options", "vx_track_essential_async", "vx_track_essential_host_async",
         "vx_track_essential_fetch"]


def _m(rows):
    return np.array(rows, vxslam.MATCH_DTYPE)


def _xy(n=8):
    last = (np.arange(2 * n, dtype=np.float32).reshape(n, 2) * np.float32(1.25))
    curr = last + np.array([3.0, 4.0], np.float32)  # every displacement is 5 px
    return last, curr


# ---------------------------------------------------------------------------- the C surface
def test_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "vx_slam.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", vxslam.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert re.search(r" T %s$" % n, out, flags=re.M), n
        assert n in vxslam.EXPORTS, n
    for n in ("vx_track_essential_options", "vx_track_essential_result"):
        assert re.search(r"\}\s*%s;" % n, hdr), n
    assert re.search(r"#define\s+VX_TRACK_ESSENTIAL_FAILED\s+5\b", hdr) and vxslam.TRACK_ESSENTIAL_FAILED == 5
    for n in ("track_essential_options", "TRACK_ESS_OPTIONS_DTYPE", "TRACK_ESS_RESULT_DTYPE"):
        assert hasattr(vxslam, n), n
    for n in ("track_essential_async", "track_essential_host_async", "track_essential_fetch"):
        assert hasattr(vxslam.Context, n), n


def test_record_sizes_match_the_c_structs():
    src = open(os.path.join(ROOT, "visionx-slam_amd", "csrc", "track_ess.hip")).read()
    sizes = dict(re.findall(r"static_assert\(sizeof\((vx_track_essential_\w+)\) == (\d+)", src))
    assert int(sizes["vx_track_essential_options"]) == vxslam.TRACK_ESS_OPTIONS_DTYPE.itemsize == 48
    R = vxslam.TRACK_ESS_RESULT_DTYPE
    assert int(sizes["vx_track_essential_result"]) == R.itemsize == 288
    # no implicit padding: every field starts where the previous one ends
    end = 0
    for name in R.names:
        dt, off = R.fields[name][:2]
        assert off == end, name
        end = off + dt.itemsize
    assert end == R.itemsize
    assert (R.fields["parallax"][1], R.fields["pose"][1], R.fields["ess"][1]) == (24, 32, 88)
    assert vxslam.TRACK_ESS_OPTIONS_DTYPE.fields["ess"][1] == 8
    # the PnP records are untouched
    assert vxslam.TRACK_OPTIONS_DTYPE.itemsize == 40 and vxslam.TRACK_RESULT_DTYPE.itemsize == 176


def test_default_options_writes_exactly_the_struct():
    buf = np.full(64, 0xAB, np.uint8)
    vxslam.lib().vx_track_essential_default_options(buf.ctypes.data)
    assert (buf[48:] == 0xAB).all() and (buf[:4] != 0xAB).any()
    o = buf[:48].view(vxslam.TRACK_ESS_OPTIONS_DTYPE)[0]
    assert o.tobytes() == vxslam.track_essential_options().tobytes()
    assert o["min_matches"] == 50 and o["min_inliers"] == 30
    assert o["ess"].tobytes() == vxslam.essential_options().tobytes()
    o = vxslam.track_essential_options(min_inliers=7, max_iterations=64, seed=9, threshold=2.0)
    assert o["min_inliers"] == 7 and o["ess"]["max_iterations"] == 64 and o["ess"]["seed"] == 9
    assert o["ess"]["threshold"] == 2.0 and o["ess"]["confidence"] == 0.999


def test_null_context_is_invalid():
    L = vxslam.lib()
    res = np.zeros(1, vxslam.TRACK_ESS_RESULT_DTYPE)
    opt = vxslam.track_essential_options()
    intr = np.array([500.0, 500.0, 320.0, 240.0])
    d = np.zeros(64, np.uint8).ctypes.data
    assert L.vx_track_essential_async(None, d, 8, d, d, 8, d, None, None, 0, None, intr.ctypes.data, opt.ctypes.data) == -1
    assert L.vx_track_essential_async(None, None, 8, None, None, 8, None, None, None, 0, None, None, None) == -1
    assert L.vx_track_essential_host_async(None, d, 1, d, d, 1, d, 0.8, None, intr.ctypes.data, opt.ctypes.data) == -1
    assert L.vx_track_essential_host_async(None, None, 0, None, None, 0, None, 0.8, None, None, None) == -1
    assert L.vx_track_essential_fetch(None, res.ctypes.data, None, None, 0) == -1
    assert L.vx_track_essential_fetch(None, None, None, None, 0) == -1
    L.vx_track_essential_default_options(None)  # a no-op


# ---------------------------------------------------------------------------- the filter
def test_ref_filter_thresholds_around_15():
    """thr = max(2 * min_dist, 30): the floor holds up to min_dist 15, 2 * min_dist takes over at 16"""
    last, curr = _xy()
    for mn, thr, kept in ((14.0, 30.0, [0, 1, 2]), (15.0, 30.0, [0, 1, 2]), (16.0, 32.0, [0, 1, 2, 3])):
        r = track_ess_ref(_m([(0, 0, mn), (1, 1, 30.0), (2, 2, 29.5), (3, 3, 32.0), (4, 4, 32.5)]), last, curr, 1)
        assert r["min_distance"] == np.float32(mn) and r["thr"] == np.float32(thr), mn
        assert list(r["good"]) == kept and list(r["pair_match"]) == kept
    r = track_ess_ref(_m([]), last, curr, 1)
    assert r["min_distance"] == 100.0 and r["thr"] == 200.0 and r["n_good_matches"] == 0
    assert r["gate"] == 1 and r["parallax"] == 0.0 and r["n_pairs"] == 0
    assert track_ess_ref(_m([]), last, curr, 0)["gate"] == 0
    r = track_ess_ref(_m([(0, 0, 150.0), (1, 1, 101.0), (2, 2, 200.0), (3, 3, 201.0)]), last, curr, 1)
    assert r["min_distance"] == 100.0 and list(r["good"]) == [0, 1, 2]


def test_ref_pairs_bad_indices_and_parallax():
    last, curr = _xy()
    m = _m([(7, 6, 5.0), (0, 7, 99.0), (3, 2, 5.0), (8, 0, 5.0), (0, 8, 5.0), (-1, 0, 5.0), (0, -1, 5.0), (2, 2, 6.0)])
    r = track_ess_ref(m, last, curr, 3)
    assert list(r["good"]) == [0, 2, 3, 4, 5, 6, 7] and r["n_bad_index"] == 4
    assert list(r["pair_match"]) == [0, 2, 7] and r["n_pairs"] == 3 and r["gate"] == 0
    assert r["pts_last"].dtype == np.float32 and np.array_equal(r["pts_last"], last[[7, 3, 2]])
    assert np.array_equal(r["pts_curr"], curr[[6, 2, 2]])
    d = last[[7, 3, 2]].astype(np.float64) - curr[[6, 2, 2]].astype(np.float64)
    assert abs(r["parallax"] - np.hypot(d[:, 0], d[:, 1]).sum() / 7) < 1e-12   # over all 7 kept matches
    assert track_ess_ref(m, last, curr, 8)["gate"] == 1 and track_ess_ref(m, last, curr, 8)["parallax"] == 0.0
    assert track_ess_ref(_m([(3, 3, 5.0), (2, 2, 6.0)]), last, curr, 1)["parallax"] == 5.0   # (3, 4) displacements


# ---------------------------------------------------------------------------- the composition
def _rot(q):
    return synth.quat_to_mat(np.asarray(q[:4]) / np.linalg.norm(q[:4]))


def test_compose_equals_the_matrix_product():
    rng = np.random.default_rng(5)
    for k in range(6):
        qa = synth.quat_from_rotvec(rng.normal(0, 1.0 + k, 3))
        qb = synth.quat_from_rotvec(rng.normal(0, 1.0 + k, 3))
        ta, tb = rng.normal(0, 2, 3), rng.normal(0, 2, 3)
        T = compose(np.concatenate([qa, ta]), np.concatenate([qb, tb]))
        Ra, Rb = _rot(qa), _rot(qb)
        assert np.abs(_rot(T) - Ra @ Rb).max() < 1e-14
        assert np.abs(T[4:] - (Ra @ tb + ta)).max() < 1e-14
        assert abs(np.linalg.norm(T[:4]) - 1.0) < 1e-15
    ident = np.array([0, 0, 0, 1.0, 0, 0, 0])
    T = np.concatenate([synth.quat_from_rotvec([0.3, -0.2, 0.1]), [1.0, 2.0, 3.0]])
    assert np.abs(compose(T, ident) - T).max() < 1e-15 and np.abs(compose(ident, T) - T).max() < 1e-15
    neg = np.concatenate([-T[:4], T[4:]])
    assert np.array_equal(compose(ident, neg)[:4], -compose(ident, T)[:4])


def test_renormalisation_is_first_order():
    """a product of norm^2 1 + e leaves as q * 2 / (2 + e): the norm error drops from e / 2 to about e^2 / 8"""
    a = np.array([0.0, 0.0, 0.0, 1.0 + 1e-4, 0, 0, 0])
    T = compose(a, np.array([0, 0, 0, 1.0, 0, 0, 0]))
    n2 = (1.0 + 1e-4) ** 2
    assert T[3] == (1.0 + 1e-4) * (2.0 / (1.0 + n2))
    assert abs(np.linalg.norm(T[:4]) - 1.0) < 1e-8   # e = 2e-4: e^2 / 8 = 5e-9, against e / 2 = 1e-4 before


def test_pose_from_Rt_takes_all_four_branches():
    cases = {"trace": [0.2, -0.1, 0.3], "x": [3.0, 0.1, -0.1], "y": [0.1, 3.0, -0.1], "z": [0.1, -0.1, 3.0]}
    seen = set()
    for name, v in cases.items():
        q = synth.quat_from_rotvec(np.array(v))
        R = synth.quat_to_mat(q)
        tr = R[0, 0] + R[1, 1] + R[2, 2]
        branch = "trace" if tr > 0 else "x" if R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2] else "y" if R[1, 1] > R[2, 2] else "z"
        assert branch == name
        seen.add(branch)
        T = pose_from_Rt(R.reshape(9), [1.0, -2.0, 0.5])
        assert np.abs(_rot(T) - R).max() < 1e-14 and list(T[4:]) == [1.0, -2.0, 0.5]
        assert abs(np.linalg.norm(T[:4]) - 1.0) < 1e-15
        assert min(np.abs(T[:4] - q).max(), np.abs(T[:4] + q).max()) < 1e-14
    assert seen == {"trace", "x", "y", "z"}


DRIVER = os.path.join(ROOT, "visionx-slam_amd", "build", "track_ess_driver")


def _driver(*args):
    if not os.path.exists(DRIVER):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "visionx-slam_amd"), "-j8"], check=True)
    out = subprocess.run([DRIVER, *args], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    return out.stdout.split()


def test_host_se3_product_is_the_restatement_bit_for_bit():
    """visionx::SE3d::operator*(const SE3d&) (host/include/visionx/types.h) against compose(), through
    hexadecimal floating-point text: no device involved"""
    rng = np.random.default_rng(11)
    for k in range(4):
        Ta = np.concatenate([synth.quat_from_rotvec(rng.normal(0, 1.0 + k, 3)), rng.normal(0, 2, 3)])
        Tb = np.concatenate([synth.quat_from_rotvec(rng.normal(0, 1.0 + k, 3)), rng.normal(0, 2, 3)])
        got = [float.fromhex(v) for v in _driver("compose", *[float(v).hex() for v in np.concatenate([Ta, Tb])])]
        assert np.array_equal(np.array(got), compose(Ta, Tb)), k


def test_tracker_rejects_positions_that_are_not_floats():
    assert _driver("narrow") == ["1"]


def test_last_frame_scene_is_what_the_matcher_would_return(oracle):
    s = synth.make_last_frame_scene(5, 128)
    m = oracle.match(s["desc_last"], s["desc_curr"])
    for k in ("query_idx", "train_idx", "distance"):
        assert np.array_equal(m[k], s["matches"][k]), k
    assert sorted(s["train_of"]) == list(range(128))
    assert s["last_xy"].dtype == s["curr_xy"].dtype == np.float32
    q = s["pose_last"][:4]
    assert abs(np.linalg.norm(q) - 1) < 1e-12 and q[3] < 0.999 and np.abs(s["pose_last"][4:]).max() > 0.1
    # the right matches are geometrically consistent with the true T_cl (a pixel or two of noise)
    tv = synth.make_two_view(5, 128)
    assert np.array_equal(s["last_xy"], tv["pts_last"]) and np.array_equal(s["curr_xy"][s["train_of"]], tv["pts_curr"])
