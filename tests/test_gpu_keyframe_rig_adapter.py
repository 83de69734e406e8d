"""KeyFrameLandmarks::CreateKeyFrameRig (visionx-slam_amd/host) through tests/cpp/keyframe_rig_driver against
the adapter that exists: after FrameTracker::TrackRig on three 300-feature cameras, ONE CreateKeyFrameRig in
one world and three KeyFrameLandmarks::CreateKeyFrame calls on a second identical setup.  Equality
throughout: the landmark lines of the host Map (ids, positions with 17 digits, observations), the feature
links of all six frames, landmark_id_ and the resident map's counts."""
import os
import subprocess

import numpy as np
import pytest

from vxslam import synth

from test_gpu_track_rig_adapter import dump

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "visionx-slam_amd", "build", "keyframe_rig_driver")
N = 300


def run(*args):
    assert os.path.exists(DRIVER), f"{DRIVER} missing: run __graft_entry__.build()"
    out = subprocess.run([DRIVER, *args], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return [line.split() for line in out.stdout.strip().splitlines()]


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    """three cameras that track with PnP; a third of every keyframe's features hold no landmark (the ones
    triangulation may fill); camera 2 has a depth image (2 m everywhere)"""
    path = str(tmp_path_factory.mktemp("kfrig"))
    for i in range(3):
        s = synth.make_track_frame_scene(301 + i, N)
        flags = s["flags"].copy()
        flags[::3] = 0
        dump(path, i, s, flags)
    d = os.path.join(path, "cam2")
    np.full((480, 640), 10000, np.uint16).tofile(os.path.join(d, "depth.bin"))
    np.array([480, 640], np.int64).tofile(os.path.join(d, "depth_shape.bin"))
    return path


def worlds(out):
    """the driver's lines per world, the world token dropped"""
    w = {"one": [], "each": []}
    for l in out:
        w[l[1]].append([l[0]] + l[2:])
    return w


def made(lines, first=50000000):
    """(created landmarks, those with two observations, those with one) of a world's landmark lines"""
    new = [l for l in lines if l[0] == "lm" and int(l[1]) >= first]
    return len(new), sum(len(l) == 7 for l in new), sum(len(l) == 6 for l in new)


def test_rig_call_equals_three_calls(scene_dir):
    w = worlds(run(scene_dir, "3", "rig"))
    a, b = w["one"], w["each"]
    nxt_a, nxt_b = a[0], b[0]
    assert nxt_a[0] == nxt_b[0] == "next"
    assert nxt_a[1] == nxt_b[1]                                   # landmark_id_
    assert [l for l in a if l[0] != "next"] == [l for l in b if l[0] != "next"]  # counts, landmarks, feature links
    assert sum(l[0] == "feat" for l in a) == 6 and sum(l[0] == "lm" for l in a) == 3 * N + made(a)[0]
    total, tri, dep = made(a)
    print("created", total, "triangulated", tri, "depth", dep)
    assert tri >= 1 and dep >= 1 and int(nxt_a[1]) == 50000000 + total
    # one rig call: its records are all cameras'; the last single call's are the last camera's
    assert int(nxt_a[2]) == total and int(nxt_b[2]) == int(nxt_b[3]) == int(nxt_a[3]) < total


def test_falls_back_pair_by_pair_without_a_list(scene_dir):
    """the last two pairs' last keyframes swapped: the tracker holds no list for them, so CreateKeyFrameRig runs
    CreateKeyFrame pair by pair — the same outcome, and LastRecords() is the last pair's only"""
    w = worlds(run(scene_dir, "3", "fallback"))
    a, b = w["one"], w["each"]
    assert a == b
    total = made(a)[0]
    assert total >= 1 and int(a[0][1]) == 50000000 + total
    assert int(a[0][2]) == int(a[0][3]) < total
