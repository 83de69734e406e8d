"""Tracking::UseRelocalisation and FrameTracker::Relocalize (visionx-slam_amd/host) through tests/cpp/reloc_driver, on
tests/test_gpu_frontend_adapter.py's sequence (synth.make_sequence, 14 frames of about 350 features, culling and
LocalBA enabled, garbage frame 9):
  * relocalisation off: every line the driver writes equals `frontend_driver sequence`'s process.txt, byte for byte
    (the default behaviour is unchanged: the frame after the garbage frame resets the map);
  * relocalisation on: the frame after the garbage frame relocalises, the keyframe and landmark counts of the map
    are those from before the failure, the state is TRACKING_GOOD, tracking goes on against the old map, and the
    pose bytes equal the C call's (vx_relocalize_async + vx_relocalize_fetch) on the same candidates, frame and map;
  * a sequence whose map cannot explain the frame (two garbage frames in a row) still ends in the reference's reset:
    every frame line equals the run without relocalisation."""
import os
import subprocess

import pytest

from vxslam import synth

import init_ref as R
from test_gpu_frontend_adapter import GARBAGE, H, INTR, W, dump_sequence, parse

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "visionx-slam_amd", "build")


def run(driver, *args):
    exe = os.path.join(BUILD, driver)
    assert os.path.exists(exe), f"{exe} missing: run __graft_entry__.build()"
    env = dict(os.environ, VX_BA_ATOMIC_ROWS="0")   # (LocalBA's row sums by slots: two runs are bitwise equal)
    out = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stderr


def read(path, name):
    return open(os.path.join(path, name)).read()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    path = tmp_path_factory.mktemp("reloc_sequence")
    dump_sequence(path, synth.make_sequence(5, 14, 350, width=W, height=H, intr=INTR, garbage=(GARBAGE,)))
    run("frontend_driver", "sequence", path)
    run("reloc_driver", "sequence", path, 0)
    run("reloc_driver", "sequence", path, 4)
    print(read(path, "reloc_4.txt"))
    return path


def test_off_is_the_default_behaviour(runs):
    a, b = read(runs, "process.txt"), read(runs, "reloc_0.txt")
    la, lb = a.splitlines(), b.splitlines()
    assert len(la) == len(lb) > 14
    for x, y in zip(la, lb):
        assert x == y
    assert a == b


def reloc_lines(path, name):
    out = {}
    for line in read(path, name).splitlines():
        t = line.split()
        if t[0] == "reloc":
            c = t.index("cands")
            s = t.index("cstatus")
            d = {t[i]: int(t[i + 1]) for i in range(2, c, 2)}
            d["cands"] = [int(x) for x in t[c + 1:s]]
            d["cstatus"] = int(t[s + 1])
            d["cpose"] = t[s + 3:s + 10]
            out[int(t[1])] = d
    return out


def frame_lines(path, name):
    return [l for l in read(path, name).splitlines() if l.startswith("frame ")]


def test_the_frame_after_the_failure_relocalises(runs):
    text = "\n".join(l for l in read(runs, "reloc_4.txt").splitlines() if not l.startswith("reloc "))
    frames, inits, final = parse_text(runs, text)
    by = {f["id"]: f for f in frames}
    off = {f["id"]: f for f in parse(os.path.join(runs, "reloc_0.txt"))[0]}
    # up to and including the garbage frame the run is the default one (resident frames change no line)
    on_lines, off_lines = frame_lines(runs, "reloc_4.txt"), frame_lines(runs, "reloc_0.txt")
    assert on_lines[:GARBAGE + 1] == off_lines[:GARBAGE + 1]
    g, r = by[GARBAGE], by[GARBAGE + 1]
    assert (g["call"], g["ok"], g["state"]) == (2, 0, R.TRACKING_BAD)
    assert off[GARBAGE + 1]["call"] == 3 and off[GARBAGE + 1]["live"] == [0, 0, 0]      # the default throws the map away
    # the frame after it relocalises: the map is the one from before the failure, the state is TRACKING_GOOD
    assert (r["call"], r["ok"], r["state"], r["kf"]) == (4, 1, R.TRACKING_GOOD, 0)
    assert r["live"] == by[GARBAGE - 1]["live"] and r["host"] == by[GARBAGE - 1]["host"] and r["live"][0] >= 3
    assert r["next_lm"] == g["next_lm"] and r["inliers"] >= 30
    rel = reloc_lines(runs, "reloc_4.txt")
    assert list(rel) == [GARBAGE + 1]
    x = rel[GARBAGE + 1]
    kf_ids = sorted(f["id"] for f in frames[:GARBAGE] if f["kf"] or f["call"] == 1) + [0]
    assert x["status"] == 0 and x["n_cand"] == len(x["cands"]) == min(4, r["live"][0])
    assert x["cands"] == sorted(x["cands"], reverse=True) and set(x["cands"]) <= set(kf_ids)   # the latest keyframes, latest first
    assert x["best_kf"] == x["cands"][x["best"]] and x["inliers"] == r["inliers"] and x["n_pool"] >= x["inliers"]
    # the pose is the C call's, byte for byte (hex strings of the seven doubles)
    assert x["cstatus"] == 0 and x["cpose"] == on_lines[GARBAGE + 1].split()[on_lines[GARBAGE + 1].split().index("pose") + 1:][:7]
    # tracking goes on against the old map: no second initialisation, no reset
    after = [f for f in frames if f["id"] > GARBAGE + 1]
    assert len(after) >= 2 and all(f["call"] == 2 and f["ok"] and f["state"] == R.TRACKING_GOOD for f in after)
    assert len(inits) == 1
    assert all(f["live"][0] >= r["live"][0] for f in after)
    # keyframes from before the failure are still in the final map; the default run's map holds none of them
    assert any(int(t[1]) < GARBAGE for t in final if t[0] == "kf")
    assert all(int(t[1]) > GARBAGE for t in parse(os.path.join(runs, "reloc_0.txt"))[2] if t[0] == "kf")


def parse_text(path, text):
    p = os.path.join(path, "reloc_4_frames.txt")
    open(p, "w").write(text + "\n")
    return parse(p)


def test_a_map_that_cannot_explain_the_frame_is_reset(tmp_path):
    dump_sequence(tmp_path, synth.make_sequence(5, 14, 350, width=W, height=H, intr=INTR, garbage=(GARBAGE, GARBAGE + 1)))
    run("reloc_driver", "sequence", tmp_path, 0)
    run("reloc_driver", "sequence", tmp_path, 4)
    on, off = read(tmp_path, "reloc_4.txt"), read(tmp_path, "reloc_0.txt")
    assert "reloc " not in on and on == off
    frames = parse(os.path.join(tmp_path, "reloc_4.txt"))[0]
    by = {f["id"]: f for f in frames}
    r = by[GARBAGE + 1]
    assert (r["call"], r["state"], r["live"], r["host"]) == (3, R.INIT, [0, 0, 0], [0, 0])
