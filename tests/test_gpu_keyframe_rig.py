"""Tracking::CreateKeyFrame for every camera of a rig step in one call (vx_dmap_create_keyframes_rig,
csrc/keyframe_rig.hip) against the code that exists, never against itself: two identically loaded
DMaps, map A takes the rig call, map B takes N vx_dmap_create_keyframe_frame calls in camera order on
the same frames, device match lists and depth images with the landmark ids carried.

Bars: the per-camera result records and the concatenated landmark records byte for byte (`pw`
included: both run the same program text under -ffp-contract=off), the maps equal
(test_gpu_keyframe.same_maps); map A against the numpy restatement (tests/keyframe_rig_ref.py) as
test_gpu_keyframe.same_records / same_state do: ids, rows, kinds and indices equal, depth points bit
for bit, triangulated points within 1e-9 relative."""
import numpy as np
import pytest

import vxslam
from vxslam import synth

import keyframe_ref as R
import keyframe_rig_ref as RR
import test_gpu_keyframe as K
import test_gpu_track_rig as T

pytestmark = pytest.mark.gpu

BLOCK = vxslam.keyframe_block()
NEW0 = 500  # the new keyframes' ids: NEW0 + camera

_scenes = {}


def scene300(i):
    """the i-th 300-feature scene (built once, never changed)"""
    if i not in _scenes:
        _scenes[i] = synth.make_keyframe_scene(6400 + i, 300)
    return _scenes[i]


class Rig:
    """one rig step: the map dict with a distinct last keyframe per camera, the cameras as the
    restatement takes them, and their frames and match lists on the device"""

    def __init__(self, ctx, scenes, depth=None, last=None, caps=None, seed=64):
        n = len(scenes)
        depth = [True] * n if depth is None else depth
        last = [True] * n if last is None else last
        self.m = synth.make_cull_scene(seed, 6, 300, special=False)
        base = int(self.m["kf_id"].max()) + 1
        self.lasts = RR.with_last_keyframes(self.m, scenes, base)
        self.cams = [RR.camera(d, NEW0 + i, self.lasts[i], depth=depth[i], last=last[i]) for i, d in enumerate(scenes)]
        self.first = int(self.m["lm_id"].max()) + 1
        self.caps = [max(len(d["uv2"]), 1) for d in scenes] if caps is None else caps
        self.frames = [vxslam.Frame(ctx, c).upload(ctx, d["uv2"].astype(np.float32), np.zeros((len(d["uv2"]), 32), np.uint8))
                       for c, d in zip(self.caps, scenes)]
        self.keep = []
        self.upload_lists()

    def upload_lists(self):
        """the cameras' match lists (as the restatement's cameras hold them now) to the device"""
        self.lists = []
        for k in self.cams:
            if k["last_kf_id"] is None:
                self.lists.append(None)
                continue
            mt = np.ascontiguousarray(k["matches"], vxslam.MATCH_DTYPE)
            a, b = K.dev(mt), K.dev(np.array([len(mt)], np.int32))
            self.keep += [a, b]
            self.lists.append((a.data_ptr(), b.data_ptr(), len(mt)))

    def ids(self):
        return self.lasts + [k["kf_id"] for k in self.cams]

    def rig_args(self):
        return [{"kf_id": k["kf_id"], "pose7": k["pose7"], "intr4": k["intr4"], "frame": f, "last_kf_id": k["last_kf_id"],
                 "matches": l, "depth": k["depth"]} for k, f, l in zip(self.cams, self.frames, self.lists)]

    def run_rig(self, dm, ctx=None, first=None):
        return dm.create_keyframes_rig(self.rig_args(), self.first if first is None else first, ctx=ctx)

    def run_single(self, dm, ctx=None, first=None):
        """N create_keyframe_frame calls in camera order, the ids carried: (results, all records)"""
        nxt = self.first if first is None else first
        res, recs = [], [np.zeros(0, vxslam.KEYFRAME_LANDMARK_DTYPE)]
        for k, f, l in zip(self.cams, self.frames, self.lists):
            g = dm.create_keyframe_frame(k["kf_id"], k["pose7"], k["intr4"], f, last_kf_id=k["last_kf_id"], matches=l,
                                         depth=k["depth"], first_landmark_id=nxt, ctx=ctx)
            res.append(g["result"])
            recs.append(g["landmarks"].copy())
            nxt = int(g["result"]["next_landmark_id"])
        return res, np.concatenate(recs)

    def close(self):
        for f in self.frames:
            f.close()
        self.keep = []


def slices(results):
    """camera i's slice of the concatenated records, from the results' counts"""
    n = [int(r["n_depth"]) + int(r["n_triangulated"]) for r in results]
    at = np.concatenate([[0], np.cumsum(n)])
    return [slice(int(at[i]), int(at[i + 1])) for i in range(len(n))]


def check(ctx, rig, label, ctx2=None, downstream=False):
    """the rig call on map A against the single calls on map B and against the restatement; returns
    the rig call's output"""
    a, b = K.loaded(ctx, rig.m), K.loaded(ctx, rig.m)
    got = rig.run_rig(a, ctx=ctx2)
    res_b, rec_b = rig.run_single(b, ctx=ctx2)
    assert len(got["results"]) == len(rig.cams)
    for i, r in enumerate(res_b):
        assert got["results"][i].tobytes() == r.tobytes(), (label, i, got["results"][i], r)
    assert got["landmarks"].tobytes() == rec_b.tobytes(), label
    K.same_maps(a, b, rig.ids())
    ref = rig.m.copy()
    want = RR.create_keyframes_rig(ref, rig.cams, rig.first, caps=rig.caps)
    assert want["error_bits"] == [0] * len(rig.cams)
    for i, s in enumerate(slices(got["results"])):
        assert got["results"][i]["first_landmark_id"] == want["first"][i]
        assert got["results"][i]["n_feat"] == len(rig.cams[i]["uv"])
        K.same_records({"result": got["results"][i], "landmarks": got["landmarks"][s]}, want["cameras"][i], f"{label} cam {i}:")
    assert int(got["results"][-1]["next_landmark_id"]) == want["next_landmark_id"]
    K.same_state(a, ref, got)
    if downstream:
        k = rig.cams[0]
        K.same_downstream(ctx, a, b, k["kf_id"], k["uv"], k["intr4"])
    a.close(), b.close()
    return got


def test_mixed_rig_of_four(ctx, slot_sums):
    """depth + last; no depth; no last keyframe; neither (zero landmarks)"""
    rig = Rig(ctx, [scene300(i) for i in range(4)], depth=[True, False, True, False], last=[True, True, False, False])
    got = check(ctx, rig, "mixed", downstream=True)
    r = got["results"]
    assert r[0]["n_depth"] >= 1 and r[0]["n_triangulated"] >= 1
    assert r[1]["n_depth"] == 0 and r[1]["n_triangulated"] >= 1
    assert r[2]["n_depth"] >= 1 and r[2]["n_triangulated"] == 0 and r[2]["n_matches"] == 0
    assert r[3]["n_depth"] == 0 and r[3]["n_triangulated"] == 0
    rig.close()


def test_empty_cameras_first_middle_and_last(ctx):
    """zero-feature and zero-landmark cameras first, in the middle and last"""
    z, f, g = R.scene(0, True), R.scene(65, True), R.scene(63, True)
    scenes = [z, f, f, g, z, f, z]
    #          zero features | full | zero landmarks | full | zero features | zero landmarks | zero features
    depth = [True, True, False, True, True, False, True]
    last = [True, True, False, True, True, False, False]
    rig = Rig(ctx, scenes, depth=depth, last=last)
    got = check(ctx, rig, "empty")
    made = [int(r["n_depth"]) + int(r["n_triangulated"]) for r in got["results"]]
    assert [r["n_feat"] for r in got["results"]] == [0, 65, 65, 63, 0, 65, 0]
    assert made[0] == made[2] == made[4] == made[5] == made[6] == 0
    for i in (1, 3):
        assert got["results"][i]["n_depth"] >= 1 and got["results"][i]["n_triangulated"] >= 1
    rig.close()


def test_chunk_boundaries(ctx):
    sizes = [BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 3, 65]
    rig = Rig(ctx, [R.scene(n, True) for n in sizes])
    got = check(ctx, rig, "chunks")
    for r in got["results"]:
        assert r["n_depth"] >= 1 and r["n_triangulated"] >= 1
    # more records than one commit chunk before the last cameras, so their bases cross a chunk's size
    assert sum(int(r["n_depth"]) + int(r["n_triangulated"]) for r in got["results"][:3]) > BLOCK
    rig.close()


@pytest.mark.parametrize("b", [1, 2, vxslam.MAX_RIG_CAMERAS])
def test_camera_counts(ctx, b):
    """B = 1 is the single call; B = 2 and B = 16 pass"""
    sizes = [300, 65, 63, 1]
    rig = Rig(ctx, [scene300(0) if i == 0 else R.scene(sizes[i % 4], True) for i in range(b)],
              depth=[i % 3 != 2 for i in range(b)], last=[i % 4 != 3 for i in range(b)])
    got = check(ctx, rig, f"B={b}")
    assert got["results"][0]["n_depth"] >= 1 and got["results"][0]["n_triangulated"] >= 1
    rig.close()


@pytest.mark.parametrize("b", [0, vxslam.MAX_RIG_CAMERAS + 1])
def test_camera_counts_refused(ctx, b):
    rig = Rig(ctx, [R.scene(1, True)] * max(b, 1))
    dm = K.loaded(ctx, rig.m)
    before = K.snapshot(dm, rig.lasts)
    with pytest.raises(vxslam.VxError) as e:
        dm.create_keyframes_rig(rig.rig_args()[:b], rig.first)
    assert e.value.code == vxslam.VX_ERR_INVALID
    K.same_snapshot(K.snapshot(dm, rig.lasts), before)
    dm.close()
    rig.close()


def test_frame_capacities(ctx):
    """capacities N, N + 3 and 2 N: the slices are capacity-strided, the rows count-strided"""
    rig = Rig(ctx, [scene300(i) for i in range(3)], caps=[300, 303, 600])
    got = check(ctx, rig, "caps")
    for r in got["results"]:
        assert r["n_feat"] == 300 and r["n_depth"] >= 1 and r["n_triangulated"] >= 1
    rig.close()


CASES = ["dup_query_last", "train_range_first", "repeat_last", "repeat_kf", "last_is_new", "id_range", "null_list"]


@pytest.mark.parametrize("case", CASES)
def test_rejected_input_leaves_the_map(ctx, case):
    """each refusal leaves the map as it was, and error_bits is set on exactly the faulty cameras"""
    rig = Rig(ctx, [scene300(0), R.scene(65, True), scene300(1)])
    good = [dict(k) for k in rig.cams]
    first, code = rig.first, vxslam.VX_ERR_INVALID
    if case == "dup_query_last":
        mt = rig.cams[2]["matches"].copy()
        mt["query_idx"][mt.size // 2] = mt["query_idx"][3]
        rig.cams[2]["matches"] = mt
    elif case == "train_range_first":
        mt = rig.cams[0]["matches"].copy()
        mt["train_idx"][mt.size - 1] = len(rig.cams[0]["uv"])
        rig.cams[0]["matches"] = mt
    elif case == "repeat_last":
        rig.cams[2]["last_kf_id"] = rig.cams[0]["last_kf_id"]
    elif case == "repeat_kf":
        rig.cams[1]["kf_id"] = rig.cams[0]["kf_id"]
    elif case == "last_is_new":
        rig.cams[1]["last_kf_id"] = rig.cams[2]["kf_id"]
    elif case == "id_range":
        first = int(rig.m["lm_id"].max()) - sum(rig.caps) + 1  # only the range's LAST id is in the map
    rig.upload_lists()
    want = RR.create_keyframes_rig(rig.m.copy(), rig.cams, first, caps=rig.caps)["error_bits"]
    expect = {"dup_query_last": [0, 0, vxslam.KF_ERR_DUP_QUERY], "train_range_first": [vxslam.KF_ERR_MATCH_RANGE, 0, 0],
              "repeat_last": [vxslam.KF_ERR_RIG_REPEAT, 0, vxslam.KF_ERR_RIG_REPEAT],
              "repeat_kf": [vxslam.KF_ERR_RIG_REPEAT, vxslam.KF_ERR_RIG_REPEAT, 0],
              "last_is_new": [0, vxslam.KF_ERR_NO_LAST, 0], "id_range": [vxslam.KF_ERR_ID_RANGE] * 3,
              "null_list": [0, 0, 0]}[case]
    assert want == expect
    if case == "null_list":  # has_last without a list: an argument error, no camera carries a bit
        rig.lists[1] = None
    dm = K.loaded(ctx, rig.m)
    before = K.snapshot(dm, rig.lasts)
    with pytest.raises(vxslam.VxError) as e:
        rig.run_rig(dm, first=first)
    assert e.value.code == code
    assert [int(x) for x in dm.last_create_rig["error_bits"]] == expect
    assert len(dm.create_results()) == 0
    for r in dm.last_create_rig:
        assert (r["n_depth"], r["n_triangulated"]) == (0, 0) and r["next_landmark_id"] == r["first_landmark_id"] == first
    K.same_snapshot(K.snapshot(dm, rig.lasts), before)
    # the good call afterwards gives what it gives on a fresh map
    rig.cams = good
    rig.upload_lists()
    ref = rig.m.copy()
    want = RR.create_keyframes_rig(ref, rig.cams, rig.first, caps=rig.caps)
    got = rig.run_rig(dm)
    for i, s in enumerate(slices(got["results"])):
        K.same_records({"result": got["results"][i], "landmarks": got["landmarks"][s]}, want["cameras"][i], f"after {case} cam {i}:")
    K.same_state(dm, ref, got)
    dm.close()
    rig.close()


def test_two_rig_calls_in_a_row(ctx):
    """step 1 creates frame 1 of two scenes against an earlier keyframe each; step 2 creates frame 2 against
    step 1's new keyframes, the landmark ids carried from call to call"""
    scenes = [scene300(2), scene300(3)]
    m = synth.make_cull_scene(65, 6, 300, special=False)
    base = int(m["kf_id"].max()) + 1
    step1 = []
    for i, d in enumerate(scenes):
        pose0, uv0, m01 = K.frame_before(d, 650 + i)
        R.with_last_keyframe(m, {"uv1": uv0, "has1": np.zeros(len(uv0), np.uint8), "pose1": pose0, "intr": d["intr"]}, base + i)
        step1.append({"kf_id": NEW0 + i, "pose7": d["pose1"], "intr4": d["intr"], "uv": d["uv1"], "last_kf_id": base + i,
                      "matches": m01, "depth": K.with_holes(d["depth"], d["uv1"], 660 + i)})
    step2 = [{"kf_id": NEW0 + 10 + i, "pose7": d["pose2"], "intr4": d["intr"], "uv": d["uv2"], "last_kf_id": NEW0 + i,
              "matches": d["matches"], "depth": d["depth"] if i == 0 else None} for i, d in enumerate(scenes)]
    rig = Rig.__new__(Rig)
    rig.m, rig.lasts, rig.caps, rig.keep = m, [base, base + 1], [300, 300], []
    rig.first = int(m["lm_id"].max()) + 1
    a, b = K.loaded(ctx, m), K.loaded(ctx, m)
    ref = m.copy()
    first = rig.first
    for step, cams, key in ((1, step1, "uv1"), (2, step2, "uv2")):
        rig.cams = cams
        rig.frames = [vxslam.Frame(ctx, 300).upload(ctx, d[key].astype(np.float32), np.zeros((300, 32), np.uint8)) for d in scenes]
        rig.upload_lists()
        want = RR.create_keyframes_rig(ref, cams, first, caps=rig.caps)
        assert want["error_bits"] == [0, 0]
        got = rig.run_rig(a, first=first)
        res_b, rec_b = rig.run_single(b, first=first)
        assert [r.tobytes() for r in got["results"]] == [r.tobytes() for r in res_b]
        assert got["landmarks"].tobytes() == rec_b.tobytes()
        assert got["results"][0]["first_landmark_id"] == first
        for i, s in enumerate(slices(got["results"])):
            K.same_records({"result": got["results"][i], "landmarks": got["landmarks"][s]}, want["cameras"][i], f"step {step} cam {i}:")
            assert got["results"][i]["n_triangulated"] >= 1
        assert got["results"][0]["n_depth"] >= 1
        K.same_state(a, ref, got)
        first = int(got["results"][-1]["next_landmark_id"])
        assert first == want["next_landmark_id"]
        rig.close()
    K.same_maps(a, b, [base, base + 1, NEW0, NEW0 + 1, NEW0 + 10, NEW0 + 11])
    a.close(), b.close()


def test_a_second_context(ctx):
    """the call on a context other than the map's waits for the map's stream first"""
    rig = Rig(ctx, [scene300(0), R.scene(65, True)])
    ctx2 = vxslam.Context(0)
    got = check(ctx, rig, "ctx2", ctx2=ctx2)
    assert got["results"][0]["n_triangulated"] >= 1
    ctx2.close()
    rig.close()


def test_the_rig_tracks_own_lists(ctx):
    """after track_rig_async on 3 cameras, track_rig_matches(i, 0) feeds the call"""
    def flags(s):
        f = s["flags"].copy()
        f[::3] = 0  # features without a landmark: the ones triangulation may fill
        return f

    cams = [T.Cam(ctx, 197, flags=flags), T.Cam(ctx, 198, flags=flags), T.Cam(ctx, 199)]
    maps = [T.build_map(ctx, cams), T.build_map(ctx, cams)]
    opts = vxslam.track_frame_options(ess={"max_iterations": 200})
    ctx.track_rig_async(maps[0], T.rig_cams(cams), opts)
    tr = ctx.track_rig_fetch()
    assert all(int(t["result"]["status"]) == vxslam.TRACK_OK for t in tr)
    depth = np.full((480, 640), 10000, np.uint16)  # 2 m everywhere
    args = [{"kf_id": NEW0 + i, "pose7": tr[i]["result"]["pose"], "intr4": c.s["intr"], "frame": c.curr,
             "last_kf_id": T.KF0 + i, "matches": ctx.track_rig_matches(i, 0), "depth": depth if i == 2 else None}
            for i, c in enumerate(cams)]
    got = maps[0].create_keyframes_rig(args, 900000)
    nxt, res, recs = 900000, [], []
    for k in args:
        g = maps[1].create_keyframe_frame(k["kf_id"], k["pose7"], k["intr4"], k["frame"], last_kf_id=k["last_kf_id"],
                                          matches=k["matches"], depth=k["depth"], first_landmark_id=nxt)
        res.append(g["result"])
        recs.append(g["landmarks"].copy())
        nxt = int(g["result"]["next_landmark_id"])
    assert [r.tobytes() for r in got["results"]] == [r.tobytes() for r in res]
    assert got["landmarks"].tobytes() == np.concatenate(recs).tobytes()
    print("track lists:", [(int(r["n_depth"]), int(r["n_triangulated"])) for r in res])
    assert res[0]["n_triangulated"] >= 1 and res[1]["n_triangulated"] >= 1 and res[2]["n_depth"] >= 1
    K.same_maps(maps[0], maps[1], [T.KF0 + i for i in range(3)] + [NEW0 + i for i in range(3)])
    maps[1].close()
    T.close(maps[0], cams)


def test_launch_counts_do_not_depend_on_the_cameras(ctx):
    stages = ["rig_kf_feat", "rig_kf_match", "rig_kf_count", "rig_kf_commit"]
    counts = {}
    for b in (2, 8):
        rig = Rig(ctx, [R.scene(65, True)] * b)
        dm = K.loaded(ctx, rig.m)
        ctx.prof_enable(True, stages)
        rig.run_rig(dm)
        p = ctx.prof_read()
        ctx.prof_enable(False)
        counts[b] = [int(p[s][1]) for s in stages]
        for s in stages:
            assert p[s][0] > 0.0, (s, p[s])
        dm.close()
        rig.close()
    assert counts[2] == counts[8] == [1, 1, 1, 1]
