"""Tracking::Track() for every camera of a rig time step in one call (vx_track_rig_async / vx_track_rig_fetch,
csrc/track_rig.hip) against the code that exists: vx_track_frame_async + vx_track_frame_fetch run camera by
camera on the same frames and the same map.  Never against the rig call itself.

Bar: equality throughout.  The rig call runs the single call's own program text per camera (the pair
kernels' bodies, the gate, the pose composition, the final block), the batched match is k_knn_rows' body per
pair, and both batched RANSACs are bit-exact per problem (their sample streams depend on the seed and the
hypothesis index only), so every fetched byte, both device match lists and the keypoint rows are the single
call's.

All cameras of a test live in ONE DMap: camera i's landmark ids are shifted by i * LM_SHIFT and its last
keyframe is keyframe KF0 + i."""
import ctypes as C

import numpy as np
import pytest

import vxslam
from vxslam import synth

pytestmark = pytest.mark.gpu

N = 300
KF0 = 100
LM_SHIFT = 100000
PNP, ESS, NONE = vxslam.TRACK_PATH_PNP, vxslam.TRACK_PATH_ESSENTIAL, vxslam.TRACK_PATH_NONE


def d2h(ctx, ptr, dtype, n):
    """n records of a device array (after the stream has drained)"""
    ctx.synchronize()
    out = np.zeros(max(n, 1), dtype)
    assert vxslam.lib().hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(out.nbytes), C.c_int(2)) == 0
    return out[:n]


def dev_list(ctx, triple):
    ptr, n_ptr, cap = triple
    n = int(d2h(ctx, n_ptr, np.int32, 1)[0])
    assert 0 <= n <= cap
    return d2h(ctx, ptr, vxslam.MATCH_DTYPE, n), cap


def few_flags(s, n=20):
    """has_landmark cleared until n right pairs remain (n < min_inliers: FEW_PAIRS)"""
    f = np.zeros(len(s["flags"]), np.uint8)
    f[np.nonzero(~s["wrong"])[0][:n]] = 1
    return f


class Cam:
    """one camera: its scene, its frames on the device, its share of the map"""

    def __init__(self, ctx, seed, n=N, wrong_frac=0.3, flags=None, kf=True, last=True, shared=False,
                 caps=None, up=None):
        up = up or ctx
        s = self.s = synth.make_track_frame_scene(seed, n, wrong_frac=wrong_frac)
        self.flags = s["flags"] if flags is None else (flags(s) if callable(flags) else flags)
        self.has_kf, self.has_last, self.shared = kf, last, shared
        ck, cl, cc = caps or (n + 20, n + 20, n + 23)
        if shared:  # the frame after a keyframe: the keyframe's descriptors at the last frame's pixels, ONE handle
            self.kf = self.last = vxslam.Frame(up, ck).upload(up, s["last_xy"], s["desc_kf"])
        else:
            self.kf = vxslam.Frame(up, ck).upload(up, s["kf_uv"].astype(np.float32), s["desc_kf"])
            self.last = vxslam.Frame(up, cl).upload(up, s["last_xy"], s["desc_last"])
        self.curr = vxslam.Frame(up, cc).upload(up, s["curr_xy"], s["desc_curr"])

    def close(self):
        for f in {id(f): f for f in (self.kf, self.last, self.curr)}.values():
            f.close()


def build_map(ctx, cams):
    dm = vxslam.DMap(ctx)
    for i, c in enumerate(cams):
        ids = c.s["lm_id"] + np.uint64(i * LM_SHIFT)
        dm.add_landmarks(ids, c.s["lm_pos"], None)
        dm.add_keyframe(KF0 + i, c.s["pose"], c.s["intr"], True, c.s["kf_uv"], ids, c.flags)
    return dm


def rig_cams(cams):
    return [vxslam.rig_camera(c.curr, c.s["intr"], last_kf_id=KF0 + i, last_kf=c.kf if c.has_kf else None,
                              last=c.last if c.has_last else None, pose_last=c.s["pose_last"])
            for i, c in enumerate(cams)]


def lists_of(ctx, cam, getter):
    out = []
    for which in (0, 1):
        if which == 0 and not cam.has_kf:
            with pytest.raises(vxslam.VxError) as e:
                getter(0)
            assert e.value.code == vxslam.VX_ERR_STATE
            out.append(None)
        else:
            out.append(dev_list(ctx, getter(which)))
    return out


def run_rig(ctx, dm, cams, opts, between=None):
    ctx.track_rig_async(dm, rig_cams(cams), opts)
    if between:
        between()
    got = ctx.track_rig_fetch()
    assert len(got) == len(cams)
    for i, c in enumerate(cams):
        got[i]["lists"] = lists_of(ctx, c, lambda w, i=i: ctx.track_rig_matches(i, w))
    return got


def run_single(ctx, dm, cams, opts):
    out = []
    for i, c in enumerate(cams):
        ctx.track_frame_async(dm if c.has_kf else None, KF0 + i, c.kf if c.has_kf else None,
                              c.last if c.has_last else None, c.curr, c.s["intr"], opts, pose_last=c.s["pose_last"])
        g = ctx.track_frame_fetch()
        g["lists"] = lists_of(ctx, c, ctx.track_frame_matches)
        out.append(g)
    return out


def blob(g):
    parts = [g["result"].tobytes(), g["pnp"][0].tobytes(), g["pnp"][1].tobytes(), g["ess"][0].tobytes(),
             g["ess"][1].tobytes(), g["keypoints"].tobytes()]
    for l in g["lists"]:
        parts.append(b"-" if l is None else l[0].tobytes() + b"|%d" % l[1])
    return tuple(parts)


def same(got, want, what=""):
    """every camera's fetched record, pair arrays and masks of both paths, both device match lists with
    their counts and capacities, and the keypoint rows: byte for byte"""
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        r = a["result"]
        print(what, "cam", i, "path", r["path"], "status", r["status"], "pnp", r["pnp"]["status"], r["pnp"]["n_pairs"],
              "ess", r["ess"]["status"], r["ess"]["n_pairs"], "inliers", r["n_inliers"], "ran", r["pnp_ran"], r["ess_ran"])
        assert r.tobytes() == b["result"].tobytes(), (i, r, b["result"])
        for path in ("pnp", "ess"):
            assert a[path][0].dtype == np.int32 and a[path][1].dtype == np.uint8
            assert np.array_equal(a[path][0], b[path][0]) and np.array_equal(a[path][1], b[path][1]), (i, path)
            assert len(a[path][0]) == r[path]["n_pairs"] == len(a[path][1])
        for which in (0, 1):
            la, lb = a["lists"][which], b["lists"][which]
            assert (la is None) == (lb is None), (i, which)
            if la is not None:
                assert la[1] == lb[1] and la[0].tobytes() == lb[0].tobytes(), (i, which, len(la[0]), len(lb[0]))
        assert a["keypoints"].tobytes() == b["keypoints"].tobytes() and len(a["keypoints"]) == r["n_keypoints"], i
        assert blob(a) == blob(b)


def paths(got):
    return [(int(g["result"]["path"]), int(g["result"]["pnp_ran"]), int(g["result"]["ess_ran"])) for g in got]


@pytest.fixture(scope="module")
def opts():
    return vxslam.track_frame_options(ess={"max_iterations": 200})


def close(dm, cams):
    dm.close()
    for c in cams:
        c.close()


# ---------------------------------------------------------------------------- one camera of each scenario
def test_mixed_rig(ctx, opts):
    cams = [Cam(ctx, 31),                                     # PnP succeeds
            Cam(ctx, 32, flags=few_flags),                    # FEW_PAIRS, the fallback succeeds
            Cam(ctx, 33, wrong_frac=1.0),                     # both paths fail
            Cam(ctx, 34, kf=False),                           # no last keyframe
            Cam(ctx, 35, flags=few_flags, last=False),        # no last frame, PnP failing
            Cam(ctx, 36, flags=few_flags, shared=True)]       # last_kf == last as one handle, PnP failing
    dm = build_map(ctx, cams)
    got = run_rig(ctx, dm, cams, opts)
    same(got, run_single(ctx, dm, cams, opts), "mixed")
    assert paths(got) == [(PNP, 1, 0), (ESS, 1, 1), (NONE, 1, 1), (ESS, 0, 1), (NONE, 1, 0), (ESS, 1, 1)]
    st = [int(g["result"]["pnp"]["status"]) for g in got]
    assert st == [vxslam.TRACK_OK, vxslam.TRACK_FEW_PAIRS, vxslam.TRACK_PNP_FAILED, 0, vxslam.TRACK_FEW_PAIRS,
                  vxslam.TRACK_FEW_PAIRS]
    assert got[2]["result"]["ess"]["status"] == vxslam.TRACK_ESSENTIAL_FAILED and got[2]["result"]["ess"]["ess"]["hypotheses_run"] > 0
    assert got[3]["result"]["pnp"].tobytes() == bytes(176) and got[4]["result"]["status"] == vxslam.TRACK_FEW_PAIRS
    assert got[0]["result"]["ess"]["n_matches"] == 0 and len(got[5]["lists"][1][0]) == N
    close(dm, cams)


# ---------------------------------------------------------------------------- the pack step's boundaries
def test_pack_boundaries(ctx, opts):
    """cameras with 0 pairs first, in the middle and last among cameras with pairs; one whose pair count equals
    its match capacity (frame capacity N exactly, every match kept and linked); heterogeneous capacities"""
    zero = lambda s: np.zeros(len(s["flags"]), np.uint8)
    cams = [Cam(ctx, 41, flags=zero, caps=(N + 3, N + 3, N)),
            Cam(ctx, 42, wrong_frac=0.0, caps=(N, N, N)),
            Cam(ctx, 43, caps=(N + 20, 2 * N, N + 20)),
            Cam(ctx, 44, flags=zero, caps=(2 * N, N, N + 3)),
            Cam(ctx, 45, caps=(2 * N, N + 3, 2 * N)),
            Cam(ctx, 46, flags=zero, caps=(N + 20, N + 20, N + 3))]
    dm = build_map(ctx, cams)
    got = run_rig(ctx, dm, cams, opts)
    same(got, run_single(ctx, dm, cams, opts), "pack")
    npairs = [int(g["result"]["pnp"]["n_pairs"]) for g in got]
    assert npairs[0] == npairs[3] == npairs[5] == 0 and npairs[1] == N == got[1]["lists"][0][1] and npairs[2] > 30 < npairs[4]
    assert paths(got) == [(ESS, 1, 1), (PNP, 1, 0), (PNP, 1, 0), (ESS, 1, 1), (PNP, 1, 0), (ESS, 1, 1)]
    assert got[1]["pnp"][1].sum() >= 30 and got[4]["pnp"][1].sum() >= 30  # masks unpacked behind a full / an empty camera
    close(dm, cams)


def test_chunk_boundary(ctx, opts):
    """N = 1024 and N = 1025 around trk::kBlock beside N = 300 cameras: a multi-chunk ordered compaction next
    to one-chunk ones, on both paths (the 1025 camera falls back)"""
    cams = [Cam(ctx, 51), Cam(ctx, 52, n=1024, caps=(1024, 1024, 1024)),
            Cam(ctx, 53, n=1025, flags=few_flags, caps=(1025, 1025, 1025)), Cam(ctx, 54, flags=few_flags)]
    dm = build_map(ctx, cams)
    got = run_rig(ctx, dm, cams, opts)
    same(got, run_single(ctx, dm, cams, opts), "chunk")
    assert paths(got) == [(PNP, 1, 0), (PNP, 1, 0), (ESS, 1, 1), (ESS, 1, 1)]
    assert got[1]["result"]["pnp"]["n_good_matches"] == 1024 and got[2]["result"]["ess"]["n_good_matches"] == 1025
    close(dm, cams)


def test_zero_count_after_the_buffers_grew(ctx, opts):
    """a large rig call grows the call's buffers; a smaller one then has a camera WITHOUT a last keyframe whose
    current frame is smaller than another camera's keyframe frame.  That camera's list-0 query count must be a
    device zero wherever the call's buffers now lie: its list-0 count slot is 0 (a non-zero query count would
    match its current rows against themselves and keep every one of them)"""
    big = [Cam(ctx, 120 + i, n=600, caps=(900, 900, 900)) for i in range(8)]
    dmb = build_map(ctx, big)
    run_rig(ctx, dmb, big, opts)
    close(dmb, big)
    cams = [Cam(ctx, 130, caps=(2 * N, N + 20, N + 20)), Cam(ctx, 131, kf=False, caps=(N, N, N)),
            Cam(ctx, 132, flags=few_flags, caps=(N + 3, N + 3, N + 3))]
    dm = build_map(ctx, cams)
    got = run_rig(ctx, dm, cams, opts)
    _, n_ptr0, _ = ctx.track_rig_matches(0, 0)
    slots = d2h(ctx, n_ptr0, np.int32, 12).reshape(3, 4)  # list 0's count of camera i: int32[4] at 16 i bytes
    print("list-0 count slots", slots[:, 0])
    assert slots[0, 0] == len(got[0]["lists"][0][0]) == N and slots[2, 0] == N and slots[1, 0] == 0
    same(got, run_single(ctx, dm, cams, opts), "zero")
    assert paths(got) == [(PNP, 1, 0), (ESS, 0, 1), (ESS, 1, 1)]
    close(dm, cams)


# ---------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("b", [1, 2, vxslam.MAX_RIG_CAMERAS])
def test_sizes(ctx, opts, b):
    cams = [Cam(ctx, 60 + i, flags=few_flags if i % 3 == 1 else None, kf=i % 5 != 4) for i in range(b)]
    dm = build_map(ctx, cams)
    got = run_rig(ctx, dm, cams, opts)
    same(got, run_single(ctx, dm, cams, opts), "B=%d" % b)
    assert [(p[1], p[2]) for p in paths(got)] == [(int(i % 5 != 4), int(i % 3 == 1 or i % 5 == 4)) for i in range(b)]
    close(dm, cams)


def test_sizes_outside_the_range(ctx, opts):
    cam = Cam(ctx, 60)
    dm = build_map(ctx, [cam])
    for b in (0, vxslam.MAX_RIG_CAMERAS + 1):
        with pytest.raises(vxslam.VxError) as e:
            ctx.track_rig_async(dm, rig_cams([cam]) * b, opts)
        assert e.value.code == vxslam.VX_ERR_INVALID
    close(dm, [cam])


# ---------------------------------------------------------------------------- every gate in one state
def test_all_gates_closed(ctx, opts):
    cams = [Cam(ctx, 70 + i) for i in range(4)]
    dm = build_map(ctx, cams)
    got = run_rig(ctx, dm, cams, opts)
    same(got, run_single(ctx, dm, cams, opts), "closed")
    assert paths(got) == [(PNP, 1, 0)] * 4
    # every essential record is the empty match list's
    c0 = cams[0].s
    ctx.track_essential_host_async(np.zeros((0, 32), np.uint8), np.zeros((0, 2), np.float32), c0["desc_curr"], c0["curr_xy"],
                                   c0["intr"], opts[1], pose_last=c0["pose_last"])
    empty = ctx.track_essential_fetch()[0]
    assert empty["n_matches"] == 0 and empty["ess"]["hypotheses_run"] == 0
    for g in got:
        assert g["result"]["ess"].tobytes() == empty.tobytes() and len(g["lists"][1][0]) == 0 and len(g["ess"][0]) == 0
    close(dm, cams)


def test_all_gates_open(ctx, opts):
    cams = [Cam(ctx, 74 + i, flags=few_flags) for i in range(4)]
    dm = build_map(ctx, cams)
    got = run_rig(ctx, dm, cams, opts)
    same(got, run_single(ctx, dm, cams, opts), "open")
    assert paths(got) == [(ESS, 1, 1)] * 4 and all(len(g["lists"][1][0]) == N for g in got)
    close(dm, cams)


def test_gate_boundary_of_one_camera(ctx):
    """min_inliers at camera 1's PnP inlier count and one above: exactly camera 1's gate flips, where the
    host rule flips (the other cameras have about 200 inliers)"""
    cams = [Cam(ctx, 80), Cam(ctx, 81, flags=lambda s: few_flags(s, 60)), Cam(ctx, 82)]
    dm = build_map(ctx, cams)
    base = vxslam.track_frame_options(ess={"max_iterations": 200})
    n_inl = int(run_rig(ctx, dm, cams, base)[1]["result"]["pnp"]["pnp"]["n_inliers"])
    print("camera 1 inliers", n_inl)
    assert 30 <= n_inl <= 60
    seen = []
    for mi in (n_inl, n_inl + 1):
        o = (vxslam.track_options(min_inliers=mi), base[1])
        got = run_rig(ctx, dm, cams, o)
        same(got, run_single(ctx, dm, cams, o), "min_inliers=%d" % mi)
        seen.append(paths(got))
    assert seen[0] == [(PNP, 1, 0)] * 3
    assert seen[1] == [(PNP, 1, 0), (ESS, 1, 1), (PNP, 1, 0)]
    close(dm, cams)


# ---------------------------------------------------------------------------- repeats, interference, ordering
def test_repeats_and_interference(ctx, opts):
    cams = [Cam(ctx, 90), Cam(ctx, 91, flags=few_flags), Cam(ctx, 92, kf=False)]
    other = Cam(ctx, 93, flags=few_flags)
    dm = build_map(ctx, cams + [other])
    runs = [[blob(g) for g in run_rig(ctx, dm, cams, opts)] for _ in range(3)]
    assert runs[0] == runs[1] == runs[2]
    pp = synth.make_pnp_problem(3, 200)
    tv = synth.make_two_view(4, 200)
    single = {}

    def between():  # a whole single-camera track and both RANSAC entry points between the rig's enqueue and fetch
        ctx.track_frame_async(dm, KF0 + 3, other.kf, other.last, other.curr, other.s["intr"], opts, pose_last=other.s["pose_last"])
        single["got"] = ctx.track_frame_fetch()
        ctx.pnp_ransac(pp["obj"], pp["img"], pp["intr"], vxslam.pnp_options(200))
        ctx.essential_ransac(tv["pts_last"], tv["pts_curr"], tv["intr"], vxslam.essential_options(max_iterations=100))

    assert [blob(g) for g in run_rig(ctx, dm, cams, opts, between=between)] == runs[0]
    # and the reverse: a rig call between the single call's enqueue and its fetch
    ctx.track_frame_async(dm, KF0 + 3, other.kf, other.last, other.curr, other.s["intr"], opts, pose_last=other.s["pose_last"])
    assert [blob(g) for g in run_rig(ctx, dm, cams, opts)] == runs[0]
    late = ctx.track_frame_fetch()
    for k in ("result", "keypoints"):
        assert late[k].tobytes() == single["got"][k].tobytes()
    assert late["result"]["path"] == ESS
    close(dm, cams + [other])


def test_frames_from_another_context(ctx, opts):
    """frames uploaded on a second context, ordered by vx_stream_wait_ctx only"""
    spec = [dict(seed=95), dict(seed=96, flags=few_flags)]
    cams = [Cam(ctx, **k) for k in spec]
    dm = build_map(ctx, cams)
    want = [blob(g) for g in run_rig(ctx, dm, cams, opts)]
    ctx2 = vxslam.Context(0)
    far = [Cam(ctx, up=ctx2, **k) for k in spec]
    ctx.wait_for(ctx2)
    assert [blob(g) for g in run_rig(ctx, dm, far, opts)] == want
    close(dm, cams + far)
    ctx2.close()


# ---------------------------------------------------------------------------- keyframe creation on the rig's list
def test_keyframe_on_the_rig_list(ctx, opts):
    """vx_dmap_create_keyframe_frame on vx_track_rig_matches(1, 0) against the same call on
    vx_track_frame_matches(0) after the single call: map, result record and landmark records"""
    def flags(s):
        f = s["flags"].copy()
        f[::3] = 0  # features without a landmark: the ones triangulation may fill
        return f

    cams = [Cam(ctx, 97), Cam(ctx, 98, flags=flags), Cam(ctx, 99)]
    maps = [build_map(ctx, cams), build_map(ctx, cams)]
    new_kf = KF0 + 50
    got = run_rig(ctx, maps[0], cams, opts)[1]
    assert got["result"]["path"] == PNP
    a = maps[0].create_keyframe_frame(new_kf, got["result"]["pose"], cams[1].s["intr"], cams[1].curr, last_kf_id=KF0 + 1,
                                      matches=ctx.track_rig_matches(1, 0), first_landmark_id=900000)
    c = cams[1]
    ctx.track_frame_async(maps[1], KF0 + 1, c.kf, c.last, c.curr, c.s["intr"], opts, pose_last=c.s["pose_last"])
    one = ctx.track_frame_fetch()
    assert one["result"].tobytes() == got["result"].tobytes()
    b = maps[1].create_keyframe_frame(new_kf, one["result"]["pose"], c.s["intr"], c.curr, last_kf_id=KF0 + 1,
                                      matches=ctx.track_frame_matches(0), first_landmark_id=900000)
    print("triangulated", a["result"]["n_triangulated"])
    assert a["result"].tobytes() == b["result"].tobytes() and a["landmarks"].tobytes() == b["landmarks"].tobytes()
    assert a["result"]["n_triangulated"] > 0 and maps[0].counts() == maps[1].counts()
    for x, y in zip(maps[0].download(), maps[1].download()):
        assert np.array_equal(x, y)
    for k in (KF0 + 1, new_kf):
        for x, y in zip(maps[0].keyframe_features(k), maps[1].keyframe_features(k)):
            assert np.array_equal(x, y)
    maps[1].close()
    close(maps[0], cams)


# ---------------------------------------------------------------------------- argument and state checks
def test_argument_and_state_checks(ctx, opts):
    L = vxslam.lib()
    fresh = vxslam.Context(0)
    out = np.zeros(4, vxslam.TRACK_FRAME_RESULT_DTYPE)
    po = C.c_void_p(out.ctypes.data)
    assert L.vx_track_rig_fetch(fresh.handle, 1, po, 4, None) == vxslam.VX_ERR_STATE  # fetch before enqueue
    assert L.vx_track_rig_matches(fresh.handle, 0, 1, None, None, None) == vxslam.VX_ERR_STATE
    assert L.vx_track_rig_pairs(fresh.handle, 0, 0, None, None, 0) == vxslam.VX_ERR_STATE
    assert L.vx_track_rig_block(fresh.handle, None, None, None, None, None, 0) == vxslam.VX_ERR_STATE
    fresh.close()
    cams = [Cam(ctx, 101), Cam(ctx, 102, kf=False)]
    dm = build_map(ctx, cams)
    good = rig_cams(cams)

    def bad(**kw):
        rc = good[:1] + [dict(good[1], **kw)]
        with pytest.raises(vxslam.VxError) as e:
            ctx.track_rig_async(dm, rc, opts)
        assert e.value.code == vxslam.VX_ERR_INVALID, kw

    bad(curr=None)                                       # a null curr
    bad(last=None)                                       # a camera with neither frame
    bad(last_kf=cams[1].kf, last_kf_id=KF0 + 77)         # a keyframe that is not in the map
    bad(intr=[0.0, 500.0, 1.0, 1.0])                     # zero focal length
    # (a frame of another device is not expressible on one GPU: the check is vx_track_frame_async's own line)
    with pytest.raises(vxslam.VxError) as e:             # a last keyframe without a map
        ctx.track_rig_async(None, good, opts)
    assert e.value.code == vxslam.VX_ERR_INVALID
    # as vx_track_frame_async: an enqueue refused for its arguments leaves the previous call's result in place
    ctx.track_rig_async(dm, good, opts)
    bad(curr=None)
    n = C.c_int(0)
    assert L.vx_track_rig_pairs(ctx.handle, 0, 0, None, None, 0) == vxslam.VX_ERR_STATE   # before the fetch
    assert L.vx_track_rig_fetch(ctx.handle, 1, po, 1, C.byref(n)) == vxslam.VX_ERR_CAPACITY and n.value == 2
    assert L.vx_track_rig_fetch(ctx.handle, 1, po, 4, C.byref(n)) == vxslam.VX_OK and n.value == 2
    assert out[0]["path"] == PNP and out[1]["path"] == ESS
    for cam in (-1, 2):                                  # cam out of range
        assert L.vx_track_rig_pairs(ctx.handle, cam, 0, None, None, 0) == vxslam.VX_ERR_INVALID
        assert L.vx_track_rig_matches(ctx.handle, cam, 1, None, None, None) == vxslam.VX_ERR_INVALID
        assert L.vx_track_rig_keypoints(ctx.handle, cam, None, 0, C.byref(n)) == vxslam.VX_ERR_INVALID
    assert L.vx_track_rig_matches(ctx.handle, 0, 2, None, None, None) == vxslam.VX_ERR_INVALID
    assert L.vx_track_rig_matches(ctx.handle, 1, 0, None, None, None) == vxslam.VX_ERR_STATE  # no last keyframe
    assert L.vx_track_rig_matches(ctx.handle, 0, 0, None, None, None) == vxslam.VX_OK
    pm = np.zeros(4, np.int32)
    assert L.vx_track_rig_pairs(ctx.handle, 0, 0, C.c_void_p(pm.ctypes.data), None, 4) == vxslam.VX_ERR_CAPACITY
    assert L.vx_track_rig_pairs(ctx.handle, 0, 1, C.c_void_p(pm.ctypes.data), None, 4) == vxslam.VX_OK  # no pairs
    kp = np.zeros(N, vxslam.KEYPOINT_DTYPE)
    assert L.vx_track_rig_keypoints(ctx.handle, 1, C.c_void_p(kp.ctypes.data), 8, C.byref(n)) == vxslam.VX_ERR_CAPACITY
    assert n.value == N
    assert L.vx_track_rig_keypoints(ctx.handle, 1, C.c_void_p(kp.ctypes.data), N, C.byref(n)) == vxslam.VX_OK
    assert kp.tobytes() == cams[1].curr.fetch(ctx, descriptors=False)[0].tobytes()
    # without the keypoint rows the records are the same and the rows are not available
    ctx.track_rig_async(dm, good, opts)
    out2 = np.zeros(2, vxslam.TRACK_FRAME_RESULT_DTYPE)
    assert L.vx_track_rig_fetch(ctx.handle, 0, C.c_void_p(out2.ctypes.data), 2, None) == vxslam.VX_OK
    assert out2.tobytes() == out[:2].tobytes()
    assert L.vx_track_rig_keypoints(ctx.handle, 0, None, 0, C.byref(n)) == vxslam.VX_ERR_STATE
    close(dm, cams)


# ---------------------------------------------------------------------------- it is really batched
# stages whose existing enqueue code already splits by grid size: ess_enqueue runs k_em_hyp in two launches
# with k_em_gate (an em_select launch) between when cameras x hypotheses exceeds what is resident at once
SPLIT_BY_GRID = ("em_hypotheses", "em_select")
NEW_STAGES = ("rig_pairs", "rig_pack", "rig_gate", "rig_epairs", "rig_epose", "rig_final")


def test_launch_counts_do_not_depend_on_the_cameras(ctx, opts):
    counts = {}
    for b in (2, 8):
        cams = [Cam(ctx, 110 + i, flags=few_flags if i % 2 else None) for i in range(b)]
        dm = build_map(ctx, cams)
        run_rig(ctx, dm, cams, opts)
        ctx.prof_enable(True)
        ctx.track_rig_async(dm, rig_cams(cams), opts)
        ctx.track_rig_fetch()
        prof = ctx.prof_read()
        ctx.prof_enable(False)
        counts[b] = {k: v[1] for k, v in prof.items() if v[1]}
        close(dm, cams)
    print(counts)
    for st in NEW_STAGES:
        assert counts[2].get(st, 0) >= 1, st
    assert counts[2]["rig_pack"] == 2 and all(counts[2][s] == 1 for s in NEW_STAGES if s != "rig_pack")
    for st in set(counts[2]) | set(counts[8]):
        if st not in SPLIT_BY_GRID:
            assert counts[2].get(st, 0) == counts[8].get(st, 0), st
    for b in (2, 8):  # the essential chain is ONE ess_enqueue either way: k_em_hyp once or twice, k_em_gate or not
        assert counts[b]["em_hypotheses"] in (1, 2) and counts[b]["em_select"] == 2 + counts[b]["em_hypotheses"], counts[b]
    for st in ("track_pairs", "track_epairs", "track_gate", "track_final", "frame_capture"):
        assert st not in counts[8], st
