"""Tracking::Track() in one call over device-resident frames (vx_track_frame_async / vx_track_frame_fetch,
csrc/track_frame.hip) against the code that exists: vx_track_pnp_host_async + fetch and
vx_track_essential_host_async + fetch on the same host arrays, composed as FrameTracker::Track composes
them (tests/track_frame_ref.py, pinned by tests/test_track_frame_cpu.py).

Bars: equality throughout.  The call runs the same kernels on the same rows as the two host-input calls
(the uploaded frames hold exactly the arrays those calls stage), so the embedded records, pair arrays,
masks and match lists are byte for byte theirs; the head is copied from them on the device."""
import ctypes as C

import numpy as np
import pytest

import vxslam
from vxslam import synth

from track_frame_ref import track_frame_ref

pytestmark = pytest.mark.gpu

KF = 7
N = 300


def dev(a):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def d2h(ctx, ptr, dtype, n):
    """n records of a device array (after the stream has drained)"""
    ctx.synchronize()
    out = np.zeros(max(n, 1), dtype)
    assert vxslam.lib().hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(out.nbytes), C.c_int(2)) == 0
    return out[:n]


def match_list(ctx, which):
    ptr, n_ptr, cap = ctx.track_frame_matches(which)
    n = int(d2h(ctx, n_ptr, np.int32, 1)[0])
    assert 0 <= n <= cap
    return d2h(ctx, ptr, vxslam.MATCH_DTYPE, n)


def load(ctx, s, flags=None):
    dm = vxslam.DMap(ctx)
    dm.add_landmarks(s["lm_id"], s["lm_pos"], None)
    dm.add_keyframe(KF, s["pose"], s["intr"], True, s["kf_uv"], s["lm_id"], s["flags"] if flags is None else flags)
    return dm


class Scene:
    """one scene's frames on the device and the yardstick calls on its host arrays"""

    def __init__(self, ctx, s, up=None, cap=N + 20):
        up = up or ctx
        self.s = s
        self.kf = vxslam.Frame(up, cap).upload(up, s["kf_uv"].astype(np.float32), s["desc_kf"])
        self.last = vxslam.Frame(up, cap).upload(up, s["last_xy"], s["desc_last"])
        self.curr = vxslam.Frame(up, cap + 3).upload(up, s["curr_xy"], s["desc_curr"])

    def close(self):
        for f in (self.kf, self.last, self.curr):
            f.close()

    def yardstick(self, ctx, dm, opts, kf=True, last=True, last_rows=None):
        """(pnp, ess, empty): the (record, pair_match, mask) of each existing call, None where Track() would
        not have the frame; `empty` is vx_track_essential_* on an empty match list"""
        s, (po, eo) = self.s, opts
        pnp = ess = None
        if kf:
            ctx.track_pnp_host_async(dm, KF, s["desc_kf"], s["desc_curr"], s["curr_xy"], s["intr"], po)
            pnp = ctx.track_pnp_fetch()
        ld, lxy = last_rows or (s["desc_last"], s["last_xy"])
        if last:
            ctx.track_essential_host_async(ld, lxy, s["desc_curr"], s["curr_xy"], s["intr"], eo, pose_last=s["pose_last"])
            ess = ctx.track_essential_fetch()
        ctx.track_essential_host_async(np.zeros((0, 32), np.uint8), np.zeros((0, 2), np.float32), s["desc_curr"], s["curr_xy"],
                                       s["intr"], eo, pose_last=s["pose_last"])
        empty = ctx.track_essential_fetch()
        assert empty[0]["n_matches"] == 0 and empty[0]["ess"]["ok"] == 0 and empty[0]["ess"]["hypotheses_run"] == 0
        return pnp, ess, empty

    def run(self, ctx, dm, opts, kf=True, last=True, last_frame=None, between=None):
        s = self.s
        ctx.track_frame_async(dm if kf else None, KF, self.kf if kf else None,
                              (last_frame or self.last) if last else None, self.curr, s["intr"], opts,
                              pose_last=s["pose_last"])
        if between:
            between()
        return ctx.track_frame_fetch()


def check(ctx, sc, got, yard, opts, kf=True, last=True, last_desc=None):
    """the whole fetched result against the yardstick; returns the head"""
    pnp, ess, empty = yard
    s, res = sc.s, got["result"]
    want = track_frame_ref(None if pnp is None else pnp[0], None if ess is None else ess[0], opts[0], opts[1],
                           n_keypoints=len(s["curr_xy"]), empty_ess=empty[0])
    print("path", res["path"], "status", res["status"], "pnp", res["pnp"]["status"], "ess", res["ess"]["status"],
          "inliers", res["n_inliers"], "ran", res["pnp_ran"], res["ess_ran"])
    if pnp is not None:  # the embedded PnP record, pair_match and mask: the PnP call's
        assert res["pnp"].tobytes() == pnp[0].tobytes()
        assert np.array_equal(got["pnp"][0], pnp[1]) and np.array_equal(got["pnp"][1], pnp[2])
        assert np.array_equal(match_list(ctx, 0), ctx.match(s["desc_kf"], s["desc_curr"]))
    else:
        assert res["pnp"].tobytes() == bytes(176) and len(got["pnp"][0]) == 0
    ran = bool(want["ess_ran"])
    src = ess if ran else empty  # the essential call's record, or the empty match list's
    assert res["ess"].tobytes() == src[0].tobytes()
    assert np.array_equal(got["ess"][0], src[1]) and np.array_equal(got["ess"][1], src[2])
    q = (s["desc_last"] if last_desc is None else last_desc) if ran else np.zeros((0, 32), np.uint8)
    assert np.array_equal(match_list(ctx, 1), ctx.match(q, s["desc_curr"]))
    assert res.tobytes() == want.tobytes(), (res, want)
    # the keypoints the fetch brought down are the frame's
    k, _ = sc.curr.fetch(ctx, descriptors=False)
    assert got["keypoints"].tobytes() == k.tobytes() and len(k) == len(s["curr_xy"])
    return res


@pytest.fixture(scope="module")
def scene(ctx):
    sc = Scene(ctx, synth.make_track_frame_scene(21, N, wrong_frac=0.3))
    yield sc
    sc.close()


@pytest.fixture(scope="module")
def opts():
    return vxslam.track_frame_options(ess={"max_iterations": 200})


@pytest.fixture(scope="module")
def few_flags(scene):
    """has_landmark cleared until 20 (< min_inliers) pairs remain: FEW_PAIRS"""
    f = np.zeros(N, np.uint8)
    f[np.nonzero(~scene.s["wrong"])[0][:20]] = 1
    return f


# ---------------------------------------------------------------------------- the six scenarios
def test_a_pnp_succeeds_gate_closed(ctx, scene, opts):
    dm = load(ctx, scene.s)
    res = check(ctx, scene, scene.run(ctx, dm, opts), scene.yardstick(ctx, dm, opts), opts)
    assert (res["path"], res["status"], res["ess_ran"]) == (vxslam.TRACK_PATH_PNP, vxslam.TRACK_OK, 0)
    assert res["ess"]["n_matches"] == 0 and res["ess"]["ess"]["ok"] == 0 and res["ess"]["ess"]["hypotheses_run"] == 0
    assert res["n_inliers"] >= 30 and np.abs(res["pose"] - scene.s["pose"]).max() < 5e-3
    dm.close()


def test_b_few_pairs_falls_back(ctx, scene, opts, few_flags):
    dm = load(ctx, scene.s, few_flags)
    res = check(ctx, scene, scene.run(ctx, dm, opts), scene.yardstick(ctx, dm, opts), opts)
    assert res["pnp"]["status"] == vxslam.TRACK_FEW_PAIRS and res["pnp"]["n_pairs"] == 20
    assert (res["path"], res["status"], res["ess_ran"]) == (vxslam.TRACK_PATH_ESSENTIAL, vxslam.TRACK_OK, 1)
    assert res["ess"]["n_matches"] == N and res["n_inliers"] == res["ess"]["ess"]["n_inliers"] >= 30
    dm.close()


def test_c_few_matches_on_both_paths(ctx, scene):
    o = vxslam.track_frame_options(min_matches=N + 1, ess={"max_iterations": 200})
    dm = load(ctx, scene.s)
    res = check(ctx, scene, scene.run(ctx, dm, o), scene.yardstick(ctx, dm, o), o)
    assert res["pnp"]["n_good_matches"] == N == res["ess"]["n_good_matches"]
    assert res["pnp"]["status"] == res["ess"]["status"] == res["status"] == vxslam.TRACK_FEW_MATCHES
    assert (res["path"], res["ess_ran"]) == (vxslam.TRACK_PATH_NONE, 1) and res["ess"]["ess"]["hypotheses_run"] == 0
    dm.close()


def test_d_no_last_keyframe(ctx, scene, opts):
    got = scene.run(ctx, None, opts, kf=False)
    res = check(ctx, scene, got, scene.yardstick(ctx, None, opts, kf=False), opts, kf=False)
    assert (res["pnp_ran"], res["ess_ran"], res["path"]) == (0, 1, vxslam.TRACK_PATH_ESSENTIAL)
    with pytest.raises(vxslam.VxError) as e:
        ctx.track_frame_matches(0)
    assert e.value.code == vxslam.VX_ERR_STATE


def test_e_no_last_frame_with_pnp_failing(ctx, scene, opts, few_flags):
    dm = load(ctx, scene.s, few_flags)
    got = scene.run(ctx, dm, opts, last=False)
    res = check(ctx, scene, got, scene.yardstick(ctx, dm, opts, last=False), opts, last=False)
    assert (res["pnp_ran"], res["ess_ran"], res["path"], res["status"]) == (1, 0, vxslam.TRACK_PATH_NONE, vxslam.TRACK_FEW_PAIRS)
    dm.close()


def test_f_all_wrong_matches_fail_both(ctx, opts):
    sc = Scene(ctx, synth.make_track_frame_scene(22, N, wrong_frac=1.0))
    dm = load(ctx, sc.s)
    res = check(ctx, sc, sc.run(ctx, dm, opts), sc.yardstick(ctx, dm, opts), opts)
    assert res["pnp"]["status"] == vxslam.TRACK_PNP_FAILED and res["ess"]["status"] == vxslam.TRACK_ESSENTIAL_FAILED
    assert (res["path"], res["status"], res["ess_ran"]) == (vxslam.TRACK_PATH_NONE, vxslam.TRACK_ESSENTIAL_FAILED, 1)
    assert res["ess"]["ess"]["hypotheses_run"] > 0 and not res["pose"].any()
    dm.close()
    sc.close()


# ---------------------------------------------------------------------------- the gate's boundaries
def test_gate_boundaries(ctx, scene):
    """min_matches at the kept count and one above; min_inliers at n_pairs and one above, and at
    pnp.n_inliers and one above: on each side the embedded status and the path are the host rule's"""
    s = scene.s
    flags = np.zeros(N, np.uint8)
    flags[np.nonzero(~s["wrong"])[0][:60]] = 1  # 60 pairs, all of them right matches
    dm = load(ctx, s, flags)
    base = vxslam.track_frame_options(ess={"max_iterations": 200})
    r0 = scene.run(ctx, dm, base)["result"]
    n_good, n_pairs, n_inl = int(r0["pnp"]["n_good_matches"]), int(r0["pnp"]["n_pairs"]), int(r0["pnp"]["pnp"]["n_inliers"])
    print("kept", n_good, "pairs", n_pairs, "inliers", n_inl)
    assert r0["path"] == vxslam.TRACK_PATH_PNP and n_good == N and n_pairs == 60 and 30 <= n_inl <= 60
    seen = {}
    for name, kw in (("mm", dict(min_matches=n_good)), ("mm+1", dict(min_matches=n_good + 1)),
                     ("np", dict(min_inliers=n_pairs)), ("np+1", dict(min_inliers=n_pairs + 1)),
                     ("ni", dict(min_inliers=n_inl)), ("ni+1", dict(min_inliers=n_inl + 1))):
        po = vxslam.track_options(**kw)
        o = (po, base[1])
        res = check(ctx, scene, scene.run(ctx, dm, o), scene.yardstick(ctx, dm, o), o)
        seen[name] = (int(res["pnp"]["status"]), int(res["path"]))
    OKP = (vxslam.TRACK_OK, vxslam.TRACK_PATH_PNP)
    assert seen["mm"] == OKP and seen["mm+1"] == (vxslam.TRACK_FEW_MATCHES, vxslam.TRACK_PATH_ESSENTIAL)
    assert seen["np"][0] != vxslam.TRACK_FEW_PAIRS and seen["np+1"] == (vxslam.TRACK_FEW_PAIRS, vxslam.TRACK_PATH_ESSENTIAL)
    assert seen["ni"] == OKP and seen["ni+1"][0] in (vxslam.TRACK_PNP_FAILED, vxslam.TRACK_FEW_PAIRS)
    assert seen["ni+1"][1] == vxslam.TRACK_PATH_ESSENTIAL
    dm.close()


# ---------------------------------------------------------------------------- other checks
def blob(got):
    return (got["result"].tobytes(), got["pnp"][0].tobytes(), got["pnp"][1].tobytes(), got["ess"][0].tobytes(),
            got["ess"][1].tobytes(), got["keypoints"].tobytes())


def test_same_handle_as_keyframe_and_last_frame(ctx, scene, opts, few_flags):
    """last_kf == last (the frame after a keyframe) reuses the first match list under a gated count: the
    results are those of two distinct handles holding the same rows, gate open (few pairs) and closed.
    The shared frame holds the keyframe's descriptors at the last frame's pixels, so the fallback passes."""
    s = scene.s
    rows = (s["desc_kf"], s["last_xy"])
    both = vxslam.Frame(ctx, scene.kf.cap).upload(ctx, rows[1], rows[0])
    twin = vxslam.Frame(ctx, scene.kf.cap).upload(ctx, rows[1], rows[0])
    for flags, path in ((few_flags, vxslam.TRACK_PATH_ESSENTIAL), (None, vxslam.TRACK_PATH_PNP)):
        dm = load(ctx, s, flags)

        def run(kf_frame, last_frame):
            ctx.track_frame_async(dm, KF, kf_frame, last_frame, scene.curr, s["intr"], opts, pose_last=s["pose_last"])
            return ctx.track_frame_fetch()

        one = run(both, both)
        m1 = match_list(ctx, 1)
        check(ctx, scene, one, scene.yardstick(ctx, dm, opts, last_rows=rows), opts, last_desc=rows[0])
        two = run(both, twin)
        assert one["result"]["path"] == path
        assert blob(one) == blob(two)
        assert np.array_equal(m1, match_list(ctx, 1)) and len(m1) == (N if flags is not None else 0)
        dm.close()
    both.close()
    twin.close()


def test_repeats_and_ransac_in_between(ctx, scene, opts, few_flags):
    dm = load(ctx, scene.s, few_flags)
    runs = [blob(scene.run(ctx, dm, opts)) for _ in range(3)]
    assert runs[0] == runs[1] == runs[2]
    pp = synth.make_pnp_problem(3, 200)
    tv = synth.make_two_view(4, 200)

    def between():
        ctx.pnp_ransac(pp["obj"], pp["img"], pp["intr"], vxslam.pnp_options(200))
        ctx.essential_ransac(tv["pts_last"], tv["pts_curr"], tv["intr"], vxslam.essential_options(max_iterations=100))

    assert blob(scene.run(ctx, dm, opts, between=between)) == runs[0]
    dm.close()


def test_frames_from_another_context(ctx, scene, opts, few_flags):
    """frames uploaded on a second context and tracked on the map's context with only a stream wait between"""
    ctx2 = vxslam.Context(0)
    dm = load(ctx, scene.s, few_flags)
    want = blob(scene.run(ctx, dm, opts))
    other = Scene(ctx, scene.s, up=ctx2)
    ctx.wait_for(ctx2)
    assert blob(other.run(ctx, dm, opts)) == want
    dm.close()
    other.close()
    ctx2.close()


def test_frames_captured_on_another_context(ctx, opts):
    """k_frame_capture on a second context (two real extractions), then the track on this one with only a
    stream wait between: the same record as with frames captured on this context"""
    imgs = synth.make_frames(0x5EED0051, 2, 240, 320)
    p = vxslam.default_orb_params(n_features=400)
    d = dev(imgs)

    def captured(c):
        fr = []
        for k in range(2):
            c.orb_extract_async(d[k].data_ptr(), 320, 240, 3, 960, k, p)
            fr.append(vxslam.Frame(c, 1024).capture(c, k))
        return fr

    def run(fr):
        ctx.track_frame_async(None, 0, None, fr[0], fr[1], [260.0, 260.0, 160.0, 120.0], opts)
        return ctx.track_frame_fetch()

    want = run(captured(ctx))
    assert want["result"]["ess_ran"] == 1 and want["result"]["ess"]["n_matches"] >= 50 and len(want["keypoints"]) >= 300
    ctx2 = vxslam.Context(0)
    fr = captured(ctx2)
    ctx.wait_for(ctx2)
    assert blob(run(fr)) == blob(want)
    for f in fr:
        f.close()
    ctx2.close()


def test_argument_and_state_checks(ctx, scene, opts):
    L, s = vxslam.lib(), scene.s
    fresh = vxslam.Context(0)
    out = np.zeros(1, vxslam.TRACK_FRAME_RESULT_DTYPE)
    assert L.vx_track_frame_fetch(fresh.handle, C.c_void_p(out.ctypes.data), None, 0, None) == vxslam.VX_ERR_STATE
    assert L.vx_track_frame_matches(fresh.handle, 1, None, None, None) == vxslam.VX_ERR_STATE
    assert L.vx_track_frame_pairs(fresh.handle, 0, None, None, 0) == vxslam.VX_ERR_STATE
    assert L.vx_track_frame_matches(fresh.handle, 2, None, None, None) == vxslam.VX_ERR_INVALID
    fresh.close()
    dm = load(ctx, s)
    with pytest.raises(vxslam.VxError) as e:  # neither a keyframe nor a last frame
        ctx.track_frame_async(dm, KF, None, None, scene.curr, s["intr"], opts)
    assert e.value.code == vxslam.VX_ERR_INVALID
    with pytest.raises(vxslam.VxError) as e:  # not a keyframe of the map
        ctx.track_frame_async(dm, KF + 1, scene.kf, scene.last, scene.curr, s["intr"], opts)
    assert e.value.code == vxslam.VX_ERR_INVALID
    with pytest.raises(vxslam.VxError) as e:  # a keyframe without a map
        ctx.track_frame_async(None, KF, scene.kf, scene.last, scene.curr, s["intr"], opts)
    assert e.value.code == vxslam.VX_ERR_INVALID
    with pytest.raises(vxslam.VxError) as e:  # zero focal length
        ctx.track_frame_async(dm, KF, scene.kf, scene.last, scene.curr, [0.0, 500.0, 1.0, 1.0], opts)
    assert e.value.code == vxslam.VX_ERR_INVALID
    # a failed enqueue leaves nothing to fetch
    assert L.vx_track_frame_fetch(ctx.handle, C.c_void_p(out.ctypes.data), None, 0, None) == vxslam.VX_ERR_STATE
    # capacities of the fetch
    ctx.track_frame_async(dm, KF, scene.kf, scene.last, scene.curr, s["intr"], opts, pose_last=s["pose_last"])
    kp = np.zeros(8, vxslam.KEYPOINT_DTYPE)
    n = C.c_int(0)
    assert L.vx_track_frame_fetch(ctx.handle, C.c_void_p(out.ctypes.data), C.c_void_p(kp.ctypes.data), 8, C.byref(n)) == vxslam.VX_ERR_CAPACITY
    assert n.value == N and out[0]["path"] == vxslam.TRACK_PATH_PNP
    pm = np.zeros(4, np.int32)
    assert L.vx_track_frame_pairs(ctx.handle, 0, C.c_void_p(pm.ctypes.data), None, 4) == vxslam.VX_ERR_CAPACITY
    assert L.vx_track_frame_pairs(ctx.handle, 1, C.c_void_p(pm.ctypes.data), None, 4) == vxslam.VX_OK  # no pairs
    dm.close()


def test_profile_shows_the_new_stages(ctx, scene, opts):
    dm = load(ctx, scene.s)
    scene.run(ctx, dm, opts)
    ctx.prof_enable(True)
    scene.run(ctx, dm, opts)
    prof = ctx.prof_read()
    ctx.prof_enable(False)
    for stage in ("track_gate", "track_final", "track_pairs", "track_epairs", "track_epose"):
        assert prof[stage][1] == 1, stage
    assert prof["track_gate"][0] > 0.0 and prof["track_final"][0] > 0.0
    dm.close()


# ---------------------------------------------------------------------------- keyframe creation on the track's list
@pytest.mark.parametrize("with_depth", [False, True])
def test_keyframe_reuses_the_track_match_list(ctx, scene, opts, with_depth):
    """vx_dmap_create_keyframe fed vx_track_frame_matches(0) and the frame's device positions, against
    vx_dmap_create_keyframe_host on the fetched arrays: map, result record and landmark records"""
    s = scene.s
    flags = s["flags"].copy()
    flags[::3] = 0  # features without a landmark: the ones triangulation may fill
    depth = np.ascontiguousarray(synth.make_depth(9)) if with_depth else None
    dm, hm = load(ctx, s, flags), load(ctx, s, flags)
    got = scene.run(ctx, dm, opts)
    pose = got["result"]["pose"]
    assert got["result"]["path"] == vxslam.TRACK_PATH_PNP
    matches = match_list(ctx, 0)
    d = scene.curr.device()
    keep = None if depth is None else dev(depth)
    dd = None if depth is None else (keep.data_ptr(), vxslam.DEPTH_TYPES[depth.dtype], depth.shape[0], depth.shape[1],
                                     depth.strides[0])
    a = dm.create_keyframe(KF + 1, pose, s["intr"], (d["xy"], d["stride"], d["count"], d["cap"]), last_kf_id=KF,
                           matches=ctx.track_frame_matches(0), depth=dd, first_landmark_id=50000)
    kp = got["keypoints"]
    uv = np.stack([kp["x"], kp["y"]], -1).astype(np.float64)
    b = hm.create_keyframe_host(KF + 1, pose, s["intr"], uv, last_kf_id=KF, matches=matches, depth=depth,
                                first_landmark_id=50000)
    print("depth", a["result"]["n_depth"], "triangulated", a["result"]["n_triangulated"])
    assert a["result"].tobytes() == b["result"].tobytes() and a["landmarks"].tobytes() == b["landmarks"].tobytes()
    assert a["result"]["n_triangulated"] + a["result"]["n_depth"] > 0
    assert dm.counts() == hm.counts()
    for x, y in zip(dm.download(), hm.download()):
        assert np.array_equal(x, y)
    for k in (KF, KF + 1):
        for x, y in zip(dm.keyframe_features(k), hm.keyframe_features(k)):
            assert np.array_equal(x, y)
    dm.close()
    hm.close()
