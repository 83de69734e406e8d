"""GPU parity of the device-resident TrackLastFrame (vx_track_essential_async /
vx_track_essential_fetch, csrc/track_ess.hip) against the numpy restatement of tracking.cpp:291-325,
:509-514, :539-541 (tests/track_ess_ref.py, pinned by tests/test_track_ess_cpu.py) with essential-matrix
RANSAC + recoverPose on the pairs it gathers.

Bars: counts, min_distance and pair_match identical to the restatement; the essential record and the
mask byte-identical to ctx.essential_ransac on the restatement's pairs (the same kernels on the same
inputs) and to oracle.essential_ransac (tests/test_gpu_essential.py's bar); the composed pose and the
parallax within 1e-12 * max(|value|, 1) of the restatement (tests/test_gpu_track.py's parallax bar: any
summation order of n <= 4096 non-negative doubles is within (n - 1) * 2^-53 = 4.5e-13 relative; the
pose is the same IEEE sequence on both sides, so equality is expected and printed)."""
import numpy as np
import pytest

import vxslam
from vxslam import synth

from track_ess_ref import compose, pose_from_Rt, track_ess_ref

pytestmark = pytest.mark.gpu

IDENT = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])


def dev(a):
    """numpy array -> device bytes (a torch tensor, kept by the caller); never empty, so its
    pointer is never NULL"""
    import torch

    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.from_numpy(np.concatenate([b, np.zeros(16, np.uint8)])).cuda()
    torch.cuda.synchronize()
    return t


def enqueue(ctx, last_xy, curr_xy, matches, intr, opts, pose_last=None, n_last=None, n_curr=None):
    """the call with an explicit device match list and packed float2 positions; returns what must stay
    alive until the fetch"""
    m = np.ascontiguousarray(matches, vxslam.MATCH_DTYPE)
    keep = (dev(np.asarray(last_xy, np.float32)), dev(np.array([len(last_xy) if n_last is None else n_last], np.int32)),
            dev(np.asarray(curr_xy, np.float32)), dev(np.array([len(curr_xy) if n_curr is None else n_curr], np.int32)),
            dev(m), dev(np.array([len(m)], np.int32)))
    ctx.track_essential_async((keep[0].data_ptr(), 8, keep[1].data_ptr()), (keep[2].data_ptr(), 8, keep[3].data_ptr()),
                              intr, opts, matches=(keep[4].data_ptr(), keep[5].data_ptr(), len(m)), pose_last=pose_last)
    return keep


def track(ctx, *args, **kw):
    keep = enqueue(ctx, *args, **kw)
    out = ctx.track_essential_fetch()
    del keep
    return out


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def check(ctx, oracle, got, ref, intr, opts, pose_last=None):
    """every field of a fetched result against the restatement `ref` + essential RANSAC on its pairs;
    returns the status the reference's return statements give"""
    res, pm, mask = got
    for k in ("n_matches", "n_good_matches", "n_pairs", "n_bad_index"):
        assert res[k] == ref[k], (k, res[k], ref[k])
    assert res["min_distance"] == ref["min_distance"]
    assert np.array_equal(pm, ref["pair_match"])
    assert np.all(np.diff(pm) > 0)
    print("parallax", res["parallax"], ref["parallax"], "equal" if res["parallax"] == ref["parallax"] else "differs")
    assert abs(res["parallax"] - ref["parallax"]) <= 1e-12 * max(ref["parallax"], 1.0)
    if ref["gate"]:
        assert res["status"] == vxslam.TRACK_FEW_MATCHES
        assert res["ess"]["ok"] == 0 and res["ess"]["hypotheses_run"] == 0 and mask.sum() == 0
        assert not res["pose"].any() and res["parallax"] == 0.0
        return vxslam.TRACK_FEW_MATCHES
    eo = np.array(opts["ess"], vxslam.EM_OPTIONS_DTYPE)
    eg, mg = ctx.essential_ransac(ref["pts_last"], ref["pts_curr"], intr, eo)
    assert res["ess"].tobytes() == eg.tobytes()
    assert np.array_equal(mask, mg)
    ec, mc = oracle.essential_ransac(ref["pts_last"], ref["pts_curr"], intr, eo)
    assert res["ess"].tobytes() == ec.tobytes()
    assert np.array_equal(mask, mc)
    if ec["ok"]:
        want = compose(pose_from_Rt(ec["R"], ec["t"]), IDENT if pose_last is None else pose_last)
        print("pose", res["pose"], "equal" if np.array_equal(res["pose"], want) else ("differs", res["pose"] - want))
        assert (np.abs(res["pose"] - want) <= 1e-12 * np.maximum(np.abs(want), 1.0)).all()
    else:
        assert not res["pose"].any()
    status = vxslam.TRACK_OK if ec["ok"] and ec["n_inliers"] >= opts["min_inliers"] else vxslam.TRACK_ESSENTIAL_FAILED
    assert res["status"] == status
    return status


@pytest.fixture(scope="module")
def scene300():
    return synth.make_last_frame_scene(3, 300, wrong_frac=0.3)


@pytest.fixture(scope="module")
def opts200():
    return vxslam.track_essential_options(max_iterations=200)


# ---------------------------------------------------------------------------- parity
def test_parity_300(ctx, oracle, scene300, opts200):
    s = scene300
    ref = track_ess_ref(s["matches"], s["last_xy"], s["curr_xy"])
    assert ref["gate"] == 0 and ref["n_pairs"] == 300
    got = track(ctx, s["last_xy"], s["curr_xy"], s["matches"], s["intr"], opts200, pose_last=s["pose_last"])
    assert check(ctx, oracle, got, ref, s["intr"], opts200, s["pose_last"]) == vxslam.TRACK_OK
    res = got[0]
    assert res["parallax"] > 1.0 and res["ess"]["n_inliers"] >= 30
    q = res["pose"][:4]
    assert abs(np.linalg.norm(q) - 1.0) < 1e-15
    # the bar tests/test_gpu_essential.py holds R to, on the composed rotation
    assert np.abs(synth.quat_to_mat(q) - s["R_cw"]).max() < 0.02
    assert np.abs(res["ess"]["R"].reshape(3, 3) - s["R"]).max() < 0.02


def test_default_options(ctx, oracle, scene300):
    s = scene300
    opts = vxslam.track_essential_options()
    assert opts["ess"]["max_iterations"] == 1000
    ref = track_ess_ref(s["matches"], s["last_xy"], s["curr_xy"])
    got = track(ctx, s["last_xy"], s["curr_xy"], s["matches"], s["intr"], opts, pose_last=s["pose_last"])
    assert check(ctx, oracle, got, ref, s["intr"], opts, s["pose_last"]) == vxslam.TRACK_OK


# ---------------------------------------------------------------------------- compaction
@pytest.mark.parametrize("kept", ["B-1", "B", "B+1", "2B+1"])
def test_compaction_boundaries(ctx, oracle, scene300, kept):
    """holes of both kinds — matches the filter drops and kept matches with an index out of range —
    on both sides of every chunk edge of both ordered compactions"""
    s = scene300
    B = vxslam.track_block()
    K = {"B-1": B - 1, "B": B, "B+1": B + 1, "2B+1": 2 * B + 1}[kept]
    edge = {B - 1, B, 2 * B - 1, 2 * B}
    drop, i = [], 0
    while len(drop) - sum(drop) < K:                   # match index i is dropped by the filter
        drop.append(i % 3 == 1 or i in edge)
        i += 1
    drop = np.array(drop)
    n = len(drop)
    k = np.arange(n)
    m = np.zeros(n, vxslam.MATCH_DTYPE)
    m["query_idx"] = (k * 37) % 300                    # features repeat: every pair stays geometrically right
    m["train_idx"] = s["train_of"][m["query_idx"]]
    m["distance"] = np.where(drop, 90.0, 4.0 + k % 7)  # thr = 30
    kept_at = np.nonzero(~drop)[0]                     # kept position j -> match index
    bad = [j for j in sorted(edge | {0, K - 1, B - 2, B + 1}) if 0 <= j < K]
    m["query_idx"][kept_at[bad[::2]]] = 300            # == the device count
    m["train_idx"][kept_at[bad[1::2]]] = 2 ** 30
    opts = vxslam.track_essential_options(min_matches=1, min_inliers=1, max_iterations=100)
    ref = track_ess_ref(m, s["last_xy"], s["curr_xy"], 1)
    assert ref["n_good_matches"] == K and ref["n_bad_index"] == len(bad) and ref["n_pairs"] == K - len(bad)
    got = track(ctx, s["last_xy"], s["curr_xy"], m, s["intr"], opts, pose_last=s["pose_last"])
    check(ctx, oracle, got, ref, s["intr"], opts, s["pose_last"])


@pytest.mark.parametrize("dist,n_good,min_d", [((10, 30, 31), 2, 10.0), ((41, 20, 40), 2, 20.0),
                                               ((150, 101, 200, 201), 3, 100.0)])
def test_distance_filter(ctx, oracle, scene300, dist, n_good, min_d):
    s = scene300
    m = np.array(s["matches"][1:1 + len(dist)], vxslam.MATCH_DTYPE)
    m["distance"] = dist
    opts = vxslam.track_essential_options(min_matches=1, min_inliers=1, max_iterations=50)
    ref = track_ess_ref(m, s["last_xy"], s["curr_xy"], 1)
    got = track(ctx, s["last_xy"], s["curr_xy"], m, s["intr"], opts)
    assert check(ctx, oracle, got, ref, s["intr"], opts) == vxslam.TRACK_ESSENTIAL_FAILED   # fewer than 5 pairs
    assert got[0]["n_good_matches"] == n_good and got[0]["min_distance"] == min_d
    assert len(got[1]) == n_good


# ---------------------------------------------------------------------------- indices, early returns
def test_bad_indices_are_counted_and_never_read(ctx, oracle, scene300, opts200):
    s = scene300
    m = np.array(s["matches"], vxslam.MATCH_DTYPE)
    # 280 / 290: inside the arrays, outside the rows they are said to hold
    m["query_idx"][[4, 70, 150]] = [280, -1, 2 ** 30]
    m["train_idx"][[9, 71, 100, 200]] = [290, 2 ** 30, -5, 291]
    ref = track_ess_ref(m, s["last_xy"][:280], s["curr_xy"][:290])
    got = track(ctx, s["last_xy"], s["curr_xy"], m, s["intr"], opts200, n_last=280, n_curr=290)
    check(ctx, oracle, got, ref, s["intr"], opts200)
    n_bad = np.count_nonzero((m["query_idx"] < 0) | (m["query_idx"] >= 280) | (m["train_idx"] < 0) | (m["train_idx"] >= 290))
    assert got[0]["n_bad_index"] == n_bad >= 7 and not (set(got[1].tolist()) & {4, 70, 150, 9, 71, 100, 200})
    assert got[0]["n_pairs"] == 300 - n_bad


def test_early_returns(ctx, oracle, scene300, opts200):
    s = scene300
    xy = (s["last_xy"], s["curr_xy"])
    # min_matches - 1 kept matches: FEW_MATCHES, no hypothesis, pose zero, parallax 0; min_matches: past the gate
    got = track(ctx, *xy, s["matches"][:49], s["intr"], opts200, pose_last=s["pose_last"])
    assert check(ctx, oracle, got, track_ess_ref(s["matches"][:49], *xy), s["intr"], opts200, s["pose_last"]) == \
        vxslam.TRACK_FEW_MATCHES
    assert got[0]["n_good_matches"] == 49 and got[0]["n_pairs"] == 49 and got[0]["ess"]["ok"] == 0
    got = track(ctx, *xy, s["matches"][:50], s["intr"], opts200, pose_last=s["pose_last"])
    assert check(ctx, oracle, got, track_ess_ref(s["matches"][:50], *xy), s["intr"], opts200, s["pose_last"]) != \
        vxslam.TRACK_FEW_MATCHES
    assert got[0]["parallax"] > 0.0 and got[0]["ess"]["hypotheses_run"] > 0
    # min_inliers: one more than recoverPose returns fails, exactly as many passes
    n_in = got[0]["ess"]["n_inliers"]
    for mi, st in ((n_in + 1, vxslam.TRACK_ESSENTIAL_FAILED), (n_in, vxslam.TRACK_OK)):
        o = vxslam.track_essential_options(min_inliers=mi, max_iterations=200)
        g = track(ctx, *xy, s["matches"][:50], s["intr"], o, pose_last=s["pose_last"])
        assert check(ctx, oracle, g, track_ess_ref(s["matches"][:50], *xy), s["intr"], o, s["pose_last"]) == st
        assert g[0]["pose"].any()   # composed whenever recoverPose gave a pose (the gate is the caller's)
    # exactly 4 and 5 surviving pairs with both gates at 0; an empty list
    right = np.nonzero(~s["wrong"])[0]
    o0 = vxslam.track_essential_options(min_matches=0, min_inliers=0, max_iterations=100)
    for n in (4, 5):
        m = s["matches"][right[:n]]
        g = track(ctx, *xy, m, s["intr"], o0)
        st = check(ctx, oracle, g, track_ess_ref(m, *xy, 0), s["intr"], o0)
        assert g[0]["n_pairs"] == n
        if n == 4:
            assert st == vxslam.TRACK_ESSENTIAL_FAILED and g[0]["ess"]["ok"] == 0 and g[0]["ess"]["hypotheses_run"] == 0
    g = track(ctx, *xy, s["matches"][:0], s["intr"], o0)
    assert check(ctx, oracle, g, track_ess_ref(s["matches"][:0], *xy, 0), s["intr"], o0) == vxslam.TRACK_ESSENTIAL_FAILED
    assert g[0]["n_matches"] == 0 and g[0]["min_distance"] == 100.0
    # argument checks
    for bad_intr in ([0.0, 500.0, 320.0, 240.0], [500.0, 0.0, 320.0, 240.0]):
        with pytest.raises(vxslam.VxError):
            track(ctx, *xy, s["matches"], bad_intr, opts200)
    with pytest.raises(vxslam.VxError):
        track(ctx, *xy, s["matches"], s["intr"], vxslam.track_essential_options(max_iterations=4097))


def test_all_outlier_matches_fail(ctx, oracle, opts200):
    s = synth.make_last_frame_scene(8, 300, wrong_frac=1.0)
    ref = track_ess_ref(s["matches"], s["last_xy"], s["curr_xy"])
    got = track(ctx, s["last_xy"], s["curr_xy"], s["matches"], s["intr"], opts200)
    assert check(ctx, oracle, got, ref, s["intr"], opts200) == vxslam.TRACK_ESSENTIAL_FAILED
    assert got[0]["n_pairs"] == 300 and got[0]["ess"]["n_inliers"] < 30


# ---------------------------------------------------------------------------- pose_last
def test_pose_last(ctx, scene300, opts200):
    s = scene300
    args = (s["last_xy"], s["curr_xy"], s["matches"], s["intr"], opts200)
    a = track(ctx, *args)                       # NULL
    b = track(ctx, *args, pose_last=IDENT)
    assert a[0]["status"] == vxslam.TRACK_OK and same(a, b)
    # T_cl itself: the identity on the right changes nothing beyond the renormalisation
    T_cl = pose_from_Rt(a[0]["ess"]["R"], a[0]["ess"]["t"])
    assert np.abs(a[0]["pose"] - T_cl).max() < 1e-15
    c = track(ctx, *args, pose_last=s["pose_last"])
    neg = np.concatenate([-s["pose_last"][:4], s["pose_last"][4:]])
    d = track(ctx, *args, pose_last=neg)
    assert np.array_equal(d[0]["pose"][:4], -c[0]["pose"][:4]) and np.array_equal(d[0]["pose"][4:], c[0]["pose"][4:])
    assert np.array_equal(synth.quat_to_mat(d[0]["pose"][:4]), synth.quat_to_mat(c[0]["pose"][:4]))
    assert c[0]["ess"].tobytes() == a[0]["ess"].tobytes() and not np.array_equal(c[0]["pose"], a[0]["pose"])


# ---------------------------------------------------------------------------- forms
def test_device_form_equals_host_form(ctx, oracle, scene300, opts200):
    s = scene300
    a = track(ctx, s["last_xy"], s["curr_xy"], s["matches"], s["intr"], opts200, pose_last=s["pose_last"])
    ctx.track_essential_host_async(s["desc_last"], s["last_xy"], s["desc_curr"], s["curr_xy"], s["intr"], opts200,
                                   pose_last=s["pose_last"])
    b = ctx.track_essential_fetch()
    assert np.array_equal(ctx.match_fetch(), s["matches"].astype(vxslam.MATCH_DTYPE))
    assert a[0]["status"] == vxslam.TRACK_OK and same(a, b)


def test_host_input_steady_state(ctx, oracle, scene300, opts200):
    """vx_track_essential_host_async over frames of different sizes: 300 features three times (eager,
    captured, replayed match graph), a 128-feature pair (a smaller capacity bucket), the large one again"""
    a = scene300
    b = synth.make_last_frame_scene(12, 128, wrong_frac=0.2)
    refs = {id(s): track_ess_ref(s["matches"], s["last_xy"], s["curr_xy"]) for s in (a, b)}
    for it, s in enumerate([a, a, a, b, a, a]):
        ctx.track_essential_host_async(s["desc_last"], s["last_xy"], s["desc_curr"], s["curr_xy"], s["intr"], opts200,
                                       pose_last=s["pose_last"])
        got = ctx.track_essential_fetch()
        assert got[0]["n_matches"] == len(s["matches"]), it
        check(ctx, oracle, got, refs[id(s)], s["intr"], opts200, s["pose_last"])
        assert np.array_equal(ctx.match_fetch(), s["matches"].astype(vxslam.MATCH_DTYPE))


def test_frame_to_pose_chain(ctx, oracle):
    """extract -> match -> track-essential with nothing fetched between (slots, the context's own
    match list) equals the same call fed the fetched keypoints and matches explicitly"""
    import torch

    frames = synth.make_frames(41, 2, 240, 320)
    p = vxslam.default_orb_params(n_features=500)
    d = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    for slot in range(2):
        ctx.orb_extract_async(d[slot].data_ptr(), 320, 240, 3, 320 * 3, slot, p)
    ctx.match_slots_async(0, 1)
    intr = np.array([260.0, 260.0, 160.0, 120.0])
    opts = vxslam.track_essential_options(min_matches=20, min_inliers=10, max_iterations=200)
    pose_last = synth.make_last_frame_scene(1, 8)["pose_last"]
    ctx.track_essential_async(0, 1, intr, opts, pose_last=pose_last)   # slots 0 and 1, the context's own match list
    a = ctx.track_essential_fetch()
    k0, _ = ctx.orb_fetch(0)
    k1, _ = ctx.orb_fetch(1)
    m = ctx.match_fetch()
    assert len(m) >= 20 and a[0]["n_matches"] == len(m) and a[0]["n_good_matches"] >= 20 and a[0]["n_bad_index"] == 0
    xy0, xy1 = np.stack([k0["x"], k0["y"]], -1), np.stack([k1["x"], k1["y"]], -1)
    b = track(ctx, xy0, xy1, m, intr, opts, pose_last=pose_last)
    assert same(a, b)
    check(ctx, oracle, a, track_ess_ref(m, xy0, xy1, 20), intr, opts, pose_last)


# ---------------------------------------------------------------------------- contexts and state
def test_contexts_and_state(ctx, scene300, opts200):
    s = scene300
    args = (s["last_xy"], s["curr_xy"], s["matches"], s["intr"], opts200)
    a = track(ctx, *args, pose_last=s["pose_last"])
    assert a[0]["status"] == vxslam.TRACK_OK
    # too small a caller buffer is an error that leaves the result fetchable
    with pytest.raises(vxslam.VxError):
        ctx.track_essential_fetch(cap=a[0]["n_pairs"] - 1)
    assert same(a, ctx.track_essential_fetch(cap=a[0]["n_pairs"]))
    # byte-identical when repeated
    assert same(a, track(ctx, *args, pose_last=s["pose_last"]))
    # a vx_essential_ransac and a vx_pnp_ransac between the async call and its fetch do not touch the result
    keep = enqueue(ctx, *args, pose_last=s["pose_last"])
    tv = synth.make_two_view(9, 400, outlier_frac=0.4)
    ctx.essential_ransac(tv["pts_last"], tv["pts_curr"], tv["intr"], vxslam.essential_options(max_iterations=100))
    other = synth.make_pnp_problem(9, 500, outlier_frac=0.4)
    ctx.pnp_ransac(other["obj"], other["img"], other["intr"], vxslam.pnp_options(500))
    assert same(a, ctx.track_essential_fetch())
    # another context of the device: nothing matched there, and the same bytes from an explicit list
    ctx2 = vxslam.Context(0)
    with pytest.raises(vxslam.VxError):
        ctx2.track_essential_fetch()
    with pytest.raises(vxslam.VxError):
        ctx2.track_essential_async((keep[0].data_ptr(), 8, keep[1].data_ptr()), (keep[2].data_ptr(), 8, keep[3].data_ptr()),
                                   s["intr"], opts200)
    assert same(a, track(ctx2, *args, pose_last=s["pose_last"]))
    ctx2.close()
    del keep


def test_interleaved_with_a_pnp_track(ctx, scene300, opts200):
    """a track_pnp_async and a track_essential_async both enqueued, then both fetched: each equals its
    solo result"""
    s = scene300
    ts = synth.make_track_scene(3, 300, wrong_frac=0.3)
    dm = vxslam.DMap(ctx)
    dm.add_landmarks(ts["lm_id"], ts["lm_pos"])
    dm.add_keyframe(7, ts["pose"], ts["intr"], True, ts["kf_uv"], ts["lm_id"], ts["flags"])
    topts = vxslam.track_options()
    tm = np.ascontiguousarray(ts["matches"], vxslam.MATCH_DTYPE)
    tk = (dev(ts["curr_xy"]), dev(np.array([300], np.int32)), dev(tm), dev(np.array([300], np.int32)))

    def pnp_async():
        ctx.track_pnp_async(dm, 7, (tk[0].data_ptr(), 8, tk[1].data_ptr()), ts["intr"], topts,
                            matches=(tk[2].data_ptr(), tk[3].data_ptr(), 300))

    args = (s["last_xy"], s["curr_xy"], s["matches"], s["intr"], opts200)
    pnp_async()
    solo_p = ctx.track_pnp_fetch()
    solo_e = track(ctx, *args, pose_last=s["pose_last"])
    assert solo_p[0]["status"] == vxslam.TRACK_OK and solo_e[0]["status"] == vxslam.TRACK_OK
    for order in (0, 1):
        if order == 0:
            pnp_async()
            keep = enqueue(ctx, *args, pose_last=s["pose_last"])
        else:
            keep = enqueue(ctx, *args, pose_last=s["pose_last"])
            pnp_async()
        if order == 0:   # fetched in the other order too
            e, p = ctx.track_essential_fetch(), ctx.track_pnp_fetch()
        else:
            p, e = ctx.track_pnp_fetch(), ctx.track_essential_fetch()
        assert same(solo_p, p) and same(solo_e, e), order
        del keep
    dm.close()


# ---------------------------------------------------------------------------- steady state
def test_null_matches_after_graph_replay(ctx, oracle, scene300, opts200):
    """per-frame steady state: vx_match_device_async replays its captured graph from the third call on,
    with a smaller match on the same context in between; the context's match list handed over with
    matches=None must still be the whole list"""
    s = scene300
    ref = track_ess_ref(s["matches"], s["last_xy"], s["curr_xy"])
    keep = (dev(s["desc_last"]), dev(s["desc_curr"]), dev(np.array([300], np.int32)), dev(s["last_xy"]),
            dev(s["curr_xy"]), dev(np.array([90], np.int32)))
    big = ((keep[0].data_ptr(), keep[2].data_ptr(), 300), (keep[1].data_ptr(), keep[2].data_ptr(), 300))
    small = ((keep[0].data_ptr(), keep[5].data_ptr(), 90), (keep[1].data_ptr(), keep[2].data_ptr(), 300))
    launched0 = ctx.graph_counts()[1]
    first = None
    for it in range(6):
        if it % 2:
            assert len(ctx.match(s["desc_last"][:100], s["desc_curr"])) <= 100   # capacity 100, synchronous
        else:
            ctx.match_device_async(*small)                                       # capacity 90, its own graph key
        ctx.match_device_async(*big)
        ctx.track_essential_async((keep[3].data_ptr(), 8, keep[2].data_ptr()), (keep[4].data_ptr(), 8, keep[2].data_ptr()),
                                  s["intr"], opts200, pose_last=s["pose_last"])
        got = ctx.track_essential_fetch()
        assert got[0]["n_matches"] == 300, it
        if it in (0, 5):
            assert check(ctx, oracle, got, ref, s["intr"], opts200, s["pose_last"]) == vxslam.TRACK_OK
        first = first or got
        assert same(first, got), it
    assert ctx.graph_counts()[1] - launched0 >= 4   # the later matches really were replays
    del keep


def test_stages_are_profiled(ctx, scene300, opts200):
    s = scene300
    ctx.prof_enable(True, ["track_epairs", "track_epose", "em_hypotheses", "em_select"])
    try:
        ctx.prof_read()
        track(ctx, s["last_xy"], s["curr_xy"], s["matches"], s["intr"], opts200)
        p = ctx.prof_read()
    finally:
        ctx.prof_enable(False)
    assert p["track_epairs"][1] == 1 and p["track_epairs"][0] > 0.0
    assert p["track_epose"][1] == 1 and p["track_epose"][0] > 0.0
    assert p["em_hypotheses"][1] >= 1 and p["em_select"][1] >= 3
