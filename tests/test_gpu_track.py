"""GPU parity of the device-resident TrackWithPnP (vx_track_pnp_async / vx_track_pnp_fetch,
csrc/track.hip) against the numpy restatement of tracking.cpp:342-400 (tests/track_ref.py, pinned by
tests/test_track_cpu.py) followed by PnP RANSAC on the pairs it gathers.

Bars: counts, min_distance and pair_match identical to the restatement; the PnP record and the mask
byte-identical to ctx.pnp_ransac on the restatement's pairs with the resolved options (the same
kernels on the same inputs) and within tests/test_gpu_ransac.py's bars of oracle.pnp_ransac; the
parallax within 1e-12 * max(value, 1) of the sequential numpy sum (any summation order of n <= 4096
non-negative doubles is within (n - 1) * 2^-53 = 4.5e-13 relative, the terms being the same IEEE
sequence on both sides)."""
import numpy as np
import pytest

import vxslam
from vxslam import synth

from track_ref import track_ref

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-9   # tests/test_gpu_ransac.py
KF = 7            # id of the last keyframe in the scenes below


def dev(a):
    """numpy array -> device bytes (a torch tensor, kept by the caller); never empty, so its
    pointer is never NULL"""
    import torch

    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.from_numpy(np.concatenate([b, np.zeros(16, np.uint8)])).cuda()
    torch.cuda.synchronize()
    return t


def load(ctx, s, bad=None, skip=()):
    """a DMap holding the scene's landmarks (those in `skip` never inserted) and its last keyframe"""
    dm = vxslam.DMap(ctx)
    keep = ~np.isin(np.arange(len(s["lm_id"])), list(skip))
    dm.add_landmarks(s["lm_id"][keep], s["lm_pos"][keep], None if bad is None else np.asarray(bad, np.uint8)[keep])
    dm.add_keyframe(KF, s["pose"], s["intr"], True, s["kf_uv"], s["lm_id"], s["flags"])
    return dm


def landmarks(s, bad=None, skip=()):
    return {int(i): (s["lm_pos"][k], 0 if bad is None else int(bad[k]))
            for k, i in enumerate(s["lm_id"]) if k not in skip}


def track(ctx, dm, curr_xy, matches, intr, opts, n_curr=None, kf=KF):
    """the call with an explicit device match list and packed float2 positions"""
    m = np.ascontiguousarray(matches, vxslam.MATCH_DTYPE)
    keep = (dev(np.asarray(curr_xy, np.float32)), dev(np.array([len(curr_xy) if n_curr is None else n_curr], np.int32)),
            dev(m), dev(np.array([len(m)], np.int32)))
    ctx.track_pnp_async(dm, kf, (keep[0].data_ptr(), 8, keep[1].data_ptr()), intr, opts,
                        matches=(keep[2].data_ptr(), keep[3].data_ptr(), len(m)))
    out = ctx.track_pnp_fetch()
    del keep
    return out


def same_as_oracle(rg, mg, rc, mc):
    for k in ("ok", "best_hypothesis", "hypotheses_run", "n_inliers"):
        assert rg[k] == rc[k], (k, rg[k], rc[k])
    assert np.array_equal(mg, mc)
    if rc["ok"]:
        assert np.abs(rg["pose"] - rc["pose"]).max() <= POSE_TOL, (rg["pose"], rc["pose"])
        assert np.abs(rg["rvec"] - rc["rvec"]).max() <= POSE_TOL
        assert abs(rg["cost0"] - rc["cost0"]) <= 1e-9 * max(rc["cost0"], 1.0)
        assert abs(rg["cost"] - rc["cost"]) <= 1e-9 * max(rc["cost"], 1.0)


def check(ctx, oracle, got, ref, intr, opts):
    """every field of a fetched result against the restatement `ref` + RANSAC on its pairs; returns
    the status the reference's return statements give"""
    res, pm, mask = got
    for k in ("n_matches", "n_good_matches", "n_pairs", "n_bad_index"):
        assert res[k] == ref[k], (k, res[k], ref[k])
    assert res["min_distance"] == ref["min_distance"]
    assert np.array_equal(pm, ref["pair_match"])
    assert np.all(np.diff(pm) > 0)
    print("parallax", res["parallax"], ref["parallax"])
    assert abs(res["parallax"] - ref["parallax"]) <= 1e-12 * max(ref["parallax"], 1.0)
    if ref["gate"]:
        assert res["status"] == ref["gate"]
        assert res["pnp"]["ok"] == 0 and res["pnp"]["hypotheses_run"] == 0 and mask.sum() == 0
        return ref["gate"]
    po = np.array(opts["pnp"], vxslam.PNP_OPTIONS_DTYPE)
    po["max_iterations"] = ref["max_iterations"]
    rg, mg = ctx.pnp_ransac(ref["obj"], ref["img"], intr, po)
    assert res["pnp"].tobytes() == rg.tobytes()
    assert np.array_equal(mask, mg)
    rc, mc = oracle.pnp_ransac(ref["obj"], ref["img"], intr, po)
    same_as_oracle(res["pnp"], mask, rc, mc)
    status = vxslam.TRACK_OK if rc["ok"] and rc["n_inliers"] >= opts["min_inliers"] else vxslam.TRACK_PNP_FAILED
    assert res["status"] == status
    return status


@pytest.fixture(scope="module")
def scene128():
    return synth.make_track_scene(12, 128, wrong_frac=0.2)


# ---------------------------------------------------------------------------- parity
def test_parity_300(ctx, oracle):
    s = synth.make_track_scene(3, 300, wrong_frac=0.3)
    opts = vxslam.track_options()
    ref = track_ref(s["matches"], s["kf_uv"], s["lm_id"], s["flags"], s["curr_xy"], landmarks(s))
    # the seed is usable: the reference path alone gives ok with >= 30 inliers
    po = vxslam.pnp_options(ref["n_pairs"])
    rc, _ = oracle.pnp_ransac(ref["obj"], ref["img"], s["intr"], po)
    assert ref["gate"] == 0 and ref["n_pairs"] == 300 and rc["ok"] == 1 and rc["n_inliers"] >= 30
    dm = load(ctx, s)
    got = track(ctx, dm, s["curr_xy"], s["matches"], s["intr"], opts)
    assert check(ctx, oracle, got, ref, s["intr"], opts) == vxslam.TRACK_OK
    assert got[0]["parallax"] > 1.0
    assert np.abs(got[0]["pnp"]["pose"] - s["pose"]).max() < 5e-3
    dm.close()


# ---------------------------------------------------------------------------- skip rules
def test_every_skip_rule(ctx, oracle, scene128):
    """tracking.cpp:376-394 on known features, inside a map that LocalBA has already run on"""
    s = {k: np.array(v) for k, v in scene128.items()}
    NO_LM, OUTLIER, NEVER, REMOVED, BAD, NAN, FAR, EDGE, LATE0, LATE1 = 3, 10, 17, 24, 31, 38, 45, 52, 59, 66
    s["flags"][NO_LM] = 0
    s["flags"][OUTLIER] = 3
    s["lm_pos"][NAN, 1] = np.nan
    s["lm_pos"][FAR] = [0.3, 0.2, -1000.5]
    s["lm_pos"][EDGE, 0] = 1000.0   # not > 1000: kept (a gross outlier for RANSAC)
    bad = np.zeros(128, np.uint8)
    bad[BAD] = 1
    opts = vxslam.track_options()
    # a map with a LocalBA window of its own (other ids), so DMap.optimize really runs
    bm = synth.make_ba_map(77, 5, 400)
    kf = 10 ** 6
    assert bm["kf_id"].max() < kf and not np.isin(s["lm_id"], bm["lm_id"]).any()
    dm = vxslam.DMap(ctx)
    vxslam.dmap_load(dm, bm)
    skip = {NEVER, LATE0, LATE1}
    keep = ~np.isin(np.arange(128), list(skip))
    dm.add_landmarks(s["lm_id"][keep], s["lm_pos"][keep], bad[keep])
    dm.add_keyframe(kf, s["pose"], s["intr"], True, s["kf_uv"], s["lm_id"], s["flags"])
    dm.remove_landmarks(s["lm_id"][[REMOVED]])
    lms = landmarks(s, bad, skip | {REMOVED})
    ref = track_ref(s["matches"], s["kf_uv"], s["lm_id"], s["flags"], s["curr_xy"], lms)
    gone = {NO_LM, OUTLIER, NEVER, REMOVED, BAD, NAN, FAR, LATE0, LATE1}
    assert ref["n_good_matches"] == 128 and set(range(128)) - set(ref["pair_match"].tolist()) == gone
    got = track(ctx, dm, s["curr_xy"], s["matches"], s["intr"], opts, kf=kf)
    check(ctx, oracle, got, ref, s["intr"], opts)
    assert EDGE in got[1] and not (set(got[1].tolist()) & gone)
    # landmarks inserted after a LocalBA run on the map (the id table grows with them)
    st = dm.optimize(vxslam.default_ba_options(window=5), ref_kf_id=bm["ref_kf_id"])
    assert st.status == 0
    dm.add_landmarks(s["lm_id"][[LATE0, LATE1]], s["lm_pos"][[LATE0, LATE1]])
    lms = landmarks(s, bad, {NEVER, REMOVED})
    ref = track_ref(s["matches"], s["kf_uv"], s["lm_id"], s["flags"], s["curr_xy"], lms)
    got = track(ctx, dm, s["curr_xy"], s["matches"], s["intr"], opts, kf=kf)
    check(ctx, oracle, got, ref, s["intr"], opts)
    assert LATE0 in got[1] and LATE1 in got[1] and NEVER not in got[1]
    # a removed id inserted again is found again (Map::InsertLandmark after RemoveLandmark)
    dm.add_landmarks(s["lm_id"][[REMOVED]], s["lm_pos"][[REMOVED]])
    got = track(ctx, dm, s["curr_xy"], s["matches"], s["intr"], opts, kf=kf)
    assert REMOVED in got[1]
    with pytest.raises(vxslam.VxError):
        track(ctx, dm, s["curr_xy"], s["matches"], s["intr"], opts, kf=kf + 1)
    dm.close()


# ---------------------------------------------------------------------------- compaction
@pytest.fixture(scope="module")
def holes(ctx, scene128):
    """the 128-feature scene with every 5th feature without a landmark (holes in the pair compaction)"""
    s = {k: np.array(v) for k, v in scene128.items()}
    s["flags"][::5] = 0
    dm = load(ctx, s)
    yield s, dm, landmarks(s)
    dm.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, "block", "block+1", 2000])
def test_compaction_boundaries(ctx, oracle, holes, n):
    s, dm, lms = holes
    B = vxslam.track_block()
    n = {"block": B, "block+1": B + 1}.get(n, n)
    k = np.arange(n)
    m = np.zeros(n, vxslam.MATCH_DTYPE)
    m["query_idx"] = (k * 37) % 128          # features repeat: every pair stays geometrically right
    m["train_idx"] = s["train_of"][m["query_idx"]]
    m["distance"] = np.where(k % 3 == 1, 90.0, 4.0 + k % 7)   # every third dropped (thr = 30)
    opts = vxslam.track_options(min_matches=1, min_inliers=1)
    ref = track_ref(m, s["kf_uv"], s["lm_id"], s["flags"], s["curr_xy"], lms, 1, 1)
    assert ref["n_good_matches"] == n - np.count_nonzero(k % 3 == 1)
    got = track(ctx, dm, s["curr_xy"], m, s["intr"], opts)
    check(ctx, oracle, got, ref, s["intr"], opts)


@pytest.mark.parametrize("dist,n_good,min_d", [((10, 30, 31), 2, 10.0), ((41, 20, 40), 2, 20.0),
                                               ((150, 101, 200, 201), 3, 100.0)])
def test_distance_filter(ctx, oracle, holes, dist, n_good, min_d):
    s, dm, lms = holes
    m = np.array(s["matches"][1:1 + len(dist)], vxslam.MATCH_DTYPE)   # features 1.. hold landmarks
    m["distance"] = dist
    opts = vxslam.track_options(min_matches=1, min_inliers=1)
    ref = track_ref(m, s["kf_uv"], s["lm_id"], s["flags"], s["curr_xy"], lms, 1, 1)
    got = track(ctx, dm, s["curr_xy"], m, s["intr"], opts)
    check(ctx, oracle, got, ref, s["intr"], opts)
    assert got[0]["n_good_matches"] == n_good and got[0]["min_distance"] == min_d
    assert len(got[1]) == n_good


# ---------------------------------------------------------------------------- early returns
def test_early_returns(ctx, oracle, holes):
    s, dm, lms = holes
    opts = vxslam.track_options()
    args = (s["kf_uv"], s["lm_id"], s["flags"], s["curr_xy"], lms)
    # min_matches - 1 kept matches: FEW_MATCHES, parallax 0; min_matches: past that gate
    got = track(ctx, dm, s["curr_xy"], s["matches"][:49], s["intr"], opts)
    assert check(ctx, oracle, got, track_ref(s["matches"][:49], *args), s["intr"], opts) == vxslam.TRACK_FEW_MATCHES
    assert got[0]["n_good_matches"] == 49 and got[0]["parallax"] == 0.0 and got[0]["n_pairs"] > 0
    got = track(ctx, dm, s["curr_xy"], s["matches"][:50], s["intr"], opts)
    assert check(ctx, oracle, got, track_ref(s["matches"][:50], *args), s["intr"], opts) != vxslam.TRACK_FEW_MATCHES
    assert got[0]["parallax"] > 0.0
    # min_inliers - 1 pairs: FEW_PAIRS, no hypothesis run
    n_pairs = track_ref(s["matches"], *args)["n_pairs"]
    o2 = vxslam.track_options(min_inliers=n_pairs + 1)
    got = track(ctx, dm, s["curr_xy"], s["matches"], s["intr"], o2)
    ref = track_ref(s["matches"], *args, 50, n_pairs + 1)
    assert check(ctx, oracle, got, ref, s["intr"], o2) == vxslam.TRACK_FEW_PAIRS
    assert got[0]["pnp"]["ok"] == 0 and got[0]["pnp"]["hypotheses_run"] == 0 and got[0]["parallax"] > 0.0
    o3 = vxslam.track_options(min_inliers=n_pairs)
    got = track(ctx, dm, s["curr_xy"], s["matches"], s["intr"], o3)
    assert check(ctx, oracle, got, track_ref(s["matches"], *args, 50, n_pairs), s["intr"], o3) != vxslam.TRACK_FEW_PAIRS
    # indices outside the two feature sets: counted, skipped
    m = np.array(s["matches"], vxslam.MATCH_DTYPE)
    m["query_idx"][[4, 70]] = [128, -1]
    m["train_idx"][[9, 71, 100]] = [120, 2 ** 30, -5]   # 120: inside the array, outside the 120 rows it is said to hold
    ref = track_ref(m, s["kf_uv"], s["lm_id"], s["flags"], s["curr_xy"][:120], lms)
    got = track(ctx, dm, s["curr_xy"], m, s["intr"], opts, n_curr=120)
    check(ctx, oracle, got, ref, s["intr"], opts)
    n_bad = np.count_nonzero((m["query_idx"] < 0) | (m["query_idx"] >= 128) | (m["train_idx"] < 0) | (m["train_idx"] >= 120))
    assert got[0]["n_bad_index"] == n_bad >= 5 and not (set(got[1].tolist()) & {4, 70, 9, 71, 100})
    # argument checks
    for bad_intr in ([0.0, 500.0, 320.0, 240.0], [500.0, 0.0, 320.0, 240.0]):
        with pytest.raises(vxslam.VxError):
            track(ctx, dm, s["curr_xy"], s["matches"], bad_intr, opts)
    with pytest.raises(vxslam.VxError):
        track(ctx, dm, s["curr_xy"], s["matches"], s["intr"], vxslam.track_options(max_iterations=4097))


def test_collinear_landmarks_fail_pnp(ctx, oracle, scene128):
    s = {k: np.array(v) for k, v in scene128.items()}
    s["lm_pos"][:, 1] = 0.0
    s["lm_pos"][:, 2] = 3.0
    dm = load(ctx, s)
    opts = vxslam.track_options()
    ref = track_ref(s["matches"], s["kf_uv"], s["lm_id"], s["flags"], s["curr_xy"], landmarks(s))
    got = track(ctx, dm, s["curr_xy"], s["matches"], s["intr"], opts)
    assert check(ctx, oracle, got, ref, s["intr"], opts) == vxslam.TRACK_PNP_FAILED
    assert got[0]["n_pairs"] == 128 and got[0]["pnp"]["ok"] == 0
    dm.close()


# ---------------------------------------------------------------------------- whole chain
def test_frame_to_pose_chain(ctx, oracle):
    """extract -> match -> track with nothing fetched between equals the same call fed the fetched
    keypoints and matches explicitly"""
    import torch

    frames = synth.make_frames(41, 2, 240, 320)
    p = vxslam.default_orb_params(n_features=500)
    d = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    for slot in range(2):
        ctx.orb_extract_async(d[slot].data_ptr(), 320, 240, 3, 320 * 3, slot, p)
    ctx.match_slots_async(0, 1)
    intr = np.array([260.0, 260.0, 160.0, 120.0])
    opts = vxslam.track_options(min_matches=20, min_inliers=10)
    k0, _ = ctx.orb_fetch(0)
    k1, _ = ctx.orb_fetch(1)
    # the keyframe (identity pose) holds a landmark per keypoint: its pixel back-projected to a depth
    z = 2.0 + 0.37 * (np.arange(len(k0)) % 9)
    pos = np.stack([(k0["x"] - intr[2]) / intr[0] * z, (k0["y"] - intr[3]) / intr[1] * z, z], -1).astype(np.float64)
    ids = np.arange(1, len(k0) + 1, dtype=np.uint64)
    dm = vxslam.DMap(ctx)
    dm.add_landmarks(ids, pos)
    dm.add_keyframe(KF, [0, 0, 0, 1, 0, 0, 0], intr, True, np.stack([k0["x"], k0["y"]], -1), ids, np.ones(len(k0), np.uint8))
    ctx.track_pnp_async(dm, KF, 1, intr, opts)          # slot 1, the context's own match list
    a = ctx.track_pnp_fetch()
    m = ctx.match_fetch()
    assert len(m) >= 20 and a[0]["n_matches"] == len(m) and a[0]["n_good_matches"] >= 20 and a[0]["n_pairs"] >= 10
    b = track(ctx, dm, np.stack([k1["x"], k1["y"]], -1), m, intr, opts)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    ref = track_ref(m, np.stack([k0["x"], k0["y"]], -1), ids, np.ones(len(k0), np.uint8),
                    np.stack([k1["x"], k1["y"]], -1), {int(i): (pos[k], 0) for k, i in enumerate(ids)}, 20, 10)
    assert check(ctx, oracle, a, ref, intr, opts) == vxslam.TRACK_OK
    dm.close()


# ---------------------------------------------------------------------------- contexts and state
def test_contexts_and_state(ctx):
    s = synth.make_track_scene(3, 300, wrong_frac=0.3)
    dm = load(ctx, s)
    opts = vxslam.track_options()
    a = track(ctx, dm, s["curr_xy"], s["matches"], s["intr"], opts)
    assert a[0]["status"] == vxslam.TRACK_OK
    # too small a caller buffer is an error that leaves the result fetchable
    with pytest.raises(vxslam.VxError):
        ctx.track_pnp_fetch(cap=a[0]["n_pairs"] - 1)
    again = ctx.track_pnp_fetch(cap=a[0]["n_pairs"])
    assert a[0].tobytes() == again[0].tobytes() and np.array_equal(a[1], again[1]) and np.array_equal(a[2], again[2])
    # byte-identical when repeated
    b = track(ctx, dm, s["curr_xy"], s["matches"], s["intr"], opts)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    # a vx_pnp_ransac between the async call and its fetch does not touch the result
    m = np.ascontiguousarray(s["matches"], vxslam.MATCH_DTYPE)
    keep = (dev(s["curr_xy"]), dev(np.array([300], np.int32)), dev(m), dev(np.array([300], np.int32)))
    ctx.track_pnp_async(dm, KF, (keep[0].data_ptr(), 8, keep[1].data_ptr()), s["intr"], opts,
                        matches=(keep[2].data_ptr(), keep[3].data_ptr(), 300))
    other = synth.make_pnp_problem(9, 500, outlier_frac=0.4)
    ctx.pnp_ransac(other["obj"], other["img"], other["intr"], vxslam.pnp_options(500))
    c = ctx.track_pnp_fetch()
    assert a[0].tobytes() == c[0].tobytes() and np.array_equal(a[1], c[1]) and np.array_equal(a[2], c[2])
    # another context of the device, ordered after the map's context by the call itself
    ctx2 = vxslam.Context(0)
    with pytest.raises(vxslam.VxError):   # nothing matched on ctx2, and no list given
        ctx2.track_pnp_async(dm, KF, (keep[0].data_ptr(), 8, keep[1].data_ptr()), s["intr"], opts)
    e = track(ctx2, dm, s["curr_xy"], s["matches"], s["intr"], opts)
    assert a[0].tobytes() == e[0].tobytes() and np.array_equal(a[1], e[1]) and np.array_equal(a[2], e[2])
    ctx2.close()
    dm.close()


# ---------------------------------------------------------------------------- steady state
def test_null_matches_after_graph_replay(ctx, oracle):
    """per-frame steady state: vx_match_device_async replays its captured graph from the third call on
    (no host-side enqueue runs then), with a smaller match on the same context in between; the
    context's match list handed over with matches=None must still be the whole list"""
    s = synth.make_track_scene(3, 300, wrong_frac=0.3)
    dm = load(ctx, s)
    opts = vxslam.track_options()
    ref = track_ref(s["matches"], s["kf_uv"], s["lm_id"], s["flags"], s["curr_xy"], landmarks(s))
    keep = (dev(s["desc_kf"]), dev(s["desc_curr"]), dev(np.array([300], np.int32)), dev(s["curr_xy"]),
            dev(np.array([90], np.int32)))
    big = ((keep[0].data_ptr(), keep[2].data_ptr(), 300), (keep[1].data_ptr(), keep[2].data_ptr(), 300))
    small = ((keep[0].data_ptr(), keep[4].data_ptr(), 90), (keep[1].data_ptr(), keep[2].data_ptr(), 300))
    launched0 = ctx.graph_counts()[1]
    for it in range(6):
        if it % 2:
            assert len(ctx.match(s["desc_kf"][:100], s["desc_curr"])) <= 100   # capacity 100, synchronous
        else:
            ctx.match_device_async(*small)                                     # capacity 90, its own graph key
        ctx.match_device_async(*big)
        ctx.track_pnp_async(dm, KF, (keep[3].data_ptr(), 8, keep[2].data_ptr()), s["intr"], opts)
        got = ctx.track_pnp_fetch()
        assert got[0]["n_matches"] == 300, it
        assert check(ctx, oracle, got, ref, s["intr"], opts) == vxslam.TRACK_OK
    assert ctx.graph_counts()[1] - launched0 >= 4   # the later matches really were replays
    dm.close()


def test_host_input_steady_state(ctx, oracle, scene128):
    """vx_track_pnp_host_async (what visionx::PnPTracker calls every frame) over keyframes of
    different sizes: 300 features three times (eager, captured, replayed), a 128-feature keyframe
    (a smaller capacity bucket), then the large one again"""
    a = synth.make_track_scene(3, 300, wrong_frac=0.3)
    b = {k: np.array(v) for k, v in scene128.items()}
    b["lm_id"] = b["lm_id"] + np.uint64(10 ** 5)
    assert not np.isin(b["lm_id"], a["lm_id"]).any()
    dm = load(ctx, a)
    dm.add_landmarks(b["lm_id"], b["lm_pos"])
    dm.add_keyframe(KF + 1, b["pose"], b["intr"], True, b["kf_uv"], b["lm_id"], b["flags"])
    opts = vxslam.track_options()
    refs = {id(s): track_ref(s["matches"], s["kf_uv"], s["lm_id"], s["flags"], s["curr_xy"], landmarks(s))
            for s in (a, b)}
    for it, (s, kf) in enumerate([(a, KF), (a, KF), (a, KF), (b, KF + 1), (a, KF), (a, KF)]):
        ctx.track_pnp_host_async(dm, kf, s["desc_kf"], s["desc_curr"], s["curr_xy"], s["intr"], opts)
        got = ctx.track_pnp_fetch()
        assert got[0]["n_matches"] == len(s["matches"]), it
        check(ctx, oracle, got, refs[id(s)], s["intr"], opts)
        assert np.array_equal(ctx.match_fetch(), s["matches"].astype(vxslam.MATCH_DTYPE))
    dm.close()


def test_pair_kernel_is_a_profiled_stage(ctx, scene128):
    s = scene128
    dm = load(ctx, s)
    ctx.prof_enable(True, ["track_pairs", "pnp_hypotheses", "pnp_refine"])
    try:
        ctx.prof_read()
        track(ctx, dm, s["curr_xy"], s["matches"], s["intr"], vxslam.track_options())
        p = ctx.prof_read()
    finally:
        ctx.prof_enable(False)
    assert p["track_pairs"][1] == 1 and p["track_pairs"][0] > 0.0
    assert p["pnp_hypotheses"][1] == 1 and p["pnp_refine"][1] == 1
    dm.close()
