"""Tracking::CreateKeyFrame on the device-resident map (vx_dmap_create_keyframe /
vx_dmap_create_keyframe_host, csrc/keyframe.hip) against the numpy restatement of
tracking.cpp:577-584 (tests/keyframe_ref.py, pinned against the chained oracle calls by
tests/test_keyframe_cpu.py, which also asserts every scene's decision margins) and against the four
edit calls the one call replaces.

Bars: the records exact (ids, rows, kind, both feature indices); depth points bit for bit (the
same IEEE operations in the same order); triangulated points within 1e-9 relative (the SVD's
rotation sequence rounds differently), the bar of tests/test_gpu_landmarks.py."""
import numpy as np
import pytest

import vxslam
from vxslam import synth

import cull_ref
import keyframe_ref as R

pytestmark = pytest.mark.gpu

NEW, LAST, FIRST = 8, R.LAST_KF_ID, 5000
SIZES = R.scene_sizes(vxslam.keyframe_block())


def dev(a):
    """numpy array -> device bytes (a torch tensor, kept by the caller); never empty, so its
    pointer is never NULL"""
    import torch

    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.from_numpy(np.concatenate([b, np.zeros(16, np.uint8)])).cuda()
    torch.cuda.synchronize()
    return t


def loaded(ctx, m):
    dm = vxslam.DMap(ctx)
    cull_ref.load(dm, m)
    return dm


def create(dm, form, kf_id, pose, intr, uv, last, matches, depth, first, ctx=None, keypoint_rows=False, opts=None):
    """the one call in either form; the device form with packed float2 rows (or KEYPOINT_DTYPE rows)
    and an explicit device match list"""
    if form == "host":
        return dm.create_keyframe_host(kf_id, pose, intr, uv, last_kf_id=last, matches=matches, depth=depth,
                                       first_landmark_id=first, opts=opts, ctx=ctx)
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    if keypoint_rows:
        rows = np.zeros(len(uv), vxslam.KEYPOINT_DTYPE)
        rows["x"], rows["y"] = uv[:, 0], uv[:, 1]
    else:
        rows = uv.astype(np.float32)
    assert np.array_equal(np.stack([rows["x"], rows["y"]], -1) if keypoint_rows else rows, uv)
    mt = np.zeros(0, vxslam.MATCH_DTYPE) if matches is None else np.ascontiguousarray(matches, vxslam.MATCH_DTYPE)
    keep = [dev(rows), dev(np.array([len(uv)], np.int32)), dev(mt), dev(np.array([len(mt)], np.int32))]
    dd = None
    if depth is not None:
        base = depth if depth.base is None or depth.flags["C_CONTIGUOUS"] else depth.base
        keep.append(dev(base))
        dd = (keep[-1].data_ptr(), vxslam.DEPTH_TYPES[depth.dtype], depth.shape[0], depth.shape[1], depth.strides[0])
    out = dm.create_keyframe(kf_id, pose, intr, (keep[0].data_ptr(), rows.dtype.itemsize if keypoint_rows else 8,
                                                 keep[1].data_ptr(), len(uv)),
                             last_kf_id=last, matches=None if last is None else (keep[2].data_ptr(), keep[3].data_ptr(), len(mt)),
                             depth=dd, first_landmark_id=first, opts=opts, ctx=ctx)
    del keep
    return out


def same_records(got, want, label=""):
    g, w = got["landmarks"], want["landmarks"]
    r = got["result"]
    assert (r["error_bits"], r["n_depth"], r["n_triangulated"]) == (0, want["n_depth"], want["n_triangulated"])
    assert r["next_landmark_id"] == r["first_landmark_id"] + len(w)
    for k in ("lm_id", "row", "kind", "feat_curr", "feat_last"):
        assert np.array_equal(g[k], w[k]), k
    dep, tri = w["kind"] == 0, w["kind"] == 1
    assert np.array_equal(g["pw"][dep], w["pw"][dep])
    if tri.any():
        rel = np.abs(g["pw"][tri] - w["pw"][tri]).max() / np.abs(w["pw"][tri]).max()
        print(label, "triangulated points: largest relative difference", float(rel))
        assert rel <= 1e-9


def same_state(dm, m, got):
    """the resident map against the restatement's edited dict; the dict then takes the call's own
    positions (checked against the restatement's by same_records), as a later call's map holds them"""
    lm = np.repeat(np.arange(len(m["lm_id"])), np.diff(m["lm_obs_ptr"]))
    assert dm.live_counts() == {"kf": int(m["kf_alive"].sum()), "lm": int((m["lm_removed"] == 0).sum()),
                                "obs": int(((m["obs_live"] > 0) & (m["lm_removed"][lm] == 0)).sum())}
    assert dm.counts() == {"kf": len(m["kf_id"]), "feat": int(m["kf_feat_ptr"][-1]), "lm": len(m["lm_id"]),
                           "obs": len(m["obs_kf_id"])}
    pose, pos = dm.download()
    assert np.array_equal(pose, m["kf_pose"].reshape(-1, 7))
    rows = got["landmarks"]["row"]
    assert np.array_equal(pos[rows], got["landmarks"]["pw"].reshape(-1, 3))
    old = np.setdiff1d(np.arange(len(pos)), rows)
    assert np.array_equal(pos[old], m["lm_pos"].reshape(-1, 3)[old])
    m["lm_pos"] = m["lm_pos"].reshape(-1, 3)
    m["lm_pos"][rows] = got["landmarks"]["pw"].reshape(-1, 3)
    for k in np.nonzero(m["kf_alive"])[0]:
        uv, lid, fl = dm.keyframe_features(int(m["kf_id"][k]))
        f0, f1 = m["kf_feat_ptr"][k], m["kf_feat_ptr"][k + 1]
        assert np.array_equal(uv, m["feat_uv"].reshape(-1, 2)[f0:f1])
        assert np.array_equal(lid, m["feat_lm_id"][f0:f1]) and np.array_equal(fl, m["feat_flags"][f0:f1])


@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("with_depth", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_sizes(ctx, n, with_depth, form):
    d = R.scene(n, with_depth)
    ref = R.scene_map(d)
    dm = loaded(ctx, ref)
    want = R.create_keyframe(ref, NEW, d["pose2"], d["intr"], d["uv2"], LAST, d["matches"], d["depth"], FIRST)
    got = create(dm, form, NEW, d["pose2"], d["intr"], d["uv2"], LAST, d["matches"], d["depth"], FIRST)
    assert (got["result"]["n_feat"], got["result"]["n_matches"]) == (len(d["uv2"]), len(d["matches"]))
    same_records(got, want, f"n={n} depth={with_depth} {form}:")
    same_state(dm, ref, got)
    dm.close()


def _run(plan):
    plan.run_async()
    return plan.fetch()


edit_scene = R.edit_scene


def track_new(ctx, dm, kf, uv, intr):
    """TrackWithPnP against keyframe kf with a frame that repeats its features"""
    n = len(uv)
    mt = np.zeros(n, vxslam.MATCH_DTYPE)
    mt["query_idx"] = mt["train_idx"] = np.arange(n)
    keep = (dev(uv.astype(np.float32)), dev(np.array([n], np.int32)), dev(mt), dev(np.array([n], np.int32)))
    ctx.track_pnp_async(dm, kf, (keep[0].data_ptr(), 8, keep[1].data_ptr()), intr, vxslam.track_options(),
                        matches=(keep[2].data_ptr(), keep[3].data_ptr(), n))
    out = ctx.track_pnp_fetch()
    del keep
    return out


def same_maps(a, b, kfs):
    assert a.counts() == b.counts() and a.live_counts() == b.live_counts()
    for x, y in zip(a.download(), b.download()):
        assert np.array_equal(x, y)
    for k in kfs:
        for x, y in zip(a.keyframe_features(k), b.keyframe_features(k)):
            assert np.array_equal(x, y)


def same_downstream(ctx, a, b, new, uv, intr):
    """the same LocalBA plan and run, one-call LocalBA, culls and tracking on both maps (bitwise)"""
    ta, tb = track_new(ctx, a, new, uv, intr), track_new(ctx, b, new, uv, intr)
    assert ta[0]["n_pairs"] > 0
    assert ta[0].tobytes() == tb[0].tobytes() and np.array_equal(ta[1], tb[1]) and np.array_equal(ta[2], tb[2])
    bo = vxslam.default_ba_options(window=8, iters=3)
    pa, pb = a.plan(bo), b.plan(bo)
    assert pa.info() == pb.info() and pa.info()["n_kf"] > 0
    sa, sb = _run(pa), _run(pb)
    assert (sa.status, sa.iterations, list(sa.cost), list(sa.obs)) == (sb.status, sb.iterations, list(sb.cost), list(sb.obs))
    pa.apply(a), pb.apply(b)
    for x, y in zip(a.download(), b.download()):
        assert np.array_equal(x, y)
    pa.close(), pb.close()
    oa, ob = a.optimize(bo), b.optimize(bo)
    assert (oa.status, oa.iterations, list(oa.obs)) == (ob.status, ob.iterations, list(ob.obs))
    for x, y in zip(a.download(), b.download()):
        assert np.array_equal(x, y)
    co = vxslam.cull_options(min_landmarks_for_culling=0)
    ca, cb = a.cull_landmarks(co), b.cull_landmarks(co)
    assert len(ca["landmarks"]) > 0
    assert np.array_equal(ca["landmarks"], cb["landmarks"]) and np.array_equal(ca["features"], cb["features"])
    ko = vxslam.cull_options(min_landmarks_for_culling=0, kf_redundant_ratio=0.5, max_keyframes=5,
                             kf_min_shared_observations=2)
    ka, kb = a.cull_keyframes(ko), b.cull_keyframes(ko)
    assert (ka["removed"], ka["kf_id"], ka["ratio"]) == (kb["removed"], kb["kf_id"], kb["ratio"])
    assert np.array_equal(ka["landmarks"], kb["landmarks"]) and np.array_equal(ka["features"], kb["features"])
    assert a.counts() == b.counts() and a.live_counts() == b.live_counts()


def test_equals_the_edit_path(ctx, slot_sums):
    """Two maps from one scene: A takes the one call, B the four edit calls with the restatement's
    decisions and A's positions.  Same counts, arrays, feature rows, LocalBA plan and run (bitwise),
    culls and tracking."""
    m, d, last, new, first = edit_scene()
    a, b = loaded(ctx, m), loaded(ctx, m)
    ref = m.copy()
    want = R.create_keyframe(ref, new, d["pose2"], d["intr"], d["uv2"], last, d["matches"], d["depth"], first)
    assert min(want["margins"].values()) > 1e-9, want["margins"]
    assert want["n_depth"] > 50 and want["n_triangulated"] > 20
    got = create(a, "host", new, d["pose2"], d["intr"], d["uv2"], last, d["matches"], d["depth"], first)
    same_records(got, want, "edit path:")
    same_state(a, ref, got)
    R.apply_edits(b, new, d["pose2"], d["intr"], d["uv2"], last, got["landmarks"])
    same_maps(a, b, (last, new))
    same_downstream(ctx, a, b, new, d["uv2"], d["intr"])
    a.close(), b.close()


def test_host_mirrors_through_the_public_calls(ctx, slot_sums):
    """what the edit calls find in a map the one call wrote: its pairs, ids and feature rows"""
    m, d, last, new, first = edit_scene(62)
    a, b = loaded(ctx, m), loaded(ctx, m)
    got = create(a, "device", new, d["pose2"], d["intr"], d["uv2"], last, d["matches"], d["depth"], first)
    recs = got["landmarks"]
    R.apply_edits(b, new, d["pose2"], d["intr"], d["uv2"], last, recs)
    tri, dep = recs[recs["kind"] == 1], recs[recs["kind"] == 0]
    assert len(tri) and len(dep)
    live = a.live_counts()["obs"]
    for x in (a, b):
        x.remove_observations([tri["lm_id"][0]], [last])     # a created pair: gone once ...
        assert x.live_counts()["obs"] == live - 1
        x.remove_observations([tri["lm_id"][0]], [last])     # ... and absent the second time
        assert x.live_counts()["obs"] == live - 1
        x.add_observations([dep["lm_id"][0]], [last], [3])   # a created landmark id is known
        assert x.live_counts()["obs"] == live
        x.set_features(new, [int(dep["feat_curr"][0])], [0], [2])
        with pytest.raises(vxslam.VxError):
            x.add_keyframe(new, d["pose2"], d["intr"], 1, d["uv2"], np.zeros(300, np.uint64), np.zeros(300, np.uint8))
        with pytest.raises(vxslam.VxError):
            x.add_landmarks([recs["lm_id"][-1]], np.zeros((1, 3)))
    same_maps(a, b, (last, new))
    same_downstream(ctx, a, b, new, d["uv2"], d["intr"])
    a.close(), b.close()


def frame_before(d, seed):
    """a frame 8 cm before the scene's first one that sees the same points: (pose, positions, matches
    frame 0 -> frame 1 with unique queries)"""
    rng = np.random.default_rng(seed)
    n = len(d["uv1"])
    q1, t1 = d["pose1"][:4], d["pose1"][4:]
    R1 = synth.quat_to_mat(q1)
    t0 = -R1 @ (-R1.T @ t1 - np.array([0.08, 0.01, 0.0]))
    pc = d["pw_true"] @ R1.T + t0
    fx, fy, cx, cy = d["intr"]
    uv0 = np.stack([fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy], -1) + rng.normal(0, 0.3, (n, 2))
    mt = np.zeros(int(0.8 * n), vxslam.MATCH_DTYPE)
    mt["query_idx"] = mt["train_idx"] = np.sort(rng.choice(n, len(mt), replace=False))
    return np.concatenate([q1, t0]), uv0.astype(np.float32).astype(np.float64), mt


def with_holes(depth, uv, seed):
    """the depth image with a hole under half of the positions"""
    rng = np.random.default_rng(seed)
    out = depth.copy()
    px = (uv + 0.5).astype(np.int64)
    ok = (px[:, 0] >= 0) & (px[:, 0] < out.shape[1]) & (px[:, 1] >= 0) & (px[:, 1] < out.shape[0]) & (rng.random(len(uv)) < 0.5)
    out[px[ok, 1], px[ok, 0]] = 0
    return out


def test_three_keyframe_chain_from_an_empty_map(ctx, slot_sums):
    """has_last = 0, then last = 1, then last = 2: every array grows from nothing, the third call
    meets a last keyframe with depth and triangulated links, one call runs on a second context, one
    reads KEYPOINT_DTYPE rows; landmark ids continue; the final map is the edit path's."""
    d = synth.make_keyframe_scene(71, 700)
    pose0, uv0, m01 = frame_before(d, 710)
    ctx2 = vxslam.Context(0)
    a, b = vxslam.DMap(ctx), vxslam.DMap(ctx)
    ref = R.scene_map(d)
    for k in ("kf_id", "kf_alive", "kf_has_cam", "feat_lm_id", "feat_flags"):
        ref[k] = ref[k][:0]
    ref["kf_pose"], ref["kf_intr"], ref["feat_uv"] = np.zeros((0, 7)), np.zeros((0, 4)), np.zeros((0, 2))
    ref["kf_feat_ptr"] = np.zeros(1, np.int64)
    steps = [(1, pose0, uv0, None, None, with_holes(d["depth"], uv0, 711), "host", None, False),
             (2, d["pose1"], d["uv1"], 1, m01, with_holes(d["depth"], d["uv1"], 712), "device", ctx2, False),
             (3, d["pose2"], d["uv2"], 2, d["matches"], None, "device", None, True)]
    first = 1
    for kid, pose, uv, last, mt, depth, form, c, kp in steps:
        want = R.create_keyframe(ref, kid, pose, d["intr"], uv, last, mt, depth, first)
        assert min(want["margins"].values()) > 1e-9, want["margins"]
        got = create(a, form, kid, pose, d["intr"], uv, last, mt, depth, first, ctx=c, keypoint_rows=kp)
        assert got["result"]["first_landmark_id"] == first
        same_records(got, want, f"chain kf {kid}:")
        same_state(a, ref, got)
        R.apply_edits(b, kid, pose, d["intr"], uv, last, got["landmarks"])
        same_maps(a, b, range(1, kid + 1))
        first = int(got["result"]["next_landmark_id"])
        if kid == 1:
            assert want["n_triangulated"] == 0 and want["n_depth"] > 100
        if kid == 2:
            assert want["n_triangulated"] > 20 and want["n_depth"] > 100
        if kid == 3:  # frame 2 carried both kinds of links when frame 3 arrived
            assert want["n_triangulated"] > 20 and want["n_depth"] == 0
    bo = vxslam.default_ba_options(window=3, iters=2)
    oa, ob = a.optimize(bo), b.optimize(bo)
    assert (oa.status, oa.iterations, list(oa.obs)) == (ob.status, ob.iterations, list(ob.obs))
    same_maps(a, b, (1, 2, 3))
    # nothing was matched on ctx2, and no list is given
    keep = (dev(np.zeros((4, 2), np.float32)), dev(np.array([4], np.int32)))
    with pytest.raises(vxslam.VxError) as e:
        a.create_keyframe(4, d["pose2"], d["intr"], (keep[0].data_ptr(), 8, keep[1].data_ptr(), 4), last_kf_id=3,
                          first_landmark_id=first, ctx=ctx2)
    assert e.value.code == vxslam.VX_ERR_STATE
    a.close(), b.close()
    ctx2.close()


def snapshot(dm, kfs):
    p = dm.plan(vxslam.default_ba_options(window=8, iters=1))
    info = p.info()
    p.close()
    return (dm.counts(), dm.live_counts(), [x.copy() for x in dm.download()], info,
            [[x.copy() for x in dm.keyframe_features(k)] for k in kfs])


def same_snapshot(x, y):
    assert x[0] == y[0] and x[1] == y[1] and x[3] == y[3]
    for p, q in zip(x[2], y[2]):
        assert np.array_equal(p, q)
    for f, g in zip(x[4], y[4]):
        for p, q in zip(f, g):
            assert np.array_equal(p, q)


@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("case", ["dup_query", "train_range", "kf_live", "no_last"])
def test_rejected_input_leaves_the_map(ctx, case, form):
    m, d, last, new, first = edit_scene(63)
    dm = loaded(ctx, m)
    before = snapshot(dm, (last,))
    mt = d["matches"].copy()
    kid, lk, bit = new, last, 0
    if case == "dup_query":
        mt["query_idx"][mt.size // 2] = mt["query_idx"][3]
        bit = vxslam.KF_ERR_DUP_QUERY
    elif case == "train_range":
        mt["train_idx"][mt.size - 1] = len(d["uv2"])
        bit = vxslam.KF_ERR_MATCH_RANGE
    elif case == "kf_live":
        kid, bit = int(m["kf_id"][0]), vxslam.KF_ERR_KF_LIVE
    else:
        lk, bit = 4040, vxslam.KF_ERR_NO_LAST
    want = R.create_keyframe(m.copy(), kid, d["pose2"], d["intr"], d["uv2"], lk, mt, d["depth"], first)
    assert want["error_bits"] == bit
    with pytest.raises(vxslam.VxError) as e:
        create(dm, form, kid, d["pose2"], d["intr"], d["uv2"], lk, mt, d["depth"], first)
    assert e.value.code == vxslam.VX_ERR_INVALID
    assert dm.last_create["error_bits"] == bit and len(dm.create_results()) == 0
    same_snapshot(snapshot(dm, (last,)), before)
    ref = m.copy()
    want = R.create_keyframe(ref, new, d["pose2"], d["intr"], d["uv2"], last, d["matches"], d["depth"], first)
    got = create(dm, form, new, d["pose2"], d["intr"], d["uv2"], last, d["matches"], d["depth"], first)
    same_records(got, want, f"after {case}:")
    same_state(dm, ref, got)
    dm.close()


@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("dt", ["u16", "f32", "f64"])
def test_depth_edges(ctx, dt, form):
    """test_depth_landmarks_edges' cases through the new call: image types, a padded row stride, a
    position that rounds to `cols`, negative positions"""
    d = dict(synth.make_keyframe_scene(22, 300, depth_type=dt))
    uv = d["uv2"].copy()
    uv[:16] = [[-1.75, 12.0]] * 16         # truncates to pixel column -1: outside
    uv[16:20] = [[639.5, 100.25]] * 4      # rounds to cols: outside
    uv[20:24] = [[639.25, 479.25]] * 4     # the last pixel
    uv[24:28] = [[-0.75, -0.25]] * 4       # (int)(-0.25) = 0, (int)(0.25) = 0: pixel (0, 0), inside
    padded = np.zeros((480, 700), d["depth"].dtype)
    padded[:, :640] = d["depth"]
    for depth in (d["depth"], padded[:, :640]):
        ref = R.scene_map(d)
        dm = loaded(ctx, ref)
        want = R.create_keyframe(ref, NEW, d["pose2"], d["intr"], uv, LAST, d["matches"], depth, FIRST)
        dep = want["landmarks"][want["landmarks"]["kind"] == 0]["feat_curr"]
        assert not np.isin(np.arange(20), dep).any() and np.isin(np.arange(20, 28), dep).all()
        got = create(dm, form, NEW, d["pose2"], d["intr"], uv, LAST, d["matches"], depth, FIRST)
        same_records(got, want, f"depth {dt} {form}:")
        same_state(dm, ref, got)
        dm.close()


def test_slot_and_the_contexts_own_match_list(ctx):
    """extract -> match -> create with nothing fetched between (an extraction slot's keypoint rows,
    the context's last match list) equals the restatement on the fetched keypoints and matches"""
    import torch

    frames = synth.make_frames(43, 2, 240, 320)
    p = vxslam.default_orb_params(n_features=500)
    dimg = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    for slot in range(2):
        ctx.orb_extract_async(dimg[slot].data_ptr(), 320, 240, 3, 320 * 3, slot, p)
    ctx.match_slots_async(0, 1)
    k0, _ = ctx.orb_fetch(0)
    k1, _ = ctx.orb_fetch(1)
    mt = ctx.match_fetch()
    assert len(mt) >= 20
    intr = np.array([260.0, 260.0, 160.0, 120.0])
    pose1 = np.array([0, 0, 0, 1.0, 0, 0, 0])
    pose2 = np.array([0, 0, 0, 1.0, -0.05, 0, 0])
    d = {"uv1": np.stack([k0["x"], k0["y"]], -1).astype(np.float64), "has1": np.zeros(len(k0), np.uint8),
         "pose1": pose1, "intr": intr}
    ref = R.scene_map(d)
    dm = loaded(ctx, ref)
    uv2 = np.stack([k1["x"], k1["y"]], -1).astype(np.float64)
    o = vxslam.keyframe_options(tri_min_angle_deg=0.05, tri_max_reproj_error=50.0)
    want = R.create_keyframe(ref, NEW, pose2, intr, uv2, LAST, mt, None, FIRST, o)
    print("slot scene:", len(mt), "matches,", want["n_triangulated"], "triangulated, margins", want["margins"])
    assert min(want["margins"].values()) > 1e-9
    got = dm.create_keyframe(NEW, pose2, intr, 1, last_kf_id=LAST, first_landmark_id=FIRST, opts=o)
    assert got["result"]["n_feat"] == len(k1) and got["result"]["n_matches"] == len(mt)
    same_records(got, want, "slot:")
    same_state(dm, ref, got)
    dm.close()


def test_profiling_stages(ctx):
    d = R.scene(65, True)
    dm = loaded(ctx, R.scene_map(d))
    ctx.prof_enable(True, ["kf_features", "kf_matches", "kf_commit"])
    create(dm, "host", NEW, d["pose2"], d["intr"], d["uv2"], LAST, d["matches"], d["depth"], FIRST)
    p = ctx.prof_read()
    ctx.prof_enable(False)
    for k in ("kf_features", "kf_matches", "kf_commit"):
        assert p[k][1] == 1 and p[k][0] > 0.0, (k, p[k])
    dm.close()
