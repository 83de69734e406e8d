"""GPU parity of map culling on the resident map (vx_dmap_cull_landmarks / vx_dmap_keyframe_redundancy /
vx_dmap_cull_keyframes, csrc/cull.hip) against the numpy restatement of tracking.cpp:652-840
(tests/cull_ref.py, pinned by tests/test_cull_cpu.py).

Every comparison is exact: the records equal the restatement's (array_equal; mean_err within 1e-12
relative: the same IEEE terms summed in the same order, the projection's operations possibly fused
differently), and the map afterwards equals a map edited through the calls that existed before.  That
is legitimate because every scene first asserts, on the CPU, that each observation error is further
than 1e-9 (relative) from 2 tau, each mean from tau and each pc.z from 1e-6 (synth.cull_margins):
seven orders of magnitude above what a different rounding order can move."""
import ctypes as C

import numpy as np
import pytest

import vxslam
from vxslam import synth

import cull_ref
from track_ref import track_ref

pytestmark = pytest.mark.gpu

MARGIN = 1e-9


def scene(seed, n_kf, n_lm, tau=5.0, **kw):
    m = synth.make_cull_scene(seed, n_kf, n_lm, tau=tau, min_margin=MARGIN, **kw)
    assert min(m["margins"].values()) > MARGIN
    return m


def loaded(ctx, m):
    dm = vxslam.DMap(ctx)
    cull_ref.load(dm, m)
    return dm


def same_records(got, want):
    gl, wl = got["landmarks"], want["landmarks"]
    for k in ("lm_id", "row", "reason", "n_projected", "reserved"):
        assert np.array_equal(gl[k], wl[k]), k
    assert np.all(np.diff(gl["row"]) > 0)
    nz = wl["mean_err"] != 0
    print("mean_err:", int(nz.sum()), "values, largest relative difference",
          float((np.abs(gl["mean_err"] - wl["mean_err"])[nz] / wl["mean_err"][nz]).max()) if nz.any() else 0.0)
    assert np.all(np.abs(gl["mean_err"] - wl["mean_err"]) <= 1e-12 * np.abs(wl["mean_err"]))
    assert np.array_equal((gl["mean_err"] != 0), (gl["reason"] == vxslam.CULL_MEAN_ERROR))
    assert np.array_equal(got["features"], want["features"])


def same_state(dm, m):
    """the resident map's membership against the restatement's edited dict"""
    live = dm.live_counts()
    lm = np.repeat(np.arange(len(m["lm_id"])), np.diff(m["lm_obs_ptr"]))
    assert live == {"kf": int(m["kf_alive"].sum()), "lm": int((m["lm_removed"] == 0).sum()),
                    "obs": int(((m["obs_live"] > 0) & (m["lm_removed"][lm] == 0)).sum())}


def reasons(res):
    return np.bincount(res["landmarks"]["reason"], minlength=6)[1:].tolist()


@pytest.fixture(scope="module")
def special():
    """10 + 2 keyframes / 2000 landmarks with the hand-placed cases, and the restatement's result"""
    m = scene(0xC011, 10, 2000)
    ref = m.copy()
    res = cull_ref.cull_landmarks(ref, vxslam.cull_options())
    return m, ref, res


def test_special_cases_reach_their_branches(special):
    """(no device: what the hand-placed cases of the scene do in the restatement)"""
    m, ref, res = special
    why = {int(r): int(w) for r, w in zip(res["landmarks"]["row"], res["landmarks"]["reason"])}
    n_proj = {int(r): int(w) for r, w in zip(res["landmarks"]["row"], res["landmarks"]["n_projected"])}
    sp = m["special"]
    for name in ("dead_kf", "reinserted", "oor", "other", "nohas_keep", "behind", "nocam", "wave_keep"):
        assert sp[name] not in why, name
    for name in ("reinserted_bad", "oor_cull", "other_cull", "nohas_cull", "wave_cull"):
        assert why[sp[name]] == vxslam.CULL_LARGE_ERROR, name
    assert n_proj[sp["wave_cull"]] == 70  # the large error is the last of 70
    assert why[sp["all_skipped"]] == why[sp["all_skipped_reset"]] == vxslam.CULL_NO_PROJECTION
    assert why[sp["mean"]] == vxslam.CULL_MEAN_ERROR
    assert sp["removed"] not in why
    ft = res["features"]
    kf = m["special_kf"]
    rows = lambda name: ft[np.isin(ft["kf_row"], [kf[name]])]
    assert len(rows("D")) == 0 and len(rows("Y_dead")) == 0      # no feature of a dead row is touched
    assert len(rows("Y")) == 1 and len(rows("C")) == 1           # reinserted_bad; all_skipped_reset (no camera)
    assert all(c > 0 for c in reasons(res)), reasons(res)        # all five reasons occur
    assert reasons(res)[0] == 20 and reasons(res)[1] == 60       # (make_ba_map's bad / single-observation landmarks)


def test_cull_landmarks_special_scene(ctx, special):
    m, ref, res = special
    dm = loaded(ctx, m)
    before = dm.counts()
    got = dm.cull_landmarks()
    same_records(got, res)
    same_state(dm, ref)
    assert dm.counts() == before  # rows stay as dead storage
    # the lists may be read again: too small arrays give the capacity error with the counts set
    one_lm, one_ft = np.zeros(1, vxslam.CULL_LANDMARK_DTYPE), np.zeros(1, vxslam.CULL_FEATURE_DTYPE)
    nl, nf = C.c_int(0), C.c_int(0)
    rc = vxslam.lib().vx_dmap_cull_results(dm.handle, 1, one_lm.ctypes.data, 1, one_ft.ctypes.data, C.byref(nl), C.byref(nf))
    assert rc == -3 and (nl.value, nf.value) == (len(res["landmarks"]), len(res["features"]))  # VX_ERR_CAPACITY
    lm2, ft2 = dm.cull_results()
    assert lm2.tobytes() == got["landmarks"].tobytes() and ft2.tobytes() == got["features"].tobytes()
    again = dm.cull_landmarks()   # nothing left to cull
    assert len(again["landmarks"]) == 0 and len(again["features"]) == 0
    # two fresh maps: the same bytes
    dm2 = loaded(ctx, m)
    got2 = dm2.cull_landmarks()
    assert got2["landmarks"].tobytes() == got["landmarks"].tobytes()
    assert got2["features"].tobytes() == got["features"].tobytes()
    dm.close(), dm2.close()


def sizes():
    b = vxslam.cull_block()
    return [1, 63, 64, 65, b - 1, b, b + 1]


@pytest.mark.parametrize("which", range(7))
def test_cull_landmarks_sizes(ctx, which):
    n = sizes()[which]
    m = scene(0xC100 + which, 4, n, special=False, lm_sigma=0.03, frac_bad=0.1, frac_single=0.1)
    o = vxslam.cull_options(min_landmarks_for_culling=0)
    ref = m.copy()
    want = cull_ref.cull_landmarks(ref, o)
    if n >= 63:
        assert 0 < len(want["landmarks"]) < n
    dm = loaded(ctx, m)
    same_records(dm.cull_landmarks(o), want)
    same_state(dm, ref)
    dm.close()


@pytest.mark.parametrize("sigma", [0.01, 0.03])
def test_cull_landmarks_2000(ctx, sigma):
    m = scene(0xC011, 10, 2000, special=False, lm_sigma=sigma)
    ref = m.copy()
    want = cull_ref.cull_landmarks(ref, vxslam.cull_options())
    assert reasons(want) == ([20, 60, 0, 20, 112] if sigma == 0.01 else [20, 60, 0, 277, 459])
    dm = loaded(ctx, m)
    same_records(dm.cull_landmarks(), want)
    same_state(dm, ref)
    dm.close()


def test_cull_landmarks_table_in_global_memory(ctx):
    """more live keyframes than the scan holds in LDS: the other kernel instance"""
    nk = vxslam.cull_lds_keyframes() + 1
    m = scene(0xC012, nk - 2, 600, special=False, lm_sigma=0.03)
    assert int(m["kf_alive"].sum()) > vxslam.cull_lds_keyframes()
    ref = m.copy()
    o = vxslam.cull_options()
    want = cull_ref.cull_landmarks(ref, o)
    assert len(want["landmarks"]) > 50
    dm = loaded(ctx, m)
    same_records(dm.cull_landmarks(o), want)
    dm.close()


def test_gate_at_199_and_200(ctx):
    for n, runs in ((199, False), (200, True)):
        m = scene(0xC200, 4, n, special=False, lm_sigma=0.03)
        ref = m.copy()
        want = cull_ref.cull_landmarks(ref, vxslam.cull_options())
        assert (len(want["landmarks"]) > 0) == runs
        dm = loaded(ctx, m)
        same_records(dm.cull_landmarks(), want)
        same_state(dm, ref)
        dm.close()


def test_nothing_and_everything_culled(ctx):
    m = scene(0xC300, 4, 300, special=False, frac_bad=0.0, tau=1e6)
    dm = loaded(ctx, m)
    o = vxslam.cull_options(min_landmark_observations=0, landmark_max_reproj_error=1e6)
    assert len(cull_ref.cull_landmarks(m.copy(), o)["landmarks"]) == 0
    got = dm.cull_landmarks(o)
    assert len(got["landmarks"]) == 0 and len(got["features"]) == 0 and dm.live_counts()["lm"] == 300
    dm.close()
    m = scene(0xC300, 4, 300, special=False, tau=1e-3)
    o = vxslam.cull_options(landmark_max_reproj_error=1e-3)
    ref = m.copy()
    want = cull_ref.cull_landmarks(ref, o)
    assert len(want["landmarks"]) == 300
    dm = loaded(ctx, m)
    same_records(dm.cull_landmarks(o), want)
    assert dm.live_counts()["lm"] == 0 and dm.live_counts()["obs"] == 0
    dm.close()


KF_LOOSE = dict(kf_redundant_ratio=0.5, max_keyframes=5, kf_min_shared_observations=2)


def _run(plan):
    plan.run_async()
    return plan.fetch()


@pytest.mark.parametrize("what", ["landmarks", "keyframes"])
def test_equals_the_edit_path(ctx, special, what, slot_sums):
    """Two maps from one scene: one culled on the device, the other edited with the restatement's
    decisions through set_landmark_bad / set_features / remove_landmarks / remove_observations /
    remove_keyframe.  Same counts, same arrays, the same LocalBA plan and run (bitwise)."""
    m = special[0]
    a, b = loaded(ctx, m), loaded(ctx, m)
    ref = m.copy()
    if what == "landmarks":
        o = vxslam.cull_options()
        want = cull_ref.cull_landmarks(ref, o)
        got = a.cull_landmarks(o)
    else:
        o = vxslam.cull_options(**KF_LOOSE)
        want = cull_ref.cull_keyframes(ref, o)
        assert want["removed"] and len(want["removed_obs"]) > 100 and len(want["landmarks"]) > 100
        got = a.cull_keyframes(o)
        assert (got["removed"], got["kf_id"], got["ratio"]) == (True, want["kf_id"], want["ratio"])
    same_records(got, want)
    cull_ref.apply_edits(b, want)
    same_state(a, ref)
    assert a.counts() == b.counts() and a.live_counts() == b.live_counts()
    for x, y in zip(a.download(), b.download()):
        assert np.array_equal(x, y)
    bo = vxslam.default_ba_options(window=8, iters=3)
    pa, pb = a.plan(bo), b.plan(bo)
    assert pa.info() == pb.info() and pa.info()["n_kf"] > 0
    sa, sb = _run(pa), _run(pb)
    assert (sa.status, sa.iterations, list(sa.cost), list(sa.obs)) == (sb.status, sb.iterations, list(sb.cost), list(sb.obs))
    pa.apply(a), pb.apply(b)
    for x, y in zip(a.download(), b.download()):
        assert np.array_equal(x, y)
    pa.close(), pb.close()
    ta, tb = a.optimize(bo), b.optimize(bo)
    assert (ta.status, ta.iterations, list(ta.obs)) == (tb.status, tb.iterations, list(tb.obs))
    assert a.counts() == b.counts() and a.live_counts() == b.live_counts()
    a.close(), b.close()


def _with_empty_keyframe(m):
    """a keyframe none of whose features holds a landmark (total == 0), as the last row"""
    m["kf_id"] = np.append(m["kf_id"], np.uint64(int(m["kf_id"].max()) + 5))
    m["kf_pose"] = np.concatenate([m["kf_pose"].reshape(-1, 7), m["kf_pose"].reshape(-1, 7)[:1]])
    m["kf_intr"] = np.concatenate([m["kf_intr"].reshape(-1, 4), m["kf_intr"].reshape(-1, 4)[:1]])
    m["kf_has_cam"] = np.append(m["kf_has_cam"], np.uint8(1))
    m["kf_alive"] = np.append(m["kf_alive"], np.uint8(1))
    m["kf_feat_ptr"] = np.append(m["kf_feat_ptr"], m["kf_feat_ptr"][-1] + 3)
    m["feat_uv"] = np.concatenate([m["feat_uv"].reshape(-1, 2), np.zeros((3, 2))])
    m["feat_lm_id"] = np.concatenate([m["feat_lm_id"], np.array([0, 5, m["lm_id"][0]], np.uint64)])
    m["feat_flags"] = np.concatenate([m["feat_flags"], np.array([0, 2, 0], np.uint8)])
    return m


@pytest.mark.parametrize("nk", [3, 4, 35])
def test_keyframe_redundancy(ctx, nk):
    m = _with_empty_keyframe(scene(0xC400 + nk, nk - 3, 40 * nk, special=False, frac_bad=0.05))
    gone = np.arange(0, len(m["lm_id"]), 7)  # removed landmarks that features still name
    m["lm_removed"][gone] = 1
    assert int(m["kf_alive"].sum()) == nk
    dm = loaded(ctx, m)
    for o in (vxslam.cull_options(), vxslam.cull_options(kf_min_shared_observations=2)):
        want = cull_ref.keyframe_redundancy(m, o)
        got = dm.keyframe_redundancy(o)
        for k in ("kf_id", "total", "redundant"):
            assert np.array_equal(got[k], want[k]), k
        assert want["total"][-1] == 0 and (want["total"][:-1] > want["redundant"][:-1]).all()
    assert want["redundant"].sum() > 0
    dm.close()


def test_keyframe_redundancy_special_scene(ctx, special):
    m = special[0]
    dm = loaded(ctx, m)
    o = vxslam.cull_options(kf_min_shared_observations=2)
    want = cull_ref.keyframe_redundancy(m, o)
    got = dm.keyframe_redundancy(o)
    for k in ("kf_id", "total", "redundant"):
        assert np.array_equal(got[k], want[k]), k
    assert len(got["kf_id"]) == int(m["kf_alive"].sum()) and np.all(np.diff(got["kf_id"].astype(np.int64)) > 0)
    assert 0 in want["total"].tolist()
    assert dm.counts() == loaded(ctx, m).counts()  # no edit
    dm.close()


def test_cull_keyframes_rules(ctx, special):
    m = special[0]
    base = [int(i) for i, a in zip(m["kf_id"], m["kf_alive"]) if a and i < 1000]
    s0 = int(m["kf_id"][m["special_kf"]["S0"]])
    cases = [
        (vxslam.cull_options(kf_redundant_ratio=1.0), (), False),                       # nobody qualifies
        (vxslam.cull_options(min_landmarks_for_culling=10 ** 6, **KF_LOOSE), (), True),  # trailing gate closed
        (vxslam.cull_options(**KF_LOOSE), base[:2], True),                              # protected ids
        (vxslam.cull_options(**KF_LOOSE), base, True),                                  # ... down to S0
        (vxslam.cull_options(min_keyframes_for_culling=10 ** 4, **KF_LOOSE), (), False),  # keyframe gate
    ]
    for i, (o, protect, removed) in enumerate(cases):
        ref = m.copy()
        want = cull_ref.cull_keyframes(ref, o, protect)
        assert want["removed"] == removed, i
        dm = loaded(ctx, m)
        got = dm.cull_keyframes(o, protect)
        assert (got["removed"], got["kf_id"], got["ratio"]) == (want["removed"], want["kf_id"], want["ratio"]), i
        same_records(got, want)
        same_state(dm, ref)
        if i == 1:
            assert len(want["landmarks"]) == 0 and len(want["features"]) > 100 and want["kf_id"] == base[0]
        if i == 2:
            assert want["kf_id"] == base[2] and len(want["landmarks"]) > 0
        if i == 3:
            # S0 holds a feature whose landmark was removed from the map: left as it is (:763)
            k = m["special_kf"]["S0"]
            f0, f1 = m["kf_feat_ptr"][k], m["kf_feat_ptr"][k + 1]
            rid = m["lm_id"][m["special"]["removed"]]
            left = np.nonzero(ref["feat_lm_id"][f0:f1] == rid)[0]
            assert want["kf_id"] == s0 and len(left) == 1 and ref["feat_flags"][f0 + left[0]] == 1
            assert int(left[0]) not in want["kf_features"]
        # the device map agrees feature by feature: a second, gated-off redundancy pass sees the same flags
        o2 = vxslam.cull_options(kf_min_shared_observations=2)
        w2, g2 = cull_ref.keyframe_redundancy(ref, o2), dm.keyframe_redundancy(o2)
        for k in ("kf_id", "total", "redundant"):
            assert np.array_equal(g2[k], w2[k]), (i, k)
        dm.close()


def dev(a):
    import torch

    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.from_numpy(np.concatenate([b, np.zeros(16, np.uint8)])).cuda()
    torch.cuda.synchronize()
    return t


def test_chain_track_second_context_and_growth(ctx, special):
    m, _, _ = special
    ref = m.copy()
    dm = loaded(ctx, m)
    other = vxslam.Context(0)
    o = vxslam.cull_options()
    same_records(dm.cull_landmarks(o, ctx=other), cull_ref.cull_landmarks(ref, o))  # a second context
    same_state(dm, ref)
    # TrackWithPnP's pair gather over a keyframe of the culled map: the pairs of the edited scene
    k = 5
    kid = int(m["kf_id"][k])
    f0, f1 = ref["kf_feat_ptr"][k], ref["kf_feat_ptr"][k + 1]
    uv = ref["feat_uv"].reshape(-1, 2)[f0:f1]
    n = f1 - f0
    assert (ref["feat_flags"][f0:f1] != m["feat_flags"][f0:f1]).any()  # the cull reset some of its features
    curr = (uv + [3.0, 4.0]).astype(np.float32)
    matches = np.zeros(n, vxslam.MATCH_DTYPE)
    matches["query_idx"] = matches["train_idx"] = np.arange(n)
    matches["distance"] = 5.0
    lms = {int(i): (p, int(b)) for i, p, b, r in zip(ref["lm_id"], ref["lm_pos"].reshape(-1, 3), ref["lm_bad"],
                                                     ref["lm_removed"]) if not r}
    topt = vxslam.track_options(min_matches=1, min_inliers=10 ** 6)  # (the gather only: PnP gated off)
    want = track_ref(matches, uv, ref["feat_lm_id"][f0:f1], ref["feat_flags"][f0:f1], curr, lms, 1, 10 ** 6)
    keep = (dev(curr), dev(np.array([n], np.int32)), dev(matches), dev(np.array([n], np.int32)))
    ctx.track_pnp_async(dm, kid, (keep[0].data_ptr(), 8, keep[1].data_ptr()), m["kf_intr"].reshape(-1, 4)[k], topt,
                        matches=(keep[2].data_ptr(), keep[3].data_ptr(), n))
    res, pm, _ = ctx.track_pnp_fetch()
    assert res["n_pairs"] == want["n_pairs"] > 0 and np.array_equal(pm, want["pair_match"])
    assert res["status"] == vxslam.TRACK_FEW_PAIRS
    # the map grows after the cull (new landmarks, observations, features pointing at them) and is culled again
    rng = np.random.default_rng(3)
    ka, kb = 6, 7
    new_ids = np.arange(77_000_001, 77_000_041, dtype=np.uint64)
    pos = ref["lm_pos"].reshape(-1, 3)[:40] + rng.normal(0, 0.05, (40, 3))
    free = {q: np.nonzero((ref["feat_flags"][ref["kf_feat_ptr"][q]:ref["kf_feat_ptr"][q + 1]] & 1) == 0)[0][:40] for q in (ka, kb)}
    o0, l0 = len(ref["obs_kf_id"]), len(ref["lm_id"])
    ref["lm_id"] = np.concatenate([ref["lm_id"], new_ids])
    ref["lm_pos"] = np.concatenate([ref["lm_pos"].reshape(-1, 3), pos])
    ref["lm_bad"] = np.concatenate([ref["lm_bad"], np.zeros(40, np.uint8)])
    ref["lm_removed"] = np.concatenate([ref["lm_removed"], np.zeros(40, np.uint8)])
    ref["lm_obs_ptr"] = np.concatenate([ref["lm_obs_ptr"], o0 + 2 * np.arange(1, 41)]).astype(np.int64)
    okf = np.tile(np.array([m["kf_id"][ka], m["kf_id"][kb]], np.uint64), 40)
    ofi = np.stack([free[ka], free[kb]], -1).reshape(-1).astype(np.uint64)
    ref["obs_kf_id"] = np.concatenate([ref["obs_kf_id"], okf])
    ref["obs_feat_idx"] = np.concatenate([ref["obs_feat_idx"], ofi])
    ref["obs_live"] = np.concatenate([ref["obs_live"], np.ones(80, np.uint8)])
    dm.add_landmarks(new_ids, pos)
    dm.add_observations(np.repeat(new_ids, 2), okf, ofi)
    for q in (ka, kb):
        g = ref["kf_feat_ptr"][q] + free[q]
        ref["feat_lm_id"][g] = new_ids
        ref["feat_flags"][g] = 1
        dm.set_features(int(m["kf_id"][q]), free[q].astype(np.int32), new_ids, np.ones(40, np.uint8))
    assert min(synth.cull_margins(ref).values()) > MARGIN
    want = cull_ref.cull_landmarks(ref, o)
    assert 0 < len(want["landmarks"]) <= 40 and want["landmarks"]["row"].min() >= l0
    same_records(dm.cull_landmarks(o), want)
    same_state(dm, ref)
    del keep
    other.close(), dm.close()
