"""Relocalisation: one PnP over the landmarks of up to 16 keyframes (vx_relocalize_async / vx_relocalize_fetch,
csrc/reloc.hip).  The yardsticks are never the call itself:
  (i)   vx_track_pnp_host_async + vx_track_pnp_fetch per candidate (and vx_match_fetch for its match list): the
        per-candidate fields, byte for byte;
  (ii)  tests/reloc_ref.py on those calls' match lists and pair_match arrays: n_pool and the three provenance
        arrays, equal;
  (iii) vx_pnp_ransac on the restated pooled arrays (obj = the landmark behind the pooled match's keyframe
        feature as float32, img = the current pixel of pool_train), max_iterations = min(100, 2 n_pool): the PnP
        record and the mask, byte for byte; zeros when the restatement says PnP does not run.
Every placed case first asserts its own premise on the restatement.

Candidates are derived from ONE scene (synth.make_track_frame_scene, 300 features): every candidate keyframe has
the scene's features and landmarks; per candidate `flips[i]` places the Hamming distance of feature i to its
current keypoint (-1: a random row, which matches nothing) and `flags` chooses which features keep their landmark.
All candidates live in one DMap as keyframes KF0 + c."""
import ctypes as C

import numpy as np
import pytest

import vxslam
from vxslam import synth

import reloc_ref

pytestmark = pytest.mark.gpu

N = 300
KF0 = 500
OK, FEW_MATCHES, FEW_PAIRS = vxslam.TRACK_OK, vxslam.TRACK_FEW_MATCHES, vxslam.TRACK_FEW_PAIRS


def d2h(ctx, ptr, dtype, n):
    ctx.synchronize()
    out = np.zeros(max(n, 1), dtype)
    assert vxslam.lib().hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(out.nbytes), C.c_int(2)) == 0
    return out[:n]


def dev_list(ctx, triple):
    ptr, n_ptr, cap = triple
    n = int(d2h(ctx, n_ptr, np.int32, 1)[0])
    assert 0 <= n <= cap
    return d2h(ctx, ptr, vxslam.MATCH_DTYPE, n)


def flipped(desc_curr, train_of, flips, rng):
    """row i = the current keypoint train_of[i]'s row with flips[i] bits flipped; flips[i] < 0: a random row"""
    bits = np.unpackbits(desc_curr[train_of], axis=1)
    for i, f in enumerate(flips):
        if f < 0:
            bits[i] = rng.integers(0, 2, 256)
        else:
            bits[i, rng.choice(256, int(f), replace=False)] ^= 1
    return np.packbits(bits, axis=1)


CLOSED = dict(flips=np.full(N, -1))


class World:
    """one scene, its current frame and its candidate keyframes on the device, one map"""

    def __init__(self, ctx, seed, cands, curr_cap=N + 23, extra_rows=0, **scene_kw):
        self.ctx = ctx
        s = self.s = synth.make_track_frame_scene(seed, N, **scene_kw)
        rng = np.random.default_rng([seed, 0xE10C])
        self.curr_xy, self.desc_curr = s["curr_xy"], s["desc_curr"]
        if extra_rows:  # unrelated rows after the scene's
            self.curr_xy = np.concatenate([self.curr_xy, rng.uniform(0, 480, (extra_rows, 2)).astype(np.float32)])
            self.desc_curr = np.concatenate([self.desc_curr, rng.integers(0, 256, (extra_rows, 32), dtype=np.uint8)])
        self.curr = vxslam.Frame(ctx, curr_cap).upload(ctx, self.curr_xy, self.desc_curr)
        self.dm = vxslam.DMap(ctx)
        self.dm.add_landmarks(s["lm_id"], s["lm_pos"], None)
        self.cands = []
        for c, k in enumerate(cands):
            flips = np.asarray(k.get("flips", s["flips"]))
            train_of = np.asarray(k.get("train_of", s["train_of"]))
            flags = np.asarray(k.get("flags", s["flags"]), np.uint8)
            desc = flipped(s["desc_curr"], train_of, flips, rng)
            fr = vxslam.Frame(ctx, k.get("cap", N + 20)).upload(ctx, s["kf_uv"].astype(np.float32), desc)
            self.dm.add_keyframe(KF0 + c, s["pose"], s["intr"], True, s["kf_uv"], s["lm_id"], flags)
            self.cands.append({"kf_id": KF0 + c, "frame": fr, "desc": desc, "flags": flags})

    def pairs(self, sel=None):
        return [(k["kf_id"], k["frame"]) for k in (self.cands if sel is None else [self.cands[i] for i in sel])]

    def close(self):
        self.dm.close()
        self.curr.close()
        for k in self.cands:
            k["frame"].close()


def reloc(w, opts, sel=None, between=None):
    ctx = w.ctx
    ctx.relocalize_async(w.dm, w.pairs(sel), w.curr, w.s["intr"], opts)
    if between:
        between()
    got = ctx.relocalize_fetch()
    got["lists"] = [dev_list(ctx, ctx.relocalize_matches(c)) for c in range(int(got["result"]["n_cand"]))]
    return got


def blob(g):
    return (g["result"].tobytes(), g["pool_cand"].tobytes(), g["pool_match"].tobytes(), g["pool_train"].tobytes(),
            g["mask"].tobytes()) + tuple(l.tobytes() for l in g["lists"])


def restate(w, opts, sel=None):
    """yardsticks (i) - (iii): what the record and the four arrays must be"""
    ctx, s = w.ctx, w.s
    cands = w.cands if sel is None else [w.cands[i] for i in sel]
    singles = []
    for k in cands:
        ctx.track_pnp_host_async(w.dm, k["kf_id"], k["desc"], w.desc_curr, w.curr_xy, s["intr"], opts)
        res, pm, _ = ctx.track_pnp_fetch()
        singles.append({"res": res, "pair_match": pm, "matches": ctx.match_fetch(), "n_good_matches": int(res["n_good_matches"])})
    pool = reloc_ref.pool_ref(singles, int(opts["min_matches"]))
    q = np.array([singles[c]["matches"]["query_idx"][m] for c, m in zip(pool["pool_cand"], pool["pool_match"])], np.int64)
    obj = s["lm_pos"][q].astype(np.float32).reshape(-1, 3)
    img = w.curr_xy[pool["pool_train"]].reshape(-1, 2)
    ran = any(pool["open"]) and pool["n_pool"] >= int(opts["min_inliers"])
    pnp, mask = np.zeros((), vxslam.PNP_RESULT_DTYPE), np.zeros(pool["n_pool"], np.uint8)
    if ran:
        po = np.array(opts["pnp"], vxslam.PNP_OPTIONS_DTYPE)
        po["max_iterations"] = reloc_ref.max_iterations_ref(pool["n_pool"], int(po["max_iterations"]))
        pnp, mask = ctx.pnp_ransac(obj, img, s["intr"], po)
    finite = bool(np.isfinite(pnp["pose"]).all())
    rec = reloc_ref.record_ref(pool, [float(x["res"]["parallax"]) for x in singles], int(pnp["ok"]), int(pnp["n_inliers"]),
                               finite, mask, int(opts["min_inliers"]))
    assert rec["ran"] == ran
    return {"singles": singles, "pool": pool, "pnp": pnp, "mask": mask, "rec": rec}


def same(got, want, what=""):
    r, pool, rec = got["result"], want["pool"], want["rec"]
    print(what, "status", r["status"], "n_cand", r["n_cand"], "n_pool", r["n_pool"], "concat", pool["n_concat"], "best",
          r["best_cand"], "inliers", r["pnp"]["n_inliers"], "kept", list(r["cand"]["n_kept"][:r["n_cand"]]),
          "inl", list(r["cand"]["n_inliers"][:r["n_cand"]]))
    n = len(want["singles"])
    assert r["n_cand"] == n
    for c, x in enumerate(want["singles"]):   # (i)
        e, t = r["cand"][c], x["res"]
        for f in ("n_matches", "n_good_matches", "n_pairs", "n_bad_index", "min_distance", "parallax"):
            assert e[f].tobytes() == t[f].tobytes(), (c, f, e[f], t[f])
        assert e["open"] == int(pool["open"][c]) and e["n_kept"] == pool["n_kept"][c] and e["n_inliers"] == rec["n_inliers"][c], c
        assert got["lists"][c].tobytes() == x["matches"].tobytes(), c
    assert r["cand"][n:].tobytes() == bytes(40 * (16 - n))
    assert r["n_pool"] == pool["n_pool"]      # (ii)
    for f in ("pool_cand", "pool_match", "pool_train"):
        assert got[f].dtype == pool[f].dtype and np.array_equal(got[f], pool[f]), f
    assert r["pnp"].tobytes() == want["pnp"].tobytes()   # (iii)
    assert np.array_equal(got["mask"], want["mask"])
    assert r["status"] == rec["status"] and r["best_cand"] == rec["best_cand"]
    assert np.float64(r["parallax"]).tobytes() == np.float64(rec["parallax"]).tobytes()


def run(w, opts, what="", sel=None):
    want = restate(w, opts, sel)
    got = reloc(w, opts, sel)
    same(got, want, what)
    return got, want


@pytest.fixture(scope="module")
def opts():
    return vxslam.track_options()


def claims(want):
    """train index -> [(candidate, pair index, distance)] over the open candidates' pair lists"""
    out = {}
    for c, x in enumerate(want["singles"]):
        if want["pool"]["open"][c]:
            for k, mi in enumerate(x["pair_match"]):
                m = x["matches"][mi]
                out.setdefault(int(m["train_idx"]), []).append((c, k, float(m["distance"])))
    return out


# ---------------------------------------------------------------------------- 1, 2 and 16 candidates
def test_one_candidate_is_track_pnp(ctx, opts):
    w = World(ctx, 61, [{}])
    got, want = run(w, opts, "one")
    x = want["singles"][0]
    assert len(np.unique(x["matches"]["train_idx"][x["pair_match"]])) == x["res"]["n_pairs"] == N   # premise: no repeats
    ctx.track_pnp_host_async(w.dm, KF0, w.cands[0]["desc"], w.desc_curr, w.curr_xy, w.s["intr"], opts)
    res, pm, mask = ctx.track_pnp_fetch()
    r = got["result"]
    assert res["status"] == OK and r["status"] == OK and r["best_cand"] == 0
    assert r["pnp"].tobytes() == res["pnp"].tobytes() and np.array_equal(got["mask"], mask)
    assert np.array_equal(got["pool_match"], pm) and not got["pool_cand"].any()
    assert np.float64(r["parallax"]).tobytes() == np.float64(res["parallax"]).tobytes()
    assert np.abs(r["pnp"]["pose"] - w.s["pose"]).max() < 5e-3
    w.close()


def test_two_and_sixteen_candidates(ctx, opts):
    rng = np.random.default_rng(7)
    cands = []
    for c in range(16):  # every candidate sees its own two thirds of the landmarks at its own distances
        cands.append({"flips": rng.integers(0, 25, N), "flags": (rng.random(N) < 0.66).astype(np.uint8)})
    w = World(ctx, 62, cands)
    for sel in ([0, 1], list(range(16))):
        got, want = run(w, opts, "n=%d" % len(sel), sel)
        assert got["result"]["status"] == OK and all(want["pool"]["open"])
        assert got["result"]["n_pool"] > max(x["res"]["n_pairs"] for x in want["singles"])  # the pool beats every candidate
        assert np.abs(got["result"]["pnp"]["pose"] - w.s["pose"]).max() < 5e-3
    for n in (0, 17):
        with pytest.raises(vxslam.VxError) as e:
            ctx.relocalize_async(w.dm, (w.pairs() + w.pairs())[:n], w.curr, w.s["intr"], opts)
        assert e.value.code == vxslam.VX_ERR_INVALID
    w.close()


# ---------------------------------------------------------------------------- the three tie rules
def test_equal_distance_goes_to_the_lower_candidate(ctx, opts):
    s_flips = synth.make_track_frame_scene(63, N)["flips"]
    w = World(ctx, 63, [{"flips": s_flips}, {"flips": s_flips}])   # different bits, equal counts
    got, want = run(w, opts, "tie-cand")
    ties = [t for t, cl in claims(want).items() if len({c for c, _, _ in cl}) == 2 and len({d for _, _, d in cl}) == 1]
    assert len(ties) > 100                                        # premise
    assert not got["pool_cand"].any() and got["result"]["cand"]["n_kept"][1] == 0
    w.close()


def test_smaller_distance_in_a_later_candidate_wins(ctx, opts):
    f0 = np.full(N, 12)
    f1 = np.where(np.arange(N) % 2 == 0, 5, 20)                   # even features: the later candidate is nearer
    w = World(ctx, 64, [{"flips": f0}, {"flips": f1}])
    got, want = run(w, opts, "later-wins")
    cl = claims(want)
    later = [t for t, v in cl.items() if len(v) == 2 and dict((c, d) for c, _, d in v)[1] < dict((c, d) for c, _, d in v)[0]]
    assert len(later) > 100                                       # premise
    won = dict(zip(got["pool_train"].tolist(), got["pool_cand"].tolist()))
    assert all(won[t] == 1 for t in later) and 0 < got["pool_cand"].sum() < len(got["pool_cand"])
    w.close()


def test_same_feature_twice_in_one_candidate_goes_to_the_lower_pair(ctx, opts):
    s = synth.make_track_frame_scene(65, N)
    train_of = s["train_of"].copy()
    train_of[1::2] = train_of[0::2]                               # features 2j and 2j + 1 both look like keypoint train_of[2j]
    w = World(ctx, 65, [{"flips": np.full(N, 9), "train_of": train_of}])
    got, want = run(w, opts, "twice")
    twice = [t for t, v in claims(want).items() if len(v) == 2 and v[0][2] == v[1][2]]
    assert len(twice) > 100                                       # premise
    x = want["singles"][0]
    first = {}
    for k, mi in enumerate(x["pair_match"]):
        first.setdefault(int(x["matches"]["train_idx"][mi]), int(mi))
    assert all(first[int(t)] == int(m) for t, m in zip(got["pool_train"], got["pool_match"]))
    assert got["result"]["n_pool"] < x["res"]["n_pairs"]
    w.close()


# ---------------------------------------------------------------------------- closed candidates
def test_closed_candidates_first_middle_last(ctx, opts):
    rng = np.random.default_rng(8)
    o = lambda: {"flips": rng.integers(0, 25, N), "flags": (rng.random(N) < 0.7).astype(np.uint8)}
    w = World(ctx, 66, [CLOSED, o(), CLOSED, o(), CLOSED])
    got, want = run(w, opts, "closed")
    assert want["pool"]["open"] == [False, True, False, True, False]   # premise
    assert set(got["pool_cand"].tolist()) == {1, 3} and got["result"]["status"] == OK and got["result"]["best_cand"] in (1, 3)
    w.close()


def test_all_candidates_closed(ctx, opts):
    w = World(ctx, 67, [CLOSED, CLOSED, CLOSED])
    got, want = run(w, opts, "all-closed")
    r = got["result"]
    assert not any(want["pool"]["open"])                           # premise
    assert r["status"] == FEW_MATCHES and r["n_pool"] == 0 and r["best_cand"] == -1 and r["parallax"] == 0.0
    assert r["pnp"].tobytes() == bytes(144) and len(got["mask"]) == 0
    w.close()


# ---------------------------------------------------------------------------- the gate on the pool
def test_pool_at_min_inliers_and_one_below(ctx):
    flags = np.zeros(N, np.uint8)
    flags[:40] = 1
    w = World(ctx, 68, [{"flags": flags}, {"flags": np.roll(flags, 20)}], wrong_frac=0.0)
    n_pool = restate(w, vxslam.track_options())["pool"]["n_pool"]
    assert n_pool == 60                                            # premise
    got, _ = run(w, vxslam.track_options(min_inliers=n_pool), "at")
    assert got["result"]["status"] in (OK, vxslam.TRACK_PNP_FAILED) and got["result"]["pnp"]["hypotheses_run"] > 0
    got, _ = run(w, vxslam.track_options(min_inliers=n_pool + 1), "below")
    assert got["result"]["status"] == FEW_PAIRS and got["result"]["pnp"].tobytes() == bytes(144) and not got["mask"].any()
    w.close()


# ---------------------------------------------------------------------------- the compaction chunk
@pytest.mark.parametrize("extra", [0, 1])
def test_concatenation_at_the_chunk_and_one_above(ctx, opts, extra):
    block = vxslam.lib().vx_track_block()
    assert block == 1024
    rng = np.random.default_rng(9)
    last = np.zeros(N, np.uint8)
    last[rng.permutation(N)[:block + extra - 3 * N]] = 1
    cands = [{"flips": rng.integers(0, 25, N)} for _ in range(3)] + [{"flips": rng.integers(0, 25, N), "flags": last}]
    w = World(ctx, 69, cands)
    got, want = run(w, opts, "chunk+%d" % extra)
    assert want["pool"]["n_concat"] == block + extra               # premise
    assert got["result"]["n_pool"] == N and got["result"]["status"] == OK
    w.close()


# ---------------------------------------------------------------------------- best_cand
def test_best_candidate_tie_goes_to_the_lower_index(ctx, opts):
    a = np.zeros(N, np.uint8)
    a[:N // 2] = 1
    w = World(ctx, 70, [{"flags": np.zeros(N, np.uint8)}, {"flags": a}, {"flags": 1 - a}], wrong_frac=0.0, noise_px=0.02)
    got, want = run(w, opts, "best-tie")
    inl = want["rec"]["n_inliers"]
    assert inl[0] == 0 and inl[1] == inl[2] == N // 2              # premise
    assert got["result"]["best_cand"] == 1
    w.close()


# ---------------------------------------------------------------------------- the LDS table's limit
def test_table_limit_and_one_row_above(ctx, opts):
    limit = ctx.relocalize_table_limit()
    assert limit >= 4096
    w = World(ctx, 71, [{}, {"flips": np.full(N, 3)}], curr_cap=limit, extra_rows=limit - N)   # a full table
    got, want = run(w, opts, "limit")
    assert got["result"]["status"] == OK and len(w.curr_xy) == limit
    before = blob(got)
    big = vxslam.Frame(ctx, limit + 1).upload(ctx, w.curr_xy, w.desc_curr)
    with pytest.raises(vxslam.VxError) as e:
        ctx.relocalize_async(w.dm, w.pairs(), big, w.s["intr"], opts)
    assert e.value.code == vxslam.VX_ERR_CAPACITY
    g2 = ctx.relocalize_fetch()                                    # the refused call left the previous result in place
    assert g2["result"].tobytes() == got["result"].tobytes() and before[4] == g2["mask"].tobytes()
    big.close()
    w.close()


# ---------------------------------------------------------------------------- repeats, interference
def test_repeats_and_interference(ctx, opts):
    rng = np.random.default_rng(10)
    w = World(ctx, 72, [{"flips": rng.integers(0, 25, N), "flags": (rng.random(N) < 0.6).astype(np.uint8)} for _ in range(4)])
    got, _ = run(w, opts, "clean")
    clean = blob(got)
    for _ in range(3):
        assert blob(reloc(w, opts)) == clean
    # other calls between the enqueue and the fetch, and the call between theirs
    s = w.s
    last = vxslam.Frame(ctx, N + 20).upload(ctx, s["last_xy"], s["desc_last"])
    fo = vxslam.track_frame_options(ess={"max_iterations": 200})
    k0, k1 = w.cands[0], w.cands[1]
    rig_cams = [vxslam.rig_camera(w.curr, s["intr"], last_kf_id=k["kf_id"], last_kf=k["frame"], last=last, pose_last=s["pose_last"])
                for k in (k0, k1)]

    def rig_blob(r):
        return tuple(x["result"].tobytes() + x["pnp"][0].tobytes() + x["pnp"][1].tobytes() + x["ess"][0].tobytes() +
                     x["ess"][1].tobytes() for x in r)

    def frame_blob(x):
        return x["result"].tobytes() + x["pnp"][0].tobytes() + x["pnp"][1].tobytes()

    def frame_async():
        ctx.track_frame_async(w.dm, k1["kf_id"], k1["frame"], last, w.curr, s["intr"], fo, pose_last=s["pose_last"])

    ctx.track_rig_async(w.dm, rig_cams, fo)
    rig_clean = rig_blob(ctx.track_rig_fetch())
    frame_async()
    frame_clean = frame_blob(ctx.track_frame_fetch())
    seen = {}

    def others():
        ctx.track_rig_async(w.dm, rig_cams, fo)
        seen["rig"] = rig_blob(ctx.track_rig_fetch())
        frame_async()
        seen["frame"] = frame_blob(ctx.track_frame_fetch())
        ctx.pnp_ransac(s["lm_pos"].astype(np.float32), s["curr_xy"][s["train_of"]], s["intr"], vxslam.pnp_options(N))

    assert blob(reloc(w, opts, between=others)) == clean
    assert seen == {"rig": rig_clean, "frame": frame_clean}
    ctx.track_rig_async(w.dm, rig_cams, fo)
    frame_async()
    assert blob(reloc(w, opts)) == clean
    assert frame_blob(ctx.track_frame_fetch()) == frame_clean and rig_blob(ctx.track_rig_fetch()) == rig_clean
    last.close()
    w.close()


# ---------------------------------------------------------------------------- the best candidate's list feeds CreateKeyFrame
def test_create_keyframe_on_the_best_candidates_list(ctx, opts):
    rng = np.random.default_rng(11)
    cands = [{"flips": rng.integers(0, 25, N), "flags": (rng.random(N) < p).astype(np.uint8)} for p in (0.3, 0.8, 0.5)]
    worlds = [World(ctx, 73, cands) for _ in range(2)]
    got = reloc(worlds[0], opts)
    best = int(got["result"]["best_cand"])
    assert got["result"]["status"] == OK and best == 1
    pose = got["result"]["pnp"]["pose"]
    out = []
    for i, w in enumerate(worlds):
        if i == 0:
            m = ctx.relocalize_matches(best)
        else:  # the list a caller has today: Track() against the best keyframe alone
            ctx.track_frame_async(w.dm, KF0 + best, w.cands[best]["frame"], None, w.curr, w.s["intr"],
                                  vxslam.track_frame_options())
            ctx.track_frame_fetch()
            m = ctx.track_frame_matches(0)
        assert dev_list(ctx, m).tobytes() == got["lists"][best].tobytes()
        out.append(w.dm.create_keyframe_frame(900, pose, w.s["intr"], w.curr, last_kf_id=KF0 + best, matches=m,
                                              first_landmark_id=7000000, ctx=ctx))
    assert out[0]["result"].tobytes() == out[1]["result"].tobytes()
    assert out[0]["landmarks"].tobytes() == out[1]["landmarks"].tobytes()
    assert worlds[0].dm.counts() == worlds[1].dm.counts() and worlds[0].dm.counts()["kf"] == 4
    for x, y in zip(worlds[0].dm.download(), worlds[1].dm.download()):
        assert np.array_equal(x, y)
    for w in worlds:
        w.close()


# ---------------------------------------------------------------------------- argument and state checks
def test_argument_and_state_checks(ctx, opts):
    L = vxslam.lib()
    fresh = vxslam.Context(0)
    out = np.zeros(1, vxslam.RELOC_RESULT_DTYPE)
    po = C.c_void_p(out.ctypes.data)
    assert L.vx_relocalize_fetch(fresh.handle, po, None, None, None, None, 0) == vxslam.VX_ERR_STATE   # fetch before enqueue
    assert L.vx_relocalize_matches(fresh.handle, 0, None, None, None) == vxslam.VX_ERR_STATE
    fresh.close()
    w = World(ctx, 74, [{}, {"flips": np.full(N, 4)}, {}])
    got = reloc(w, opts, [0, 1])
    clean = blob(got)

    def refused(dm, cands, curr, intr, code=vxslam.VX_ERR_INVALID):
        with pytest.raises(vxslam.VxError) as e:
            ctx.relocalize_async(dm, cands, curr, intr, opts)
        assert e.value.code == code

    p = w.pairs()
    intr = w.s["intr"]
    refused(w.dm, [p[0], p[0]], w.curr, intr)                      # a keyframe named twice
    refused(w.dm, [p[0], (KF0 + 77, p[1][1])], w.curr, intr)       # a keyframe that is not in the map
    refused(w.dm, [p[0], (p[1][0], None)], w.curr, intr)           # a candidate without a frame
    refused(None, p, w.curr, intr)                                 # no map
    refused(w.dm, p, None, intr)                                   # no current frame
    refused(w.dm, p, w.curr, [0.0, 500.0, 1.0, 1.0])               # zero focal length
    assert L.vx_relocalize_async(ctx.handle, w.dm.handle, 1, None, w.curr.handle, C.c_float(0.8), None, None) == vxslam.VX_ERR_INVALID
    w.dm.remove_keyframe(KF0 + 2)
    refused(w.dm, p, w.curr, intr)                                 # a dead keyframe
    # a refused enqueue leaves the previous call's result in place
    g = ctx.relocalize_fetch()
    g["lists"] = [dev_list(ctx, ctx.relocalize_matches(c)) for c in range(2)]
    assert blob(g) == clean
    for c in (-1, 2):
        assert L.vx_relocalize_matches(ctx.handle, c, None, None, None) == vxslam.VX_ERR_INVALID
    small = np.zeros(4, np.int32)
    assert L.vx_relocalize_fetch(ctx.handle, po, None, C.c_void_p(small.ctypes.data), None, None, 4) == vxslam.VX_ERR_CAPACITY
    assert out[0].tobytes() == got["result"].tobytes()             # ... with *out filled
    assert L.vx_relocalize_fetch(ctx.handle, po, None, None, None, None, 0) == vxslam.VX_OK
    w.close()


# ---------------------------------------------------------------------------- it is really one sequence
NEW_STAGES = ("reloc_pairs", "reloc_pool", "reloc_final")


def test_launch_counts_do_not_depend_on_the_candidates(ctx, opts):
    rng = np.random.default_rng(12)
    w = World(ctx, 75, [{"flips": rng.integers(0, 25, N)} for _ in range(16)])
    counts = {}
    for n in (2, 16):
        sel = list(range(n))
        reloc(w, opts, sel)
        ctx.prof_enable(True)
        reloc(w, opts, sel)
        prof = ctx.prof_read()
        ctx.prof_enable(False)
        counts[n] = {k: v[1] for k, v in prof.items() if v[1]}
    print(counts)
    assert counts[2] == counts[16]
    assert all(counts[2][s] == 1 for s in NEW_STAGES + ("pnp_hypotheses", "pnp_refine"))
    assert "track_pairs" not in counts[2] and "rig_pairs" not in counts[2]
    w.close()
