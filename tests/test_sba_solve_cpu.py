"""The inputs of tests/test_gpu_sba_solve.py do what they claim — checked on the CPU restatement
(oracle.sba_system / oracle.sba_optimize), no GPU: the 6 x 6 block pattern of each case (long-range
blocks for the loop closures, the expected components for the splits), a tile-level symbolic
factorisation restated in numpy (tests/sba_ref.tile_pattern) that finds the fill tiles, positive
definiteness on the free rows, and the two bars of sba_ref.check_solution met with margin by
numpy.linalg.solve and by a plain FP64 Cholesky against the 80-bit reference.

Fill at tile granularity: the 14-keyframe loop closure the issue asks for (landmarks of keyframes 2, 3
seen again by keyframe 13) makes the long-range tile (4, 0) and a gap in column 0's panel list (tile
(3, 0) stays zero), but no fill tile — keyframe 13's tile row is already full in S, since those
landmarks' tracks reach keyframe 6 and its own band keyframe 9.  "e-loop14-short" (tracks ending at
keyframe 3) is the 5-tile case with a fill tile; the 26-keyframe cases fill 4 and 3 tiles."""
import numpy as np
import pytest

import sba_ref as R
from vxslam import synth

FILL_TILES = {"e-loop14": 0, "e-loop14-short": 1, "e-loop26": 4, "f-band-loop26": 3}


@pytest.fixture(scope="module")
def systems(oracle):
    out = {}
    for name in R.CASES:
        m, kw = R.case(name)
        S, rhs = oracle.sba_system(m, oracle.sba_options(iters=1, **kw))
        assert np.abs(S - S.T).max() <= 1e-12 * np.abs(S).max()
        out[name] = (m, kw, R.symmetrise(S), rhs)  # (as the GPU test does with vx_sba_plan_system's lower triangle)
    return out


def test_map_edits_keep_the_map_consistent():
    """close_loop / split_window edit only what they say: every other array equals a fresh make_ba_map
    (no generator draw moved), each landmark's observation list stays in keyframe order and each entry
    points at a feature of that keyframe that carries the landmark's id."""
    for name in R.LOOP_CASES + ("f-split-3-9",):
        nk, nl, edits, _ = R.CASES[name]
        m, _ = R.case(name)
        base = synth.make_ba_map(R.SEED, nk, nl, n_old_kf=0)
        for k in ("kf_id", "kf_pose", "kf_intr", "kf_has_cam", "kf_feat_ptr", "lm_id", "lm_pos"):
            assert np.array_equal(m[k], base[k]), (name, k)
        n_loop = sum(e[3] for e in edits if e[0] == "loop")
        assert len(m["obs_kf_id"]) == len(base["obs_kf_id"]) + n_loop == m["lm_obs_ptr"][-1]
        changed = np.nonzero(m["feat_flags"] != base["feat_flags"])[0]
        assert len(changed) == n_loop and (base["feat_flags"][changed] == 0).all()
        assert np.array_equal(np.delete(m["feat_uv"], changed, 0), np.delete(base["feat_uv"], changed, 0))
        row_of = {int(k): r for r, k in enumerate(m["kf_id"])}
        for l in range(len(m["lm_id"])):
            o0, o1 = int(m["lm_obs_ptr"][l]), int(m["lm_obs_ptr"][l + 1])
            ids = m["obs_kf_id"][o0:o1]
            assert (ids[1:] > ids[:-1]).all(), (name, l)
            for o in range(o0, o1):
                f = int(m["kf_feat_ptr"][row_of[int(m["obs_kf_id"][o])]]) + int(m["obs_feat_idx"][o])
                assert m["feat_lm_id"][f] == m["lm_id"][l] and m["feat_flags"][f] & 1
        if any(e[0] == "split" for e in edits):
            assert m["lm_bad"].sum() > base["lm_bad"].sum()
        else:
            assert np.array_equal(m["lm_bad"], base["lm_bad"])


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_pattern(systems, name):
    m, kw, S, rhs = systems[name]
    nk = kw["window"]
    free = R.free_keyframes(m, kw)
    B = R.block_pattern(S)
    comps = R.components(B, free)
    assert [len(c) for c in comps] == R.COMPONENTS[name]
    for r in range(nk):  # gauge rows: the identity, no rhs
        if r not in free:
            assert np.array_equal(S[6 * r:6 * r + 6], np.eye(6 * nk)[6 * r:6 * r + 6]) and not rhs[6 * r:6 * r + 6].any()
    far = [(i, j) for i in free for j in free if i - j > 4 and B[i, j]]
    loops = [e for e in R.CASES[name][2] if e[0] == "loop"]
    if loops:
        (_, src, dst, *_), = loops
        assert all(B[dst, s] for s in src) and all(i == dst for i, _ in far)
    else:
        assert not far  # the band: a landmark's keyframes are at most 5 consecutive ones
    for e in R.CASES[name][2]:
        if e[0] == "split":
            assert not B[e[1] + 1:, :e[1] + 1].any()
    if name == "h-isolated-kf5":
        d = S[30:36, 30:36]
        assert np.array_equal(d, 1e-6 * np.eye(6)) and not rhs[30:36].any()
    # tiles: the symbolic factorisation's fill
    fill = 0
    for c in comps:
        nzS, nzL = R.tile_pattern(B, c)
        assert nzS.shape[0] == max(1, -(-6 * len(c) // 16)) and not (nzS & ~nzL).any()
        fill += int((nzL & ~nzS).sum())
    assert fill == FILL_TILES.get(name, 0)
    if name in R.LOOP_CASES and name != "e-loop14":
        assert fill >= 1
    if name == "e-loop14":  # the long-range tile and the gap in column 0's panel list
        nzS, nzL = R.tile_pattern(B, comps[0])
        assert nzS[4, 0] and not nzL[3, 0]
    if name == "c-3tiles-nopad":
        assert 6 * len(comps[0]) == 48  # three tiles, no padding row
    if name == "b-2tiles":
        assert 6 * 2 < 16 < 6 * 3  # the third keyframe's block straddles the tile boundary


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_is_well_posed_and_bars_hold_on_cpu(systems, name):
    m, kw, S, rhs = systems[name]
    free = R.free_keyframes(m, kw)
    comps = R.components(R.block_pattern(S), free)
    idx = np.concatenate([np.arange(6 * r, 6 * r + 6) for r in free])
    assert np.linalg.eigvalsh(S[np.ix_(idx, idx)]).min() > 0
    for solve in (np.linalg.solve, R.solve_chol64):
        x = np.zeros_like(rhs)
        for c in comps:
            ci = np.concatenate([np.arange(6 * r, 6 * r + 6) for r in c])
            x[ci] = solve(S[np.ix_(ci, ci)], rhs[ci])
        for rec in R.check_solution(S, rhs, x, comps, f"{name}/{solve.__name__}"):
            assert rec["bwd"] <= rec["cap"] / 16  # margin to spare
            assert rec["ratio"] is None or rec["ratio"] <= R.FWD_FACTOR / 4
    # the reference's own residual is below FP64's resolution of the problem
    for c in comps:
        ci = np.concatenate([np.arange(6 * r, 6 * r + 6) for r in c])
        A, b = S[np.ix_(ci, ci)], rhs[ci]
        x_ext = R.solve_ext(A, b)
        res = np.abs(np.array(A, np.longdouble) @ x_ext - b).max()
        assert res <= 2.0 ** -60 * (np.abs(A).sum(axis=1).max() * np.abs(x_ext).max() + np.abs(b).max())


@pytest.mark.parametrize("name", ["e-loop14", "e-loop26"])
def test_loop_map_converges(oracle, name):
    m, kw = R.case(name)
    st = oracle.sba_optimize(m, oracle.sba_options(iters=8, **kw))
    assert st.status == 0 and st.accepted >= 2
    assert st.final_cost < 0.2 * st.initial_cost
