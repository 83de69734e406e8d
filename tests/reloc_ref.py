"""numpy restatement of vx_relocalize_async's pool and record rules (include/vx_slam.h, csrc/reloc.hip): what
happens between the per-candidate pair lists (TrackWithPnP's own, tests/track_ref.py) and the one
solvePnPRansac call, and what the record says afterwards.  Plain sequential loops; pinned on hand-written lists
by tests/test_reloc_cpu.py.

A candidate is a dict with `matches` (records with query_idx / train_idx / distance: Match(kf_c, curr)),
`pair_match` (indices into matches of its pairs, in pair order) and `n_good_matches`."""
import numpy as np

OK, FEW_MATCHES, FEW_PAIRS, PNP_FAILED, BAD_ROTATION = range(5)


def pool_ref(cands, min_matches=50):
    """The pool: the open candidates' pairs concatenated candidate-major in pair order; of all pairs that name
    one current feature (train_idx) exactly one survives: the smallest match distance, then the lower candidate,
    then the lower pair index.  The survivors keep the concatenation order.

    Returns a dict: open (list of bool), n_concat, pool_cand (uint8), pool_match, pool_train (int32), n_pool,
    n_kept (per candidate)."""
    is_open = [int(c["n_good_matches"]) >= min_matches for c in cands]
    concat = []  # (candidate, pair index, match index, train index, distance)
    for ci, c in enumerate(cands):
        if not is_open[ci]:
            continue
        for k, mi in enumerate(np.asarray(c["pair_match"], np.int64)):
            m = c["matches"][int(mi)]
            concat.append((ci, k, int(mi), int(m["train_idx"]), np.float32(m["distance"])))
    winner = {}  # train index -> (distance, candidate, pair index), the smallest in that order
    for ci, k, _, t, d in concat:
        key = (d, ci, k)
        if t not in winner or key < winner[t]:
            winner[t] = key
    kept = [(ci, mi, t) for ci, k, mi, t, d in concat if winner[t] == (d, ci, k)]
    pool_cand = np.array([x[0] for x in kept], np.uint8)
    return {"open": is_open, "n_concat": len(concat), "pool_cand": pool_cand,
            "pool_match": np.array([x[1] for x in kept], np.int32), "pool_train": np.array([x[2] for x in kept], np.int32),
            "n_pool": len(kept), "n_kept": [int((pool_cand == ci).sum()) for ci in range(len(cands))]}


def max_iterations_ref(n_pool, max_iterations=-1):
    """solvePnPRansac's budget on the pool (tracking.cpp:421)"""
    return min(100, 2 * n_pool) if max_iterations < 0 else max_iterations


def record_ref(pool, parallax, pnp_ok, pnp_n_inliers, pose_finite, mask, min_inliers=30):
    """The record's head after PnP on the pool: status by TrackWithPnP's gates in the order of its return
    statements (:357 no candidate open, :402 on n_pool, :425, :441), n_inliers per candidate, best_cand (most
    inliers, ties to the lower index; -1 unless OK) and its parallax (0 unless OK).  `mask`: the pooled inlier
    mask (ignored when PnP did not run); `parallax`: per candidate."""
    n_cand = len(pool["open"])
    ran = any(pool["open"]) and pool["n_pool"] >= min_inliers
    if not any(pool["open"]):
        status = FEW_MATCHES
    elif pool["n_pool"] < min_inliers:
        status = FEW_PAIRS
    elif not pnp_ok or pnp_n_inliers < min_inliers:
        status = PNP_FAILED
    elif not pose_finite:
        status = BAD_ROTATION
    else:
        status = OK
    mask = np.asarray(mask, np.uint8) if ran else np.zeros(pool["n_pool"], np.uint8)
    n_inl = [int(((pool["pool_cand"] == ci) & (mask != 0)).sum()) for ci in range(n_cand)]
    best = -1
    if status == OK:
        best = 0
        for ci in range(1, n_cand):
            if n_inl[ci] > n_inl[best]:
                best = ci
    return {"status": status, "ran": ran, "n_inliers": n_inl, "best_cand": best,
            "parallax": float(parallax[best]) if best >= 0 else 0.0}
