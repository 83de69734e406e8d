"""The cases of tests/ransac_cases.py are what they claim, on the CPU: every committed case realises its
situation (classifier over the reference count stream), the oracle's loop equals the plain Python loop
on it, the straddle cases tell the old block loop (csrc/essential.hip's, before the fix) from the fixed
one (now replay() of csrc/ransac_common.hpp), and the
budget-formula sweep has the margin and the share of usable cases that tests/test_gpu_ransac_replay.py
relies on (RANSACUpdateNumIters against mpmath at 50 digits)."""
import numpy as np
import pytest

import ransac_cases as rc

RESEED = "reseed this case: commit the tuple ransac_cases.reseed(oracle, kind, tag) returns"


def _pnp_ref(oracle, case, extra=1):
    d = rc.build(case)
    return d, rc.pnp_stream(oracle, d, case[2], case[4] + extra)


def _ess_ref(oracle, case, extra=1):
    d = rc.build(case)
    return d, rc.ess_stream(oracle, d, case[2], case[4] + extra)


def test_sample4_is_the_oracles(oracle):
    """the 4-sample form: the hypotheses whose first three draws are collinear world points are the ones
    the oracle has no model for"""
    case = rc.PNP_CASES["invalid_mix"]
    d, counts = _pnp_ref(oracle, case)
    n, n_line = len(d["obj"]), case[1][2]
    collinear = {h for h in range(case[4]) if all(i < n_line for i in rc.sample4(case[2], h, n)[:3])}
    invalid = {h for h in range(case[4]) if counts[h] is None}
    assert collinear and collinear <= invalid
    assert rc.sample5(7, 3, 40)[:4] == rc.sample4(7, 3, 40)  # one counter stream for both sizes


@pytest.mark.parametrize("tag", sorted(rc.PNP_CASES))
def test_pnp_case(oracle, tag):
    case = rc.PNP_CASES[tag]
    d, counts = _pnp_ref(oracle, case)
    n, cf, H = len(d["obj"]), case[3], case[4]
    assert tag in rc.classify_pnp(counts, n, cf, H), RESEED
    best, run, good, _ = rc.pnp_loop(counts, n, cf, H)
    o = oracle.pnp_options(n, max_iterations=H, confidence=cf, seed=case[2])
    r, mask = oracle.pnp_ransac(d["obj"], d["img"], d["intr"], o)
    assert (r["best_hypothesis"], r["hypotheses_run"], r["n_inliers"], r["ok"]) == (best, run, good, int(best >= 0))
    assert mask.sum() == good


def test_pnp_cases_cover_every_situation():
    assert set(rc.PNP_CASES) == set(rc.PNP_TAGS)
    assert set(rc.ESS_CASES) | {"straddle"} == set(rc.ESS_TAGS)
    assert len(rc.STRADDLE_CASES) >= 3


@pytest.mark.parametrize("kind,tag", [("pnp", "n4"), ("pnp", "all_low"), ("pnp", "last_other_max"), ("ess", "n5"),
                                      ("ess", "gate129"), ("ess", "lane63")])
def test_reseed_finds_the_committed_case(oracle, kind, tag):
    assert rc.reseed(oracle, kind, tag) == (rc.PNP_CASES if kind == "pnp" else rc.ESS_CASES)[tag]


def _check_ess(oracle, case, tag):
    d, rows = _ess_ref(oracle, case)
    n, cf, H = len(d["pts_last"]), case[3], case[4]
    assert tag in rc.classify_ess(rows, n, cf, H), RESEED
    best, run, good, _ = rc.ess_loop(rows, n, cf, H)
    o = oracle.essential_options(max_iterations=H, confidence=cf, seed=case[2])
    r, _ = oracle.essential_ransac(d["pts_last"], d["pts_curr"], d["intr"], o)
    hm = (-1, -1) if best is None else best
    assert (r["best_hypothesis"], r["best_model"], r["hypotheses_run"], r["n_ransac_inliers"]) == hm + (run, good)
    # the fixed block loop is the sequential loop, within H * 10 / 64 rounds; so is its gate form
    new = rc.ess_block_loop(rows, n, cf, H, True)
    assert new[:4] == hm + (run, good)
    assert new[4] <= (H * rc.K_MODELS + rc.BLOCK - 1) // rc.BLOCK
    if H > rc.FIRST_CHUNK:
        gate = rc.ess_block_loop(rows, n, cf, H, True, rc.FIRST_CHUNK)[5]
        assert (gate if gate > rc.FIRST_CHUNK else 0) == rc.gate_value(rows, n, cf, H)
        assert run <= rc.FIRST_CHUNK or rc.gate_value(rows, n, cf, H) >= run
    return rows, n, hm + (run, good)


@pytest.mark.parametrize("tag", sorted(rc.ESS_CASES))
def test_ess_case(oracle, tag):
    _check_ess(oracle, rc.ESS_CASES[tag], tag)


@pytest.mark.parametrize("k", range(len(rc.STRADDLE_CASES)))
def test_straddle_case_tells_the_loops_apart(oracle, k):
    """the old block loop ends before the block that holds the straddled hypothesis's remaining models
    and keeps an earlier, worse model; the fixed one agrees with the sequential loop"""
    case = rc.STRADDLE_CASES[k]
    rows, n, ref = _check_ess(oracle, case, "straddle")
    old = rc.ess_block_loop(rows, n, case[3], case[4], False)
    assert old[:4] != ref, RESEED
    assert old[0] == ref[0] and old[1] < ref[1] and old[3] < ref[3]


@pytest.mark.parametrize("tag", sorted(rc.ESS_CASES))
def test_old_loop_only_differs_on_straddles(oracle, tag):
    """the other situations never depended on the lost models: both block loops agree there"""
    case = rc.ESS_CASES[tag]
    d, rows = _ess_ref(oracle, case)
    n = len(d["pts_last"])
    assert rc.ess_block_loop(rows, n, case[3], case[4], False)[:4] == rc.ess_block_loop(rows, n, case[3], case[4], True)[:4]


# ------------------------------------------------------------------------------------- budget formula
@pytest.mark.parametrize("points", [4, 5])
def test_budget_formula_sweep(oracle, points):
    """Margin: every swept quotient is >= 1e-9 from a half-integer and from the clamp comparison, so
    the expected integer does not depend on the last bits of any log; the formula on the exact
    rational inlier ratio gives the same integers; the double formulas (Python's, and for four points
    the oracle's) equal mpmath over the whole sweep.  Share skipped: at most 10 % of the cases end at
    the kept hypothesis instead of at the formula's value."""
    H = rc.SWEEP_H[points]
    rows = rc.sweep(points)
    assert len(rows) > 5000
    assert {r[0] for r in rows} == set(rc.SWEEP_N) and {r[2] for r in rows} == set(rc.SWEEP_CONFIDENCE)
    assert min(r[4] for r in rows) >= rc.MARGIN
    assert any(r[3] == H for r in rows) and any(r[3] == 0 for r in rows)
    for n, k, cf, e, _ in rows:
        assert rc.update_iters_exact(cf, n, k, H, points) == e, (n, k, cf)
        assert rc.update_iters(cf, (n - k) / n, H, points) == e, (n, k, cf)
        if points == 4:
            assert oracle.pnp_update_iters(cf, (n - k) / n, H) == e, (n, k, cf)
    ref = rc.sweep_reference(oracle, points)
    total = skipped = 0
    for batch, _, out, _, expected in ref:
        assert len(batch) * H * rc.SWEEP_RECORD_BYTES[points] <= rc.SWEEP_CALL_BYTES
        for r, o, e in zip(batch, out, expected):
            total += 1
            if e is None:
                skipped += 1
            else:
                assert o["hypotheses_run"] == e, (r, o)
    print("sweep, %d points: %d cases in %d calls, %d skipped (%.1f %%)" % (points, total, len(ref), skipped,
                                                                           100.0 * skipped / total))
    assert total == len(rows) and skipped <= 0.10 * total
