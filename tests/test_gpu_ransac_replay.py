"""GPU parity of the two RANSAC loop replays (replay() of csrc/ransac_common.hpp with one model per
hypothesis in k_pnp_refine, with ten in k_em_gate / k_em_pick) in every situation tests/ransac_cases.py commits a case
for, of the essential gate (a case alone = one k_em_hyp launch, the same case in a padded batch = two,
byte-equal), of RANSACUpdateNumIters with the device log / rint against mpmath at 50 digits, and of
runs that follow a longer one through the same context (records beyond a problem's budget are stale).

Bars: PnP as tests/test_gpu_ransac.py (decisions and mask identical, refit within 1e-9); essential
records and masks byte for byte the oracle's.  The cases were chosen on the CPU (oracle + numpy) and are
pinned to their situations by tests/test_ransac_replay_cpu.py."""
import numpy as np
import pytest
import torch

import ransac_cases as rc
import vxslam

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-9


def _pnp_same(rg, mg, rc_, mc):
    for k in ("ok", "best_hypothesis", "hypotheses_run", "n_inliers"):
        assert rg[k] == rc_[k], (k, rg[k], rc_[k])
    assert np.array_equal(mg, mc)
    if rc_["ok"]:
        assert np.abs(rg["pose"] - rc_["pose"]).max() <= POSE_TOL, (rg["pose"], rc_["pose"])
        assert np.abs(rg["rvec"] - rc_["rvec"]).max() <= POSE_TOL
        assert abs(rg["cost0"] - rc_["cost0"]) <= 1e-9 * max(rc_["cost0"], 1.0)
        assert abs(rg["cost"] - rc_["cost"]) <= 1e-9 * max(rc_["cost"], 1.0)


def _ess_same(rg, mg, rc_, mc):
    assert rg.tobytes() == rc_.tobytes(), (rg, rc_)
    assert np.array_equal(mg, mc)


def _pnp_opt(case, n, H=None):
    return vxslam.pnp_options(n, max_iterations=case[4] if H is None else H, confidence=case[3], seed=case[2])


def _ess_opt(case, H=None):
    return vxslam.essential_options(max_iterations=case[4] if H is None else H, confidence=case[3], seed=case[2])


# --------------------------------------------------------------------------------------------- PnP
@pytest.mark.parametrize("tag", sorted(rc.PNP_CASES))
def test_pnp_replay_case(ctx, oracle, tag):
    case = rc.PNP_CASES[tag]
    d = rc.build(case)
    o = _pnp_opt(case, len(d["obj"]))
    rg, mg = ctx.pnp_ransac(d["obj"], d["img"], d["intr"], o)
    rc_, mc = oracle.pnp_ransac(d["obj"], d["img"], d["intr"], o)
    _pnp_same(rg, mg, rc_, mc)


def _pnp_batch():
    """every case in one call, small budgets (1, 2, 3, 63, 64, 65) beside 4096: hmax = 4096 is the
    record stride, and the records beyond a problem's own H are never written"""
    items = [(rc.PNP_CASES[t], None) for t in sorted(rc.PNP_CASES)]
    for H, t in zip((1, 4096, 2, 3, 4096, 63, 64, 65, 4096), sorted(rc.PNP_CASES)):
        items.append((rc.PNP_CASES[t], H))
    ps = [rc.build(c) for c, _ in items]
    offs = np.cumsum([0] + [len(p["obj"]) for p in ps])
    opts = np.stack([_pnp_opt(c, len(p["obj"]), H) for (c, H), p in zip(items, ps)])
    return (offs, np.concatenate([p["obj"] for p in ps]), np.concatenate([p["img"] for p in ps]),
            np.stack([p["intr"] for p in ps]), opts)


def test_pnp_replay_batch(ctx, oracle):
    args = _pnp_batch()
    offs = args[0]
    assert {1, 4096} <= set(args[4]["max_iterations"].tolist())
    og, mg = ctx.pnp_ransac_batch(*args)
    oc, mc = oracle.pnp_ransac_batch(*args)
    for k in range(len(offs) - 1):
        _pnp_same(og[k], mg[offs[k]:offs[k + 1]], oc[k], mc[offs[k]:offs[k + 1]])


# ----------------------------------------------------------------------------------------- essential
def _launches(ctx, call):
    """(result of call(), k_em_hyp launches it made)"""
    ctx.prof_enable(True, ["em_hypotheses"])
    ctx.prof_read()
    try:
        out = call()
        n = ctx.prof_read()["em_hypotheses"][1]
    finally:
        ctx.prof_enable(False)
    return out, n


def _gated_batch(d, o):
    """the problem followed by empty problems, enough of them and with enough max_iterations that
    P * hmax exceeds 8 x the CU count and hmax the first chunk: ess_enqueue launches k_em_hyp twice"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    hmax = max(int(o["max_iterations"]), rc.FIRST_CHUNK + 1)
    P = 8 * cus // hmax + 2
    opts = np.stack([o] * P)
    opts["max_iterations"][1:] = hmax
    n = len(d["pts_last"])
    offs = np.array([0] + [n] * P)
    assert P * hmax > 8 * cus
    return offs, d["pts_last"], d["pts_curr"], np.stack([d["intr"]] * P), opts


ESS_ALL = [(t, rc.ESS_CASES[t]) for t in sorted(rc.ESS_CASES)] + [("straddle%d" % k, c)
                                                                 for k, c in enumerate(rc.STRADDLE_CASES)]


@pytest.mark.parametrize("tag,case", ESS_ALL, ids=[t for t, _ in ESS_ALL])
def test_ess_replay_case_alone_and_gated(ctx, oracle, tag, case):
    d = rc.build(case)
    o = _ess_opt(case)
    (rg, mg), launches = _launches(ctx, lambda: ctx.essential_ransac(d["pts_last"], d["pts_curr"], d["intr"], o))
    assert launches == 1
    rc_, mc = oracle.essential_ransac(d["pts_last"], d["pts_curr"], d["intr"], o)
    _ess_same(rg, mg, rc_, mc)
    args = _gated_batch(d, o)
    (og, mb), launches = _launches(ctx, lambda: ctx.essential_ransac_batch(*args))
    assert launches == 2
    _ess_same(og[0], mb, rg, mg)
    assert not og["ok"][1:].any()


# ------------------------------------------------------------------------------------ budget formula
@pytest.mark.parametrize("points", [4, 5])
def test_budget_formula_sweep(ctx, oracle, points):
    """hypotheses_run of an exact problem is RANSACUpdateNumIters at the kept count (device log and
    rint): equal to mpmath at 50 digits over the whole sweep; the kept hypothesis and count equal the
    sequential reference's in every case, the skipped ones included"""
    call = ctx.pnp_ransac_batch if points == 4 else ctx.essential_ransac_batch
    checked = 0
    for rows, args, out, mask, expected in rc.sweep_reference(oracle, points):
        og, mg = call(*args)
        if points == 5:
            assert og.tobytes() == out.tobytes()
        for k in ("ok", "best_hypothesis", "n_inliers"):
            assert np.array_equal(og[k], out[k]), k
        assert np.array_equal(mg, mask)
        for r, g, e in zip(rows, og, expected):
            if e is not None:
                assert g["hypotheses_run"] == e, (r, g["hypotheses_run"], e)
                checked += 1
    assert checked >= 0.9 * len(rc.sweep(points))


# --------------------------------------------------------------------------------------- stale records
def _big_pnp():
    """64 matches of which 40 fit, H = 4096 and confidence 1: log(DBL_MIN) / log(1 - (40 / 64)^k) is beyond
    4096 for k = 4 and 5, so the clamp keeps the budget, all 4096 records are written (the gate stays
    open) and every all-inlier sample's record holds 40"""
    d = rc.exact_pnp(3, 64, range(40))
    return d, vxslam.pnp_options(64, max_iterations=4096, confidence=1.0, seed=9)


def _big_ess():
    d = rc.exact_two_view(3, 64, range(40))
    return d, vxslam.essential_options(max_iterations=4096, confidence=1.0, seed=9)


def _pnp_small_batch():
    """the lane-63 case (its loop stops early) beside a neighbour with H = 1"""
    a, b = rc.PNP_CASES["lane63"], rc.PNP_CASES["tie_block"]
    ps = [rc.build(a), rc.build(b)]
    offs = np.cumsum([0] + [len(p["obj"]) for p in ps])
    opts = np.stack([_pnp_opt(a, len(ps[0]["obj"])), _pnp_opt(b, len(ps[1]["obj"]), 1)])
    return (offs, np.concatenate([p["obj"] for p in ps]), np.concatenate([p["img"] for p in ps]),
            np.stack([p["intr"] for p in ps]), opts)


def _equal(a, b):
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("order", ["big_first", "small_first"])
def test_stale_records(order):
    """A context that has held 4096 high-count records per problem gives, bit for bit, what a fresh one
    gives on problems whose loops stop early (a gated essential batch with gate 0 and with a small
    gate, a PnP batch with an H = 1 neighbour) — and the other way round."""
    dp, op = _big_pnp()
    de, oe = _big_ess()
    small_p = _pnp_small_batch()
    small_e = [_gated_batch(rc.build(rc.ESS_CASES[t]), _ess_opt(rc.ESS_CASES[t])) for t in ("gate0", "gate129", "gate_stopped")]

    def big(c):
        return c.pnp_ransac(dp["obj"], dp["img"], dp["intr"], op), c.essential_ransac(de["pts_last"], de["pts_curr"],
                                                                                      de["intr"], oe)

    def small(c):
        return [c.pnp_ransac_batch(*small_p)] + [c.essential_ransac_batch(*a) for a in small_e]

    fresh = vxslam.Context(0)
    used = vxslam.Context(0)
    try:
        ref = small(fresh) if order == "big_first" else list(big(fresh))
        first = big(used) if order == "big_first" else small(used)
        assert first is not None
        got = small(used) if order == "big_first" else list(big(used))
        for a, b in zip(got, ref):
            _equal(a, b)
    finally:
        fresh.close()
        used.close()
