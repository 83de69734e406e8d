"""k_ba_win's row hand-off: every (workgroup, keyframe) entry's pose-stage terms travel as tagged
granules in the entry's own partial slot (the data is the flag), and the consumer sums a row's slots
in slot order.  So a persistent window is bitwise repeatable — over the runs of a plan (tags derive
from the plan's run generation: stale granules of earlier runs and of iterations an early stop
skipped must never match), over plan builds, against k_ba_iter's slot sums — and a stale or torn
granule changes bits.  Parity bars as tests/test_gpu_parity.py (BASELINE.json north_star)."""
import os

import numpy as np
import pytest

from vxslam import synth

pytestmark = pytest.mark.gpu

BA_RTOL = 1e-4
GATE_MARGIN = 1e-6
RUNS = 4  # eager, captured, replayed twice: several generations of tags over the same granules

# (name, map arguments, options): cases tests/test_gpu_parity.py already runs against the restatement
CASES = [
    ("w12", (201, 12, 2500, dict(n_old_kf=4)), dict(window=12)),
    ("w12_iters1", (201, 12, 2500, dict(n_old_kf=4)), dict(window=12, iters=1)),
    # stops early: the iterations after the stop keep the granules and tags of whatever ran them last
    ("w12_iters20", (201, 12, 2500, dict(n_old_kf=4)), dict(window=12, iters=20)),
    ("C2", (0x5EED0000 + 10, 10, 2000, dict(n_streams=1, n_old_kf=2)), dict(window=10)),
]
IDS = [c[0] for c in CASES]


def _canon(q):
    q = q.copy()
    q[q[:, 3] < 0] *= -1
    return q


def _assert_ba_close(m_gpu, m_cpu, st_gpu, st_cpu):
    assert st_gpu.status == st_cpu.status
    assert st_gpu.n_window_kf == st_cpu.n_window_kf and st_gpu.n_landmarks == st_cpu.n_landmarks
    assert st_gpu.iterations == st_cpu.iterations
    assert list(st_gpu.obs[:st_gpu.iterations]) == list(st_cpu.obs[:st_cpu.iterations])  # no gate flips
    for a, b in zip(st_gpu.cost[:st_gpu.iterations], st_cpu.cost[:st_cpu.iterations]):
        assert abs(a - b) <= 1e-6 * abs(b)
    pg, pc = m_gpu["kf_pose"].copy(), m_cpu["kf_pose"].copy()
    pg[:, :4], pc[:, :4] = _canon(pg[:, :4]), _canon(pc[:, :4])
    for a, b in ((pg, pc), (m_gpu["lm_pos"], m_cpu["lm_pos"])):
        err = np.abs(a - b) / np.maximum(np.abs(b), 1e-3)
        assert err.max() <= BA_RTOL, err.max()


def _assert_bitwise(a, b, sa, sb):
    assert sa.iterations == sb.iterations
    assert np.array_equal(a["kf_pose"], b["kf_pose"]) and np.array_equal(a["lm_pos"], b["lm_pos"])
    assert list(sa.cost[:16]) == list(sb.cost[:16])
    assert list(sa.obs[:16]) == list(sb.obs[:16])


def _run(plan, m, n):
    out = []
    for _ in range(n):
        plan.run_async()
        mm = m.copy()
        st = plan.fetch(mm)
        out.append((mm, st))
    return out


_cache = {}


def _case(ctx, oracle, name):
    """One case's runs, made once: RUNS runs of a persistent plan, one of a second plan built from
    the same map, one of a plan on k_ba_iter's partial slots, and the restatement."""
    if name in _cache:
        return _cache[name]
    import vxslam

    _, (seed, nk, nl, kw), opts_kw = next(c for c in CASES if c[0] == name)
    m = synth.make_ba_map(seed, nk, nl, **kw)
    mc = m.copy()
    st_c = oracle.ba_optimize(mc, oracle.ba_options(**opts_kw))
    assert st_c.gate_margin >= GATE_MARGIN, f"gate margin {st_c.gate_margin}: reseed this case"
    opts = vxslam.default_ba_options(**opts_kw)
    plan = ctx.ba_plan(m, opts)
    persistent = [plan.persistent()]
    runs = _run(plan, m, RUNS)
    persistent.append(plan.persistent())  # (no run fell back)
    plan.close()
    plan2 = ctx.ba_plan(m, opts)
    persistent.append(plan2.persistent())
    second = _run(plan2, m, 1)[0]
    persistent.append(plan2.persistent())
    plan2.close()
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("VX_BA_ATOMIC_ROWS", "0")  # (read at plan build)
        plan3 = ctx.ba_plan(m, opts)
    slots_persistent = plan3.persistent()
    slots = _run(plan3, m, 1)[0]
    plan3.close()
    _cache[name] = dict(cpu=(mc, st_c), runs=runs, second=second, slots=slots, persistent=persistent,
                        slots_persistent=slots_persistent)
    return _cache[name]


@pytest.mark.parametrize("name", IDS)
def test_win_runs_match_oracle(ctx, oracle, name):
    r = _case(ctx, oracle, name)
    assert all(r["persistent"]), r["persistent"]
    for mg, st in r["runs"]:
        _assert_ba_close(mg, r["cpu"][0], st, r["cpu"][1])


@pytest.mark.parametrize("name", IDS)
def test_win_runs_and_builds_bitwise(ctx, oracle, name):
    r = _case(ctx, oracle, name)
    assert all(r["persistent"]), r["persistent"]
    m0, s0 = r["runs"][0]
    for mg, st in r["runs"][1:]:
        _assert_bitwise(mg, m0, st, s0)
    _assert_bitwise(r["second"][0], m0, r["second"][1], s0)


@pytest.mark.parametrize("name", IDS)
def test_win_matches_slot_sums(ctx, oracle, name):
    """k_ba_iter on its partial slots sums every row in the same slot order from the same pose-stage
    terms: the same poses and landmarks bit for bit; the stop rule sums in another order (per slot
    there, per row here), so the costs agree to rounding."""
    r = _case(ctx, oracle, name)
    assert all(r["persistent"]) and not r["slots_persistent"]
    (mw, sw), (ms, ss) = r["runs"][0], r["slots"]
    assert sw.iterations == ss.iterations and list(sw.obs[:16]) == list(ss.obs[:16])
    assert np.array_equal(mw["kf_pose"], ms["kf_pose"]) and np.array_equal(mw["lm_pos"], ms["lm_pos"])
    for x, y in zip(sw.cost[:sw.iterations], ss.cost[:ss.iterations]):
        assert abs(x - y) <= 1e-9 * abs(y)


def _c3(ctx):
    """The window bench.py times (129 workgroups, every XCD) on its own context, run alone."""
    if "C3" in _cache:
        return _cache["C3"]
    import vxslam

    nk, nl, ns = synth.ba_config("C3")
    m = synth.make_ba_map(0x5EED0000 + nk, nk, nl, n_streams=ns, n_old_kf=ns * 2)
    bctx = vxslam.Context(0)
    plan = bctx.ba_plan(m, vxslam.default_ba_options(window=nk))
    assert plan.persistent()
    alone = _run(plan, m, 3)
    _cache["C3"] = dict(m=m, bctx=bctx, plan=plan, alone=alone)
    return _cache["C3"]


@pytest.fixture(scope="module")
def c3(ctx):
    r = _c3(ctx)
    yield r
    r["plan"].close()
    r["bctx"].close()
    _cache.pop("C3", None)


def test_win_c3_runs_bitwise(c3):
    m0, s0 = c3["alone"][0]
    assert s0.status == 0 and s0.iterations >= 2
    for mg, st in c3["alone"][1:]:
        _assert_bitwise(mg, m0, st, s0)
    assert c3["plan"].persistent()


def test_win_c3_bitwise_under_uneven_load(ctx, c3):
    """The hand-off while another context keeps part of the chip busy (extraction of 640x480 frames
    back to back, as the pipeline's front end does): the producers arrive unevenly and the sweeps
    re-poll; every run still equals the window run alone bit for bit."""
    import torch
    import vxslam

    frames = synth.make_frames(43, 2)
    d = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    p = vxslam.default_orb_params(n_features=2000)
    m0, s0 = c3["alone"][0]
    plan, m = c3["plan"], c3["m"]
    for i in range(20):
        for s in range(3):
            ctx.orb_extract_async(d[(i + s) & 1].data_ptr(), 640, 480, 3, 640 * 3, s, p)
        plan.run_async()
        mm = m.copy()
        st = plan.fetch(mm)
        _assert_bitwise(mm, m0, st, s0)
    ctx.synchronize()
    assert plan.persistent()
