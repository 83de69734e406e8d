"""k_ba_win's pose solve: behind a workgroup barrier wave 0 solves every entry of its workgroup, lane p
the entry at position p, from the sums the eight sweeping waves staged in LDS.  Small windows put many
entries into few workgroups, so one wave's lanes solve more entries than the workgroup has waves and
some waves sweep (and stage) two or three entries — the case the C3 window (5-8 entries a workgroup)
does not reach.  The arithmetic is k_ba_iter's: every run is bitwise repeatable, bitwise equal to
k_ba_iter on its partial slots, and within tests/test_gpu_parity.py's bars of the restatement
(1e-4 relative, identical iteration and observation counts, gate margin >= 1e-6)."""
import numpy as np
import pytest

from vxslam import synth

pytestmark = pytest.mark.gpu

BA_RTOL = 1e-4
GATE_MARGIN = 1e-6
RUNS = 4  # eager, captured, replayed twice
WAVES = 8  # of a 512-thread workgroup
FUSED_K = 64  # entry positions per workgroup (csrc/ba_plan.hpp: kBaFusedK)

# (name, map arguments, options, iterations of the restatement, its observation counts or None)
CASES = [
    ("s301", (301, 24, 400, dict(n_old_kf=4)), dict(window=24), 5, [1119, 516, 230, 161, 156]),
    ("s301_iters1", (301, 24, 400, dict(n_old_kf=4)), dict(window=24, iters=1), 1, [1119]),
    ("s303", (303, 20, 300, dict(n_old_kf=2)), dict(window=20), 5, None),
    # stops early: the stop rule's wave decides beside the solving wave
    ("s304_iters20", (304, 24, 400, dict(n_old_kf=4)), dict(window=24, iters=20), 8, None),
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


def _entries(plan):
    """entries (positions that hold a keyframe) per workgroup, from the plan's entry records"""
    lay = plan.layout()
    nb, ft = lay["workgroups"], lay["threads"]
    tab = np.frombuffer(plan.fused_tables(), np.int32)
    at = nb * 4 * (1 + ft // 128) + 7 * nb * ft  # blk | lm_slot | lm_run | lobs_rec, then the entries
    kent = tab[at: at + nb * FUSED_K * 8].reshape(nb, FUSED_K, 8)
    return ft, (kent[:, :, 0] >= 0).sum(1)


_cache = {}


def _map(name):
    _, (seed, nk, nl, kw), opts_kw, _, _ = next(c for c in CASES if c[0] == name)
    return synth.make_ba_map(seed, nk, nl, **kw), opts_kw


def _oracle(oracle, name):
    key = ("cpu", name)
    if key not in _cache:
        m, opts_kw = _map(name)
        st = oracle.ba_optimize(m, oracle.ba_options(**opts_kw))
        assert st.gate_margin >= GATE_MARGIN, f"gate margin {st.gate_margin}: reseed this case"
        _cache[key] = (m, st)
    return _cache[key]


def _case(ctx, oracle, name):
    """One case's runs, made once: RUNS runs of a persistent plan, one of a second plan built from
    the same map, one of a plan on k_ba_iter's partial slots, and the restatement."""
    if name in _cache:
        return _cache[name]
    import vxslam

    m, opts_kw = _map(name)
    cpu = _oracle(oracle, name)
    opts = vxslam.default_ba_options(**opts_kw)
    plan = ctx.ba_plan(m, opts)
    persistent = [plan.persistent()]
    threads, entries = _entries(plan)
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
    _cache[name] = dict(cpu=cpu, runs=runs, second=second, slots=slots, persistent=persistent,
                        slots_persistent=slots_persistent, threads=threads, entries=entries)
    return _cache[name]


@pytest.mark.parametrize("name", IDS)
def test_solve_wave_has_more_entries_than_waves(ctx, oracle, name):
    """The case is what it is meant to be: a 512-thread workgroup whose wave 0 solves more entries than
    the workgroup has waves, so at least one wave swept and staged two entries."""
    r = _case(ctx, oracle, name)
    assert all(r["persistent"]), r["persistent"]
    assert r["threads"] == 64 * WAVES
    assert r["entries"].max() > WAVES, f"entries per workgroup {r['entries'].tolist()}: reseed this case"


@pytest.mark.parametrize("name", IDS)
def test_solve_runs_match_oracle(ctx, oracle, name):
    r = _case(ctx, oracle, name)
    assert all(r["persistent"]), r["persistent"]
    _, _, _, iters, obs = next(c for c in CASES if c[0] == name)
    st_c = r["cpu"][1]
    assert st_c.iterations == iters
    if obs is not None:
        assert list(st_c.obs[:iters]) == obs
    for mg, st in r["runs"]:
        _assert_ba_close(mg, r["cpu"][0], st, st_c)


@pytest.mark.parametrize("name", IDS)
def test_solve_runs_and_builds_bitwise(ctx, oracle, name):
    r = _case(ctx, oracle, name)
    assert all(r["persistent"]), r["persistent"]
    m0, s0 = r["runs"][0]
    for mg, st in r["runs"][1:]:
        _assert_bitwise(mg, m0, st, s0)
    _assert_bitwise(r["second"][0], m0, r["second"][1], s0)


@pytest.mark.parametrize("name", IDS)
def test_solve_matches_slot_sums(ctx, oracle, name):
    """k_ba_iter on its partial slots solves every entry on wave 0's lanes from the same slot-order
    sums: the same poses and landmarks bit for bit; the stop rule sums in another order (per slot
    there, per row here), so the costs agree to rounding."""
    r = _case(ctx, oracle, name)
    assert all(r["persistent"]) and not r["slots_persistent"]
    (mw, sw), (ms, ss) = r["runs"][0], r["slots"]
    assert sw.iterations == ss.iterations and list(sw.obs[:16]) == list(ss.obs[:16])
    assert np.array_equal(mw["kf_pose"], ms["kf_pose"]) and np.array_equal(mw["lm_pos"], ms["lm_pos"])
    for x, y in zip(sw.cost[:sw.iterations], ss.cost[:ss.iterations]):
        assert abs(x - y) <= 1e-9 * abs(y)


def test_solve_fault_fallback(ctx, oracle, monkeypatch):
    """One arrival that never comes ($VX_BA_WIN_TEST_FAULT): the wave that sweeps row 0 runs out and
    sets the workgroup's fault word before the staging barrier, wave 0 does not solve, every wave
    passes both barriers and leaves, and vx_ba_plan_fetch re-runs the window with the per-iteration
    launches, which the plan then keeps."""
    import vxslam

    m, opts_kw = _map("s301")
    mc, st_c = _oracle(oracle, "s301")
    monkeypatch.setenv("VX_BA_WIN_TEST_FAULT", "1")
    plan = ctx.ba_plan(m, vxslam.default_ba_options(**opts_kw))
    assert plan.persistent()
    plan.run_async()
    mg = m.copy()
    st = plan.fetch(mg)
    assert not plan.persistent()
    _assert_ba_close(mg, mc, st, st_c)
    plan.run_async()
    mg = m.copy()
    _assert_ba_close(mg, mc, plan.fetch(mg), st_c)
    plan.close()
