"""The Schur BA's dense pose solve pinned at its OUTPUT: the step dx (vx_sba_plan_step) of every factor
form against an 80-bit Cholesky of the GPU's own reduced system, on covisibility the banded synth maps
never produce — loop closures (long-range tiles, panel gaps, fill), unequal components in one launch,
one- and two-tile systems, a system without padding rows, an isolated keyframe, a gauge-free window
(tests/sba_ref.py: the inputs, the reference and the bars; tests/test_sba_solve_cpu.py: the inputs do
what they claim).

Pairing dx with its system: with iters = 2, iteration 0 assembles S0, factors and solves, iteration 1
is the last and does not solve, so dx is the solve of S0 damped with lambda_init; a second plan with
iters = 1 gives S0 / rhs0 through plan.system() unfactored (the assembly is deterministic).  S0 is
symmetrised from its lower triangle, the bars are taken per connected component.

Measured on the MI355X (largest forward-error ratio to max(e64, n 2^-53) over the case's components,
bar 16; largest backward error, cap (3 n + 1) 2^-53): DESIGN.md §10.
"""
import numpy as np
import pytest

import sba_ref as R

pytestmark = pytest.mark.gpu

ENV = ("VX_SBA_FACTOR", "VX_SBA_FACTOR_GROUPS", "VX_SBA_FACTOR_COLS", "VX_SBA_LOOKAHEAD_LDS", "VX_SBA_PANEL_SLOTS")
SINGLE = ("single", dict(VX_SBA_FACTOR="single"))
FORMS = [
    ("default", {}),
    ("multi-g1", dict(VX_SBA_FACTOR="multi", VX_SBA_FACTOR_GROUPS="1")),
    ("multi-g2", dict(VX_SBA_FACTOR="multi", VX_SBA_FACTOR_GROUPS="2")),
    ("multi-g3", dict(VX_SBA_FACTOR="multi", VX_SBA_FACTOR_GROUPS="3")),
    ("multi-g2-global-lookahead", dict(VX_SBA_FACTOR="multi", VX_SBA_FACTOR_GROUPS="2", VX_SBA_LOOKAHEAD_LDS="0")),
    ("pair-g2", dict(VX_SBA_FACTOR="multi", VX_SBA_FACTOR_GROUPS="2", VX_SBA_FACTOR_COLS="2")),
    ("block-g1", dict(VX_SBA_FACTOR="block", VX_SBA_FACTOR_GROUPS="1")),
    ("block-g2", dict(VX_SBA_FACTOR="block", VX_SBA_FACTOR_GROUPS="2")),
    ("block-g5", dict(VX_SBA_FACTOR="block", VX_SBA_FACTOR_GROUPS="5")),
]
# case (g): the operands from global memory — two panel slots for the one-workgroup factor, the
# look-ahead column over global memory with one and with three workgroups per component
GLOBAL_FORMS = [
    ("single-2slots", dict(VX_SBA_FACTOR="single", VX_SBA_PANEL_SLOTS="2")),
    ("multi-g1-global-lookahead", dict(VX_SBA_FACTOR="multi", VX_SBA_FACTOR_GROUPS="1", VX_SBA_LOOKAHEAD_LDS="0")),
    ("multi-g3-global-lookahead", dict(VX_SBA_FACTOR="multi", VX_SBA_FACTOR_GROUPS="3", VX_SBA_LOOKAHEAD_LDS="0")),
]
CASES = [(n, False) for n in R.CASES] + [("e-loop26", True)]


def _form(monkeypatch, env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _run(ctx, m, kw, iters):
    """a fresh plan run once: (plan, map after the fetch, stats)"""
    import vxslam

    mm = m.copy()
    plan = ctx.sba_plan(mm, vxslam.default_sba_options(iters=iters, **kw))
    plan.run_async()
    st = plan.fetch(mm)
    return plan, mm, st


def _system(ctx, m, kw):
    """the first assembly S0 (symmetric), rhs0 and the components of the free keyframes, from the GPU"""
    plan, _, st = _run(ctx, m, kw, 1)
    S, rhs = plan.system()
    info = plan.info()
    plan.close()
    assert st.status == 0 and st.iterations == 1
    S = R.symmetrise(S)
    comps = R.components(R.block_pattern(S), R.free_keyframes(m, kw))
    assert info["n_comp"] == len(comps)
    # the host's symbolic factorisation against its numpy restatement: S's tiles plus the fill, and
    # the rhs row's tile per column
    tiles = [R.tile_pattern(R.block_pattern(S), c)[1] for c in comps]
    assert info["n_tiles"] == sum(int(t.sum()) + t.shape[0] for t in tiles), (info, [int(t.sum()) for t in tiles])
    return S, rhs, comps


def _step(ctx, m, kw):
    plan, _, st = _run(ctx, m, kw, 2)
    dx, fail = plan.step()
    plan.close()
    assert st.status == 0 and st.iterations == 2 and st.step[0] == 2  # (one solve: iteration 0's)
    assert fail == 0
    return dx


@pytest.mark.parametrize("name,global_operands", CASES, ids=[n + ("-g-global" if g else "") for n, g in CASES])
def test_sba_step_matches_extended_precision_solve(ctx, monkeypatch, name, global_operands):
    m, kw = R.case(name)
    _form(monkeypatch, {})
    S, rhs, comps = _system(ctx, m, kw)
    assert [len(c) for c in comps] == R.COMPONENTS[name]
    _form(monkeypatch, SINGLE[1])
    ref = _step(ctx, m, kw)
    free = R.free_keyframes(m, kw)
    for r in range(kw["window"]):
        if r not in free:
            assert not ref[6 * r:6 * r + 6].any()  # a gauge keyframe's step stays 0
    R.check_solution(S, rhs, ref, comps, f"{name}/single")
    for label, env in (GLOBAL_FORMS if global_operands else FORMS):
        _form(monkeypatch, env)
        dx = _step(ctx, m, kw)
        assert dx.tobytes() == ref.tobytes(), (name, label, np.abs(dx - ref).max())
        if label == "default":  # (bitwise the single form's: the same figures, checked on their own)
            R.check_solution(S, rhs, dx, comps, f"{name}/default")


def test_sba_step_hook_errors(ctx):
    import vxslam
    import ctypes as C

    m, kw = R.case("b-2tiles")
    plan = ctx.sba_plan(m, vxslam.default_sba_options(iters=2, **kw))
    with pytest.raises(vxslam.VxError, match="plan not run"):
        plan.step()
    plan.run_async()
    dx, fail = plan.step()
    assert dx.shape == (6 * kw["window"],) and fail == 0 and dx[12:].any()
    short, f = np.zeros(6), C.c_int32(0)
    assert vxslam.lib().vx_sba_plan_step(ctx.handle, plan._h, vxslam._p(short), 6, C.byref(f)) != 0  # n must be 30
    plan.close()
    empty = ctx.sba_plan(m, vxslam.default_sba_options(iters=2, **kw), ref_kf_id=int(m["kf_id"][0]))  # < 2 keyframes
    empty.run_async()
    with pytest.raises(vxslam.VxError, match="empty plan"):
        empty.step()
    empty.close()


def test_sba_no_stale_fill_after_a_factorisation(ctx, oracle, monkeypatch):
    """k_sba_blocks writes only S's nonzero blocks, so the factor's fill tiles must have been cleared
    (k_sba_update) before the next assembly.  iters = 2 on the 26-keyframe loop closure: iteration 1's
    assembly follows iteration 0's factorisation and evaluates the accepted trial state, the state the
    fetch returns; it equals the restatement's system there (damping lambda_init: the accept's smaller
    lambda is the next assembly's) within 1e-9 of max|S|, and every fill-only tile is exactly zero."""
    _form(monkeypatch, {})
    for name in ("e-loop26", "e-loop14-short"):
        m, kw = R.case(name)
        plan, mg, st = _run(ctx, m, kw, 2)
        S_g, r_g = plan.system()
        plan.close()
        assert list(st.step[:2]) == [2, 1]
        S_c, r_c = oracle.sba_system(mg, oracle.sba_options(iters=1, **kw), lam=kw["lam"])
        lo = np.tril_indices(S_c.shape[0])
        scale = np.abs(S_c[lo]).max()
        assert np.abs(S_g[lo] - S_c[lo]).max() <= 1e-9 * scale, (name, np.abs(S_g[lo] - S_c[lo]).max() / scale)
        assert np.abs(r_g - r_c).max() <= 1e-9 * max(np.abs(r_c).max(), 1.0)
        B = R.block_pattern(R.symmetrise(S_c))
        n_fill = 0
        for comp in R.components(B, R.free_keyframes(m, kw)):
            nzS, nzL = R.tile_pattern(B, comp)
            for i, j in zip(*np.nonzero(nzL & ~nzS)):
                tile = S_g[np.ix_(R.tile_rows(comp, i), R.tile_rows(comp, j))]
                assert tile.size and not tile.any(), (name, i, j, np.abs(tile).max())
                n_fill += 1
        assert n_fill >= 1


def test_sba_plan_reuse_on_a_loop_closure_is_bitwise(ctx, monkeypatch):
    """three runs of one plan (each after the first starts on its predecessor's factor, dx and state):
    dx, poses and landmarks bitwise equal"""
    import vxslam

    _form(monkeypatch, {})
    for name in ("e-loop14", "e-loop26"):
        m, kw = R.case(name)
        plan = ctx.sba_plan(m, vxslam.default_sba_options(iters=6, **kw))
        outs = []
        for _ in range(3):
            plan.run_async()
            mm = m.copy()
            st = plan.fetch(mm)
            dx, fail = plan.step()
            assert fail == 0 and st.accepted >= 2
            outs.append((dx.tobytes(), mm["kf_pose"].tobytes(), mm["lm_pos"].tobytes(), list(st.cost), list(st.step)))
        plan.close()
        assert outs[1] == outs[0] and outs[2] == outs[0], name


@pytest.mark.parametrize("name", ["e-loop14", "e-loop14-short", "e-loop26", "f-split-1-11", "f-split-3-9", "f-band-loop26"])
def test_sba_loop_and_split_windows_end_to_end(ctx, oracle, monkeypatch, name):
    """cases (e) and (f) through test_gpu_sba's parity check against the restatement at iters = 8"""
    from test_gpu_sba import _case

    _form(monkeypatch, {})
    m, kw = R.case(name)
    st_g, _ = _case(ctx, oracle, m, dict(iters=8, **kw))
    assert st_g.status == 0 and st_g.accepted >= 2
