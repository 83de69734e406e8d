"""oracle/sba_oracle.cpp against one exact Levenberg-Marquardt iteration of the Schur BA
(tests/sba_step_ref.py) on placed windows: every case is what it claims (its own check), the
restatement's reduced system within C_ORACLE_SYS brackets per entry, its counts and decisions identical,
its cost within 1e-13 (exact on the lattice), its state after one step (max_iterations = 2) within
C_ORACLE_STATE times the error model on an accept and bitwise the input on a reject.  The two constants
are measured here and asserted to be the restatement's own figures rounded up to a power of two."""
import time

import numpy as np
import pytest
from mpmath import mp, mpf

import sba_step_ref as S

_sys, _state = {}, {}


def _opts(oracle, kw, **over):
    o = S.options(**dict(kw, **over))
    return oracle.sba_options(window=o["window"], iters=o["iters"], min_point=o["min_point"], fixed=o["fixed"],
                              huber=o["huber"], max_err=o["max_err"], lam=o["lam"], rel_tol=o["rel_tol"])


@pytest.mark.parametrize("name", S.NAMES)
def test_case_is_what_it_claims(name):
    S.reference(name)


@pytest.mark.parametrize("name", S.NAMES)
def test_restatement_system(oracle, name):
    m, kw, _ = S.case(name)
    ref = S.reference(name)
    Sc, rc = oracle.sba_system(m, _opts(oracle, kw), lam=S.options(**kw)["lam"])
    _sys[name] = S.compare_system(ref["asm"], Sc, rc, S.C_ORACLE_SYS, name)
    print(f"{name}: restatement's system needs C = {_sys[name]:.3g}")


@pytest.mark.parametrize("name", S.NAMES)
def test_restatement_step(oracle, name):
    m, kw, _ = S.case(name)
    ref = S.reference(name)
    a0 = ref["asm"]
    m1 = m.copy()
    st = oracle.sba_optimize(m1, _opts(oracle, kw, iters=2))
    assert st.status == 0 and (st.n_window_kf, st.n_landmarks) == (len(a0["win"]), len(a0["lms"]))
    exact = name in S.EXACT_COST
    assert st.obs[0] == a0["count"] and st.step[0] == 2
    S.check_cost(st.cost[0], a0["cost"], exact, name, 1e-13)
    if "asm1" not in ref:
        assert st.iterations == 1
        S.bitwise_state(m, m1, name)
        _state[name] = 0.0
        return
    d = ref["decision"]
    assert st.iterations == 2 and st.step[1] == d["step"] and st.obs[1] == ref["asm1"]["count"]
    assert st.accepted == d["accepted"] and st.lambda_ == d["lam"], (st.accepted, st.lambda_, d)
    S.check_cost(st.cost[1], ref["asm1"]["cost"], name == "zero_cost", name + " (trial)", 1e-9)
    if d["step"] == 0:
        S.bitwise_state(m, m1, name + " (rejected)")
        _state[name] = 0.0
    else:
        # poses and landmarks are judged at the restatement's own dx, the dx against the 50-digit solve of
        # the restatement's own system (bitwise what orc_sba_system returns: the same assembly)
        dx = oracle.sba_last_step(st.n_window_kf)
        Sc, rc = oracle.sba_system(m, _opts(oracle, kw), lam=ref["opts"]["lam"])
        S.compare_step(dx, Sc, rc, ref["sol"]["comps"], S.C_SOLVE, name)
        tr = S.trial(m, a0, dx, ref["sol"]["kappa"])
        _state[name] = S.compare_trial(tr, m, m1, S.C_ORACLE_STATE, name)
        if name == "dead_kf":  # dx = 0 exactly: the keyframe's pose keeps its bits through an accepted step
            assert not dx[18:24].any()
            assert np.array_equal(m["kf_pose"].reshape(-1, 7)[3].view(np.uint64), m1["kf_pose"].reshape(-1, 7)[3].view(np.uint64))
    print(f"{name}: restatement's state needs C = {_state[name]:.3g}")


def test_constants_are_what_the_restatement_needs(oracle):
    for name in S.NAMES:
        if name not in _sys:
            test_restatement_system(oracle, name)
        if name not in _state:
            test_restatement_step(oracle, name)
    ws, wt = max(_sys, key=_sys.get), max(_state, key=_state.get)
    print(f"largest C: system {_sys[ws]:.3g} ({ws}), state {_state[wt]:.3g} ({wt})")
    assert S.C_ORACLE_SYS / 2 <= _sys[ws] <= S.C_ORACLE_SYS
    assert S.C_ORACLE_STATE / 2 <= _state[wt] <= S.C_ORACLE_STATE
    assert (S.C_DEV_SYS, S.C_DEV_STATE) == (16 * S.C_ORACLE_SYS, 16 * S.C_ORACLE_STATE)


def test_decide_replays_a_long_run(oracle):
    """decide() over the restatement's recorded costs and counts of an 8-iteration run gives its step
    codes, iteration count and accept count, on an accepting and on a rejecting start."""
    for name in ("generic", "reject", "zero_cost", "lattice_gate13"):
        m, kw, _ = S.case(name)
        st = oracle.sba_optimize(m.copy(), _opts(oracle, kw, iters=8))
        n = st.iterations
        steps, last = S.replay(list(st.cost[:n]), list(st.obs[:n]), S.options(**dict(kw, iters=8)))
        assert steps == list(st.step[:n]) and len(steps) == n, (name, steps, list(st.step[:n]))
        assert last["accepted"] == st.accepted


def test_reference_precision_and_time():
    """50 digits are enough (the same assembly and solve at 100 digits agree to 1e-30 relative), and the
    whole reference set costs well under a minute of CPU."""
    t0 = time.perf_counter()
    for name in S.NAMES:
        S.reference(name)
    total = sum(S.ref_seconds.values())
    print(f"reference set: {total:.1f} s ({max(S.ref_seconds, key=S.ref_seconds.get)} the longest), "
          f"{time.perf_counter() - t0:.1f} s in this test")
    assert total < 60.0
    for name in ("generic", "far_block", "ill_landmark"):
        m, kw, _ = S.case(name)
        a, b = S.reference(name)["asm"], S.assemble(m, kw, S.options(**kw)["lam"], dps=100)
        with mp.workdps(100):
            top = max(abs(v) for row in b["S"] for v in row)
            d = max(abs(x - y) for ra, rb in zip(a["S"], b["S"]) for x, y in zip(ra, rb))
            assert d <= mpf(10) ** -30 * top and abs(a["cost"] - b["cost"]) <= mpf(10) ** -30 * b["cost"]
