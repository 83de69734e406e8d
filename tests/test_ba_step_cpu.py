"""oracle/ba_oracle.cpp against one exact Gauss-Newton iteration (tests/ba_step_ref.py) on placed
windows: every decision (gate, depth, the two min_* counts, the stop on zero observations) identical,
skipped entries bitwise unchanged, applied ones within C_ORACLE times the error model.  Landmarks are
judged from the restatement's own poses (landmark_stage): the error of a pose step of kappa 1e11 is a
thousand times a landmark's own bracket and is already judged once, on the pose."""
import numpy as np
import pytest
from mpmath import mp, mpf

import ba_step_ref as R


def _run(oracle, m, opts):
    out = m.copy()
    st = oracle.ba_optimize(out, oracle.ba_options(**R.options(**opts)))
    assert st.status == 0
    return out, st


def _check_iteration(ref, m0, m1, obs, cost, name, exact, C):
    return R.check_iteration(ref, ref["opts"], m0, m1, obs, cost, name, exact, C, 1e-13)


_worst = {}


@pytest.mark.parametrize("name", R.NAMES)
def test_restatement_matches_step(oracle, name):
    m, opts, _ = R.case(name)
    ref = dict(R.reference(name), opts=opts)
    m1, st = _run(oracle, m, opts)
    assert st.iterations == 1
    _worst[name] = _check_iteration(ref, m, m1, st.obs[0], st.cost[0], name, name in R.EXACT_COST, R.C_ORACLE)
    print(f"{name}: restatement needs C = {_worst[name]:.3g}")


def test_c_oracle_is_what_the_restatement_needs(oracle):
    """C_ORACLE is the restatement's own figure rounded up, not a guess: within a factor 2 of it."""
    for name in R.NAMES:
        if name not in _worst:
            test_restatement_matches_step(oracle, name)
    worst = max(_worst.values())
    print("largest C:", worst, max(_worst, key=_worst.get))
    assert R.C_ORACLE / 2 <= worst <= R.C_ORACLE
    assert R.C_DEV == 2.0 ** int(np.ceil(np.log2(16 * R.C_ORACLE)))


@pytest.mark.parametrize("name", R.TWO_ITER)
def test_restatement_second_iteration(oracle, name):
    """Iteration 2 from the restatement's own iteration-1 state."""
    m, opts, _ = R.case(name)
    m1, _ = _run(oracle, m, opts)
    m2, st = _run(oracle, m, dict(opts, iters=2))
    assert st.iterations == 2
    start = R.advanced(m, m1["kf_pose"], m1["lm_pos"])
    ref = dict(R.step(start, opts), opts=opts)
    assert ref["gate"] >= 1e-6, f"{name}: gate distance {ref['gate']} in iteration 2: reseed this case"
    _check_iteration(ref, start, m2, st.obs[1], st.cost[1], name + "[it 2]", False, R.C_ORACLE)


def test_tiny_is_bitwise(oracle):
    m, opts, _ = R.case("tiny")
    R.reference("tiny")
    m1, st = _run(oracle, m, opts)
    assert st.obs[0] == 30 and st.cost[0] == 0.0
    assert np.array_equal(m["kf_pose"], m1["kf_pose"]) and np.array_equal(m["lm_pos"], m1["lm_pos"])


def test_all_gated_stops(oracle):
    """total_obs == 0 ends the run after its first iteration, whatever max_iterations says."""
    m, opts, _ = R.case("all_gated")
    R.reference("all_gated")
    m1, st = _run(oracle, m, dict(opts, iters=5))
    assert st.iterations == 1 and st.obs[0] == 0 and st.cost[0] == 0.0
    assert np.array_equal(m["kf_pose"], m1["kf_pose"]) and np.array_equal(m["lm_pos"], m1["lm_pos"])


@pytest.mark.parametrize("name", R.NAMES)
def test_reference_precision(name):
    """50 digits are enough: the same step at 100 digits agrees to 1e-40."""
    m, opts, _ = R.case(name)
    a, b = R.reference(name), R.step(m, opts, dps=100)
    assert a["obs"] == b["obs"]
    with mp.workdps(100):
        d = [abs(a["cost"] - b["cost"])]
        for key, vals in (("kf", ("pose", "dx")), ("lm", ("pos", "dp"))):
            for row, ra in a[key].items():
                rb = b[key][row]
                assert ra["applied"] == rb["applied"] and ra["obs"] == rb["obs"]
                for v in vals:
                    d += [abs(x - y) for x, y in zip(ra[v], rb[v])]
        assert max(d) <= mpf(10) ** -40, (name, mp.nstr(max(d), 5))
