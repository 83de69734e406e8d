"""The Schur BA on the device, one Levenberg-Marquardt iteration at a time, against the 50-digit
reference of tests/sba_step_ref.py on placed windows: a diagonal block 4e-7 of max|S|, residuals exactly
on and 2^-20 beside the reprojection and Huber gates, depths on and one ulp beside 1e-6, held and
pose-stage-only landmarks, a keyframe with every observation gated, the k_sba_lm packing limits (256
observations, 256 landmarks), a diagonal block of more than 256 observations and self pairs, millimetre
parallax, every branch of se3_left_update, a rejected first step, zero cost and zero observations.
Every case runs through every variant:

    default   the plan as built
    split3    VX_SBA_DIAG_SPLIT=3: each diagonal block over three workgroups + k_sba_blocks_diag
    split8    VX_SBA_DIAG_SPLIT=8 (most parts empty on these windows)
    single    VX_SBA_FACTOR=single: the one-workgroup k_sba_solve
    dmap      the plan built on the device from the resident map (DMap.sba_plan)
    shard2    two landmark shards run by vx_sba_shard_emulate_run, their systems summed in rank order
    one_call  Context.sba_optimize (state and statistics only)

max_iterations = 1: system() per entry of the lower triangle under C_DEV_SYS brackets, obs[0] equal,
cost[0] within 1e-12 (exact on the lattice), the state bitwise unchanged.  max_iterations = 2: step()
against the 50-digit solve of the same variant's own system (per covisibility component, C_SOLVE
kappa 2^-53 |dx|), fail == 0, step[1] the reference's decision; on an accept the fetched state against
trial() at the device's own dx within C_DEV_STATE times the model (fixed, held, pose-only entries
bitwise) and cost[1] / obs[1] against the assembly of that fetched state; on a reject the state bitwise
the input and cost[1] against the assembly at trial(dx_device) within 1e-9 (the trial state is not
fetched: its rounding, <= C_DEV_STATE brackets of ~1e-15, moves a cost by |grad| / cost ~ 1e4 times that).
max_iterations = 3 pins the damping of the third assembly, the stop rules get tests of their own."""
import numpy as np
import pytest

import ba_step_ref as R
import sba_step_ref as S

pytestmark = pytest.mark.gpu

VARIANTS = {
    "default": {},
    "split3": {"VX_SBA_DIAG_SPLIT": "3"},
    "split8": {"VX_SBA_DIAG_SPLIT": "8"},
    "single": {"VX_SBA_FACTOR": "single"},
    "dmap": {},
    "shard2": {},
    "one_call": {},
}
HOOKS = [v for v in VARIANTS if v != "one_call"]  # variants with system() and step()

_runs, _asm, _worst, _seen = {}, {}, {}, set()


def _options(kw, **over):
    import vxslam

    o = S.options(**dict(kw, **over))
    return vxslam.default_sba_options(window=o["window"], iters=o["iters"], min_point=o["min_point"], fixed=o["fixed"],
                                      huber=o["huber"], max_err=o["max_err"], lam=o["lam"], rel_tol=o["rel_tol"])


def _run(ctx, name, variant, iters, **over):
    """dict(out, st, S, rhs, dx, fail) of one run, made once per (case, variant, iterations, overrides)."""
    key = (name, variant, iters, tuple(sorted(over.items())))
    if key in _runs:
        return _runs[key]
    import vxslam

    m, kw, _ = S.case(name)
    opts = _options(kw, iters=iters, **over)
    out = m.copy()
    rec = dict(S=None, rhs=None, dx=None, fail=0)
    with pytest.MonkeyPatch.context() as mp:
        for k, v in VARIANTS[variant].items():
            mp.setenv(k, v)  # (read at plan build and at run)
        if variant == "one_call":
            st = ctx.sba_optimize(out, opts)
        elif variant == "dmap":
            dm = vxslam.DMap(ctx)
            kf_order, lm_order = vxslam.dmap_load(dm, m)
            plan = dm.sba_plan(opts, ref_kf_id=m["ref_kf_id"])
            plan.run_async()
            st = plan.fetch()
            plan.apply(dm)
            pose, pos = dm.download()
            out["kf_pose"].reshape(-1, 7)[kf_order] = pose
            out["lm_pos"].reshape(-1, 3)[lm_order] = pos
            plans = [plan]
        elif variant == "shard2":
            plans = [ctx.sba_plan(m, opts, shard_rank=r, shard_count=2) for r in range(2)]
            assert sum(p.info()["n_opt"] for p in plans) == len(S.reference(name)["asm"]["lms"])
            ctx.sba_shard_emulate(plans)
            sts = [p.fetch(out) for p in plans]  # (each shard writes the poses and its own landmarks)
            st = sts[0]
            assert (list(sts[1].step), list(sts[1].cost), list(sts[1].obs)) == (list(st.step), list(st.cost), list(st.obs))
        else:
            plans = [ctx.sba_plan(m, opts)]
            plans[0].run_async()
            st = plans[0].fetch(out)
        if variant != "one_call":
            rec["S"], rec["rhs"] = plans[0].system()
            rec["dx"], rec["fail"] = plans[0].step()
            for p in plans:
                p.close()
            if variant == "dmap":
                dm.close()
    assert st.status == 0
    rec.update(out=out, st=st)
    _runs[key] = rec
    if not over:
        _seen.add((name, variant, iters))
    return rec


def _note(kind, variant, name, ratio, C):
    _worst[(kind, variant)] = max(_worst.get((kind, variant), (0.0, "")), (float(ratio), name))
    print(f"{name}[{variant}]: {kind} needs C = {ratio:.3g} of {C:g}")


def _assembly_at(name, state_map, lam, tag):
    """assemble() of a case at a fetched state (doubles), once per distinct state."""
    m, kw, _ = S.case(name)
    key = (name, state_map["kf_pose"].tobytes(), state_map["lm_pos"].tobytes(), lam)
    if key not in _asm:
        _asm[key] = S.assemble(R.advanced(m, state_map["kf_pose"], state_map["lm_pos"]), kw, lam, moved=True)
        a = _asm[key]
        assert a["gate"] >= 1e-6 and a["z"] >= 1e-6, f"{tag}: a residual {a['gate']:.3g} from a gate at this state"
    return _asm[key]


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", S.NAMES)
def test_assembly(ctx, name, variant):
    m, kw, _ = S.case(name)
    ref = S.reference(name)
    a0 = ref["asm"]
    run = _run(ctx, name, variant, 1)
    st, what = run["st"], f"{name}[{variant}]"
    assert st.iterations == 1 and st.step[0] == 2 and st.accepted == 0
    assert (st.n_window_kf, st.n_landmarks) == (len(a0["win"]), len(a0["lms"]))
    assert st.obs[0] == a0["count"], f"{what}: obs {st.obs[0]} != {a0['count']}"
    S.check_cost(st.cost[0], a0["cost"], name in S.EXACT_COST, what)
    S.bitwise_state(m, run["out"], what)
    if variant in HOOKS:
        assert run["fail"] == 0
        _note("system", variant, name, S.compare_system(a0, run["S"], run["rhs"], S.C_DEV_SYS, what), S.C_DEV_SYS)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", S.NAMES)
def test_step(ctx, name, variant):
    m, kw, _ = S.case(name)
    ref = S.reference(name)
    a0, d = ref["asm"], ref["decision"]
    run = _run(ctx, name, variant, 2)
    st, out, what = run["st"], run["out"], f"{name}[{variant}]"
    assert run["fail"] == 0
    assert st.obs[0] == a0["count"]
    if "asm1" not in ref:  # the run stops on zero observations
        assert st.iterations == 1
        S.bitwise_state(m, out, what)
        return
    assert st.iterations == 2 and list(st.step[:2]) == [2, d["step"]], f"{what}: steps {list(st.step[:2])}, reference {d['step']}"
    assert st.accepted == d["accepted"] and st.lambda_ == d["lam"], (st.accepted, st.lambda_, d["lam"])
    if variant in HOOKS:
        one = _run(ctx, name, variant, 1)
        r = S.compare_step(run["dx"], one["S"], one["rhs"], ref["sol"]["comps"], S.C_SOLVE, what)
        _note("solve", variant, name, r, S.C_SOLVE)
        for r_, fx in enumerate(a0["fixed"]):
            if fx:
                assert not run["dx"][6 * r_:6 * r_ + 6].any()
        dx = run["dx"]
    else:
        dx = _run(ctx, name, "default", 2)["dx"]  # (one_call is the default plan: the same bits)
    if d["step"] == 1:
        tr = S.trial(m, a0, dx, ref["sol"]["kappa"])
        _note("state", variant, name, S.compare_trial(tr, m, out, S.C_DEV_STATE, what), S.C_DEV_STATE)
        a1 = _assembly_at(name, out, ref["opts"]["lam"], what)
        assert st.obs[1] == a1["count"], f"{what}: obs[1] {st.obs[1]} != {a1['count']}"
        S.check_cost(st.cost[1], a1["cost"], False, what + " (trial)")
    else:
        S.bitwise_state(m, out, what + " (rejected)")
        key = (name, "trial", dx.tobytes())
        if key not in _asm:
            tr = S.trial(m, a0, dx, ref["sol"]["kappa"])
            _asm[key] = S.assemble(m, kw, ref["opts"]["lam"], state=S.trial_state(tr))
        a1 = _asm[key]
        assert st.obs[1] == a1["count"]
        S.check_cost(st.cost[1], a1["cost"], name == "zero_cost", what + " (rejected trial)", 1e-9)


@pytest.mark.parametrize("variant", HOOKS)
@pytest.mark.parametrize("name", ["dead_kf", "zero_cost"])
def test_zero_rows_are_exact(ctx, name, variant):
    """A keyframe whose every observation is gated, and a window without residuals: rhs and dx rows exactly
    zero, and after the accepted step of dead_kf the keyframe's pose bitwise what it was."""
    m, _, _ = S.case(name)
    S.reference(name)
    run = _run(ctx, name, variant, 2)
    rows = range(18, 24) if name == "dead_kf" else range(18)
    assert not run["dx"][list(rows)].any()
    assert not _run(ctx, name, variant, 1)["rhs"][list(rows)].any()
    if name == "dead_kf":
        assert run["st"].step[1] == 1
        assert np.array_equal(m["kf_pose"].reshape(-1, 7)[3].view(np.uint64), run["out"]["kf_pose"].reshape(-1, 7)[3].view(np.uint64))


@pytest.mark.parametrize("variant", HOOKS)
@pytest.mark.parametrize("name,lam_next,steps", [("generic", 1e-4 * 0.1, [2, 1, 1]), ("ill_landmark", 1e-6, [2, 1, 1]),
                                                 ("reject", 1e-9 * 10.0, [2, 0, 3])])
def test_lambda_path(ctx, name, variant, lam_next, steps):
    """The third assembly's damping: lam * 0.1 after an accept, clamped at 1e-6 (ill_landmark starts there: 1e-7
    would show on every diagonal entry at 1e-6 relative), lam * 10 after a reject, which also pins that the
    rejected trial state is not what is assembled again.  After an accept the third assembly is of the
    second trial state; the cases are chosen so that it is accepted (asserted), so it is the fetched state."""
    m, kw, _ = S.case(name)
    S.reference(name)
    run = _run(ctx, name, variant, 3)
    st, what = run["st"], f"{name}[{variant}, it 3]"
    assert run["fail"] == 0 and st.iterations == 3 and list(st.step[:3]) == steps, list(st.step[:3])
    if steps[1] == 0:
        S.bitwise_state(m, run["out"], what)
        assert run["st"].cost[2] == run["st"].cost[0]
    else:
        # the second step starts from the accepted state, not from the one before it: the fetched state
        # against trial() of the assembly at this variant's max_iterations = 2 output, at the device's dx
        two = _run(ctx, name, variant, 2)
        assert not np.array_equal(two["out"]["kf_pose"], run["out"]["kf_pose"])
        a1 = _assembly_at(name, two["out"], S.options(**kw)["lam"], what)
        start = R.advanced(m, two["out"]["kf_pose"], two["out"]["lm_pos"])
        comps = S.components(a1)
        tr = S.trial(start, a1, run["dx"], S.solve_system(a1["S"], a1["rhs"], comps)[1])
        _note("state", variant, name + "/it3", S.compare_trial(tr, start, run["out"], S.C_DEV_STATE, what), S.C_DEV_STATE)
    a = _assembly_at(name, run["out"], lam_next, what)
    assert st.obs[2] == a["count"]
    S.check_cost(st.cost[2], a["cost"], False, what)
    _note("system", variant, name + "/it3", S.compare_system(a, run["S"], run["rhs"], S.C_DEV_SYS, what), S.C_DEV_SYS)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_stop_rules(ctx, variant):
    m, _, _ = S.case("zero_cost")
    for c in ("zero_cost", "generic", "all_gated"):
        S.reference(c)
    # lam * 10 > 1e12 after the first reject
    run = _run(ctx, "zero_cost", variant, 6, lam=2e11)
    assert run["st"].iterations == 2 and list(run["st"].step[:2]) == [2, 0] and run["st"].lambda_ == 2e12
    # reject, re-assemble, reject, ...: nothing moves by a bit
    run = _run(ctx, "zero_cost", variant, 6)
    assert run["st"].iterations == 6 and list(run["st"].step[:6]) == [2, 0, 3, 0, 3, 0] and run["st"].accepted == 0
    assert list(run["st"].cost[:6]) == [0.0] * 6 and list(run["st"].obs[:6]) == [30] * 6
    S.bitwise_state(m, run["out"], f"zero_cost[{variant}]")
    # rel < rel_tol after an accept
    ref = S.reference("generic")
    rel = float((ref["asm"]["cost"] - ref["asm1"]["cost"]) / ref["asm"]["cost"])
    assert 0.1 < rel < 0.9
    run = _run(ctx, "generic", variant, 6, rel_tol=0.99)
    assert run["st"].iterations == 2 and list(run["st"].step[:2]) == [2, 1]
    two = _run(ctx, "generic", variant, 2)
    S.bitwise_state(two["out"], run["out"], f"generic[{variant}, rel_tol 0.99]")
    run = _run(ctx, "generic", variant, 6, rel_tol=0.0)
    assert run["st"].iterations == 6 and run["st"].accepted >= 2
    # no valid observation
    mg, _, _ = S.case("all_gated")
    run = _run(ctx, "all_gated", variant, 5)
    assert run["st"].iterations == 1 and run["st"].obs[0] == 0 and run["st"].cost[0] == 24 * 25.0
    S.bitwise_state(mg, run["out"], f"all_gated[{variant}]")


def test_report_device_ratios():
    """The largest multiple of each model every variant needed in this session (DESIGN.md §10 quotes
    them), and no (case, variant) left out of either iteration count (this test runs after the others)."""
    missing = {(n, v, i) for n in S.NAMES for v in VARIANTS for i in (1, 2)} - _seen
    assert not missing, sorted(missing)[:8]
    for (kind, variant), (ratio, name) in sorted(_worst.items()):
        print(f"{kind:6s} {variant:8s}: largest C = {ratio:.3g} ({name})")
    caps = dict(system=S.C_DEV_SYS, solve=S.C_SOLVE, state=S.C_DEV_STATE)
    assert all(r <= caps[kind] for (kind, _), (r, _) in _worst.items())
