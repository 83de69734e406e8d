"""LocalBA on the device, one Gauss-Newton iteration at a time, against the 50-digit reference of
tests/ba_step_ref.py, on placed windows: every branch of se3_left_update, pose systems of kappa up to
1e12, landmarks with millimetre parallax, residuals and depths exactly on and 2^-20 beside every gate,
both min_* counts at and one below their thresholds, and the stop on zero observations.  Every case
runs through every kernel variant a window of that size can take:

    win          the default: one persistent k_ba_win launch per window
    iter_atomic  VX_BA_PERSIST=0: k_ba_iter per iteration, row sums by atomics
    iter_slots   VX_BA_ATOMIC_ROWS=0: k_ba_iter on its partial slots
    t1024        VX_BA_FUSED_THREADS=1024: the 1024-thread form (pose_obs_accum<false>) C4 / C5 windows use
    t256         VX_BA_FUSED_THREADS=256
    unfused      VX_BA_FUSED=0: k_pose_kf + k_landmark_solve
    global       global_poses: the large-window kernels
    one_call     Context.ba_optimize: the plan built and run in one call

(VX_BA_COMPACT is a process-wide static, off by default, and is left out.  The two cases whose options
let a keyframe with one or two observations step, pose_obs1 and pose_obs2, run on the unfused kernels
under every id: plans with min_pose_observations < 3 do not take the fused layout.)  With iters=1: obs[0] equal
to the reference's, cost[0] within 1e-12 relative (exact on the weight-1 lattice cases), applied /
skipped identical, skipped entries bitwise unchanged, applied poses against step() and applied
landmarks against landmark_stage() on the fetched poses, both within C_DEV times the error model.
With iters=2 the reference of iteration 2 starts from the same variant's iters=1 output: the pose stage
that runs inside the kernel after the landmark stage is pinned apart from the prologue that feeds
iteration 0."""
import numpy as np
import pytest

import ba_step_ref as R

pytestmark = pytest.mark.gpu

VARIANTS = {
    "win": {},
    "iter_atomic": {"VX_BA_PERSIST": "0"},
    "iter_slots": {"VX_BA_ATOMIC_ROWS": "0"},
    "t1024": {"VX_BA_FUSED_THREADS": "1024"},
    "t256": {"VX_BA_FUSED_THREADS": "256"},
    "unfused": {"VX_BA_FUSED": "0"},
    "global": {},
    "one_call": {},
}

_runs = {}
_worst = {}


def _run(ctx, name, variant, iters=1):
    """(state, stats) of one run, made once per (case, variant, iterations)."""
    key = (name, variant, iters)
    if key in _runs:
        return _runs[key]
    import vxslam

    m, opts_kw, _ = R.case(name)
    opts = vxslam.default_ba_options(**R.options(**dict(opts_kw, iters=iters)))
    out = m.copy()
    if variant == "one_call":
        st = ctx.ba_optimize(out, opts)
    else:
        with pytest.MonkeyPatch.context() as mp:
            for k, v in VARIANTS[variant].items():
                mp.setenv(k, v)  # (read at plan build)
            plan = ctx.ba_plan(m, opts, global_poses=variant == "global")
        lay = plan.layout()
        # a plan that lets a keyframe with one or two observations step (min_pose < 3) takes the unfused
        # kernels whatever the environment says: only their pose solve carries the LDL^T branch such a
        # system needs (csrc/ba.hip fused_eligible, solve_pose<true>)
        can_fuse = R.options(**opts_kw)["min_pose"] >= 3
        if not can_fuse or variant in ("unfused", "global"):
            assert not lay["fused"] and not plan.persistent()
        elif variant == "win":
            assert plan.persistent()
        elif variant in ("iter_atomic", "iter_slots"):
            assert lay["threads"] == 512 and not plan.persistent()
        else:
            assert lay["threads"] == {"t1024": 1024, "t256": 256}[variant]
        if lay["fused"] and name in ("step_mixed", "step_1.5"):
            assert lay["workgroups"] == 1  # both sides of theta = 0.1 under one wave-wide vote
        plan.run_async()
        st = plan.fetch(out)
        if variant == "win" and can_fuse:
            assert plan.persistent()  # (the run did not fall back)
        plan.close()
    assert st.status == 0
    _runs[key] = (out, st)
    return _runs[key]


def _note(variant, name, ratio):
    _worst[variant] = max(_worst.get(variant, (0.0, "")), (ratio, name))
    print(f"{name}[{variant}]: needs C = {ratio:.3g} of C_DEV = {R.C_DEV:g}")


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", R.NAMES)
def test_one_iteration(ctx, name, variant):
    m, opts, _ = R.case(name)
    ref = R.reference(name)
    out, st = _run(ctx, name, variant)
    assert st.iterations == 1
    r = R.check_iteration(ref, opts, m, out, st.obs[0], st.cost[0], f"{name}[{variant}]", name in R.EXACT_COST,
                          R.C_DEV, 1e-12)
    _note(variant, name, r)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", R.TWO_ITER)
def test_second_iteration(ctx, name, variant):
    m, opts, _ = R.case(name)
    R.reference(name)
    out1, _ = _run(ctx, name, variant)
    out2, st = _run(ctx, name, variant, iters=2)
    assert st.iterations == 2
    start = R.advanced(m, out1["kf_pose"], out1["lm_pos"])
    ref = R.step(start, opts)
    assert ref["gate"] >= 1e-6, f"{name}: gate distance {ref['gate']} in iteration 2: reseed this case"
    r = R.check_iteration(ref, opts, start, out2, st.obs[1], st.cost[1], f"{name}[{variant}, it 2]", False,
                          R.C_DEV, 1e-12)
    _note(variant, name + "/it2", r)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_tiny_is_bitwise(ctx, variant):
    """dx = 0 exactly (se3_left_update's theta^2 < 1e-20 branch): nothing moves by a bit."""
    m, _, _ = R.case("tiny")
    R.reference("tiny")
    out, st = _run(ctx, "tiny", variant)
    assert st.obs[0] == 30 and st.cost[0] == 0.0
    assert np.array_equal(m["kf_pose"], out["kf_pose"]) and np.array_equal(m["lm_pos"], out["lm_pos"])


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_all_gated_stops(ctx, variant):
    """total_obs == 0 ends the run after its first iteration, whatever max_iterations says."""
    m, _, _ = R.case("all_gated")
    R.reference("all_gated")
    out, st = _run(ctx, "all_gated", variant, iters=5)
    assert st.iterations == 1 and st.obs[0] == 0 and st.cost[0] == 0.0
    assert np.array_equal(m["kf_pose"], out["kf_pose"]) and np.array_equal(m["lm_pos"], out["lm_pos"])


def test_report_device_ratio():
    """The largest multiple of the error model each variant needed in this session (DESIGN.md §2 quotes it)."""
    for variant, (ratio, name) in sorted(_worst.items()):
        print(f"{variant}: largest C = {ratio:.3g} ({name})")
    assert all(r <= R.C_DEV for r, _ in _worst.values())
