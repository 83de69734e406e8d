"""One Levenberg-Marquardt iteration of the Schur-complement joint BA (vx_sba_*, csrc/sba.hip) in
50-digit arithmetic, and the placed windows it is asked about.  numpy + mpmath; the exact pieces, the
scene builder and the comparison helpers are tests/ba_step_ref.py's.

The reference is the iteration as mathematics, by the rules include/vx_slam.h and csrc/sba.hip state:
  window / landmark set   SelectKeyFrames + filter (local_ba.cpp:42-108): ba_step_ref._select
  observations            the pose stage's feature-driven set (local_ba.cpp:126-138): every flagged,
                          non-outlier feature of a window keyframe with a camera that names a good
                          landmark; optimised landmarks get a slot, the others are read from the map
  fixed keyframes         the oldest `fixed` window rows and keyframes without a camera
  per observation         e = uv - ProjectToPixel, front = pc.z > 1e-6, gate |e| > max_err, Huber weight
                          and rho, J_T = Jp [I | -hat(pc)] (2x6), J_p = Jp R (2x3)
  per optimised landmark  V = sum w J_p^T J_p, V + lam diag(V) + 1e-6 I, its inverse -- or 0 when fewer
                          than min_point observations are valid: the landmark is held -- and g_p
  reduced system          S = blockdiag(H_TT) - sum_l Y W^T, rhs = g_T - sum Y g_p (b = +J^T W e),
                          lam * diag(H_TT) + 1e-6 on the diagonal, identity rows for fixed keyframes
  cost                    sum rho over valid observations + rho(max_err) for every gated or
                          behind-camera one; the valid count
  step                    S dx = rhs by a plain solve; T <- exp(dx) T in closed form;
                          dp = V^-1 (g_p - sum over free keyframes W^T dx_k)
  decision                decide(): the LM rules in plain Python

assemble() takes the state from the map or, for a trial state, as 50-digit values.  Alongside every sum
it keeps a componentwise running-error bracket (in double: a bracket needs two digits, not fifty):

    S_ij   sum_o |w J_T^T J_T|_ij + sum_l (1 + kappa_2(V_l)) (|Y_l| |W_l^T|)_ij (+ the damping term)
    rhs_i  sum_o w |J_T^T| (|e| + |uv|) + sum_l (1 + kappa_2(V_l)) |Y_l| sum_o w |J_p^T| (|e| + |uv|)

(the residual is a rounded difference of pixel-sized numbers, so it enters as |e| + |uv|; the Schur term
passes through V^-1, hence kappa_2 of the damped V).  An implementation in double precision is held to
C * 2^-53 * bracket per entry of the lower triangle: a block 1e-6 of max|S| is judged on its own size.

Error model of the applied state, as ba_step_ref's: |x - x_ref|_inf <= C * (kappa * 2^-53 * |step|_inf
+ 4 * 2^-53 * max(1, |x|_inf)), kappa = kappa_2 of the keyframe's component of S for a pose and of the
damped V for a landmark, the reference evaluated at the implementation's own dx.

Constants (tests/test_sba_step_cpu.py measures them over every case and asserts they are the
restatement's own figures rounded up to a power of two, not guesses):
"""
import time
from fractions import Fraction

import numpy as np
from mpmath import mp, mpf

import ba_step_ref as R
from ba_step_ref import DELTA, EPS, Scene, _exp_update, _frustum_points, _mv, _perturbed, _pixel, _placed, _rot, _solve

# largest multiple of 2^-53 * bracket an entry of oracle/sba_oracle.cpp's S / rhs needs: 3.80 (case
# far_block, the (omega_z, omega_z) entry of keyframe 4's own block, whose Schur term is 1e-7 of it: the
# bracket is then sum |w J_T^T J_T| alone, and each J_T entry carries a handful of roundings; where a Schur
# term with its 1 + kappa(V) takes part the figure is 0.6 or less: step_small 0.59, fixed0 0.27), rounded
# up to a power of two
C_ORACLE_SYS = 4.0
# largest multiple of the state model its poses / landmarks need: 4.30 (case wide_kf, the worst of 280
# landmarks; lm_pack_lm's 257 need 4.23: the model ties a landmark's loss to |dp| alone), rounded up
C_ORACLE_STATE = 8.0
C_DEV_SYS = 16.0 * C_ORACLE_SYS      # reciprocals within 11 ulp, rsq within 20 ulp,
C_DEV_STATE = 16.0 * C_ORACLE_STATE  # tree and butterfly sum orders
C_SOLVE = 64.0  # |dx - dx_ref| <= C_SOLVE kappa(S) 2^-53 |dx_ref| per component, as ba_step_ref.C_DEV

K_LAMBDA_MIN = 1e-6
OPT_DEFAULTS = dict(window=5, iters=2, min_point=2, fixed=2, huber=5.0, max_err=5.0, lam=1e-4, rel_tol=1e-6)
_TRI = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


def options(**kw):
    o = dict(OPT_DEFAULTS)
    o.update(kw)
    return o


# ------------------------------------------------------------------------------------ the problem
def problem(m, o):
    """Window rows, fixed flags, optimised landmark rows and the observation list (keyframe row r of the
    window, landmark row l, slot or -1, feature index f) in keyframe-major order."""
    win, lm_row, lms = R._select(m, o)
    slot = {l: s for s, l in enumerate(lms)}
    fixed = [r < o["fixed"] or not m["kf_has_cam"][k] for r, k in enumerate(win)]
    obs, fp = [], m["kf_feat_ptr"]
    for r, k in enumerate(win):
        if not m["kf_has_cam"][k]:
            continue
        for f in range(int(fp[k]), int(fp[k + 1])):
            fl = int(m["feat_flags"][f])
            if not fl & 1 or fl & 2:
                continue
            l = lm_row.get(int(m["feat_lm_id"][f]))
            if l is None or m["lm_bad"][l]:
                continue
            obs.append((r, l, slot.get(l, -1), f))
    return win, fixed, lms, obs


def _rho_gate(o):
    d, me = mpf(o["huber"]), mpf(o["max_err"])
    return me * me if me <= d else 2 * d * me - d * d


def _sym3(t):
    return [[t[0], t[1], t[2]], [t[1], t[3], t[4]], [t[2], t[4], t[5]]]


def _kappa_np(A):
    ev = np.abs(np.linalg.eigvalsh(np.array([[float(x) for x in row] for row in A])))
    return float(ev.max() / ev.min()) if ev.min() > 0 else float("inf")


def assemble(m, opts, lam, state=None, dps=50, moved=None):
    """One assembly at the map's state (or `state` = (poses {map row: 7 mpf}, positions {map row: 3 mpf}))
    with damping lam.  Returns a dict: win, fixed, lms, obs (one record per observation), lm (one record
    per optimised landmark row), S / rhs (mpf, full symmetric n x n / n) with brackets S_br / rhs_br
    (numpy), HTT diagonal D, cost, count, gate / z (the smallest relative distances of a residual norm
    from max_err and huber and of a depth from 1e-6, the observations in `m["placed"]` left out -- at a
    trial state (`state` given, or `moved`: the map holds a state after a step) only those of them that
    cannot have moved: fixed keyframe, landmark not optimised), n_huber (valid observations with weight < 1)."""
    with mp.workdps(dps):
        o = options(**opts)
        lam = mpf(lam)
        win, fixed, lms, obs = problem(m, o)
        nk, n = len(win), 6 * len(win)
        pose = {k: [mpf(float(x)) for x in m["kf_pose"].reshape(-1, 7)[k]] for k in win}
        pos = {}
        if state is not None:
            pose.update({k: list(v) for k, v in state[0].items()})
            pos.update({l: list(v) for l, v in state[1].items()})
        placed = set(m.get("placed", ()))
        if state is not None if moved is None else moved:  # a placed residual stays placed only where nothing moves
            placed = {f for (r, l, sl, f) in obs if f in placed and fixed[r] and sl < 0}
        lmp, uvs, intr = m["lm_pos"].reshape(-1, 3), m["feat_uv"].reshape(-1, 2), m["kf_intr"].reshape(-1, 4)
        rots = {k: _rot(pose[k][:4]) for k in win}
        d_h, me, rho_g = mpf(o["huber"]), mpf(o["max_err"]), _rho_gate(o)
        H = [[[mpf(0)] * 6 for _ in range(6)] for _ in range(nk)]
        gT = [[mpf(0)] * 6 for _ in range(nk)]
        S_br, rhs_br = np.zeros((n, n)), np.zeros(n)
        cost, count, gate, zd, n_huber = mpf(0), 0, float("inf"), float("inf"), 0
        recs, per_slot = [], {l: [] for l in lms}
        for (r, l, s, f) in obs:
            k = win[r]
            q, t, Rm = pose[k][:4], pose[k][4:], rots[k]
            P = pos[l] if l in pos else [mpf(float(x)) for x in lmp[l]]
            uv = [mpf(float(uvs[f, 0])), mpf(float(uvs[f, 1]))]
            fx, fy, cx, cy = [mpf(float(x)) for x in intr[k]]
            pc = [Rm[i][0] * P[0] + Rm[i][1] * P[1] + Rm[i][2] * P[2] + t[i] for i in range(3)]
            rec = dict(r=r, l=l, slot=s, f=f, ok=False, front=pc[2] > mpf(1e-6), pc=pc)
            recs.append(rec)
            if f not in placed:
                zd = min(zd, float(abs(pc[2] - mpf(1e-6)) / mpf(1e-6)))
            if not rec["front"]:
                cost += rho_g
                continue
            e = [uv[0] - (fx * pc[0] / pc[2] + cx), uv[1] - (fy * pc[1] / pc[2] + cy)]
            en = mp.sqrt(e[0] * e[0] + e[1] * e[1])
            rec.update(e=e, en=en)
            if f not in placed:
                gate = min(gate, float(abs(en - me) / me), float(abs(en - d_h) / d_h))
            if en > me:
                cost += rho_g
                continue
            w = mpf(1) if en <= d_h else d_h / en
            n_huber += en > d_h
            cost += en * en if en <= d_h else 2 * d_h * en - d_h * d_h
            count += 1
            Jp = [[fx / pc[2], 0, -fx * pc[0] / (pc[2] * pc[2])], [0, fy / pc[2], -fy * pc[1] / (pc[2] * pc[2])]]
            Sx = [[1, 0, 0, 0, pc[2], -pc[1]], [0, 1, 0, -pc[2], 0, pc[0]], [0, 0, 1, pc[1], -pc[0], 0]]
            JT = [[sum(Jp[a][i] * Sx[i][c] for i in range(3)) for c in range(6)] for a in range(2)]
            JP = [[sum(Jp[a][i] * Rm[i][c] for i in range(3)) for c in range(3)] for a in range(2)]
            rec.update(ok=True, w=w, JT=JT, JP=JP)
            # (double copies for the brackets)
            wf, ea = float(w), [float(abs(e[a])) + abs(float(uvs[f, a])) for a in range(2)]
            JTa, JPa = np.abs(np.array(JT, float)), np.abs(np.array(JP, float))
            rec.update(ea=ea, JPa=JPa, wf=wf)
            if not fixed[r]:
                Hr, gr = H[r], gT[r]
                for i in range(6):
                    for j in range(6):
                        Hr[i][j] += w * (JT[0][i] * JT[0][j] + JT[1][i] * JT[1][j])
                    gr[i] += w * (JT[0][i] * e[0] + JT[1][i] * e[1])
                S_br[6 * r:6 * r + 6, 6 * r:6 * r + 6] += wf * (JTa.T @ JTa)
                rhs_br[6 * r:6 * r + 6] += wf * (JTa.T @ np.array(ea))
            if s >= 0:
                per_slot[l].append(rec)
        S = [[mpf(0)] * n for _ in range(n)]
        rhs = [mpf(0)] * n
        D = [mpf(0)] * n
        for r in range(nk):
            for i in range(6):
                for j in range(6):
                    S[6 * r + i][6 * r + j] = H[r][i][j]
                rhs[6 * r + i] = gT[r][i]
                D[6 * r + i] = H[r][i][i]
        lm = {}
        for l in lms:
            rs = per_slot[l]
            V = [mpf(0)] * 6
            gp = [mpf(0)] * 3
            gp_br = np.zeros(3)
            for rec in rs:
                JP, w, e = rec["JP"], rec["w"], rec["e"]
                for ti, (a, b) in enumerate(_TRI):
                    V[ti] += w * (JP[0][a] * JP[0][b] + JP[1][a] * JP[1][b])
                for a in range(3):
                    gp[a] += w * (JP[0][a] * e[0] + JP[1][a] * e[1])
                gp_br += rec["wf"] * (rec["JPa"].T @ np.array(rec["ea"]))
                rec["W"] = [[w * (rec["JT"][0][a] * JP[0][b] + rec["JT"][1][a] * JP[1][b]) for b in range(3)]
                            for a in range(6)]
            Vd = list(V)
            for ti in (0, 3, 5):
                Vd[ti] += lam * V[ti] + mpf(1e-6)
            held = len(rs) < o["min_point"]
            rec_l = dict(V=V, Vd=Vd, gp=gp, cnt=len(rs), held=held, obs=rs, kappa=_kappa_np(_sym3(Vd)), Vinv=None,
                         pos=pos[l] if l in pos else [mpf(float(x)) for x in lmp[l]])
            lm[l] = rec_l
            if held:
                continue
            Vi = mp.inverse(mp.matrix(_sym3(Vd)))
            Vi = [[Vi[i, j] for j in range(3)] for i in range(3)]
            rec_l["Vinv"] = Vi
            amp = 1.0 + rec_l["kappa"]
            free = [rec for rec in rs if not fixed[rec["r"]]]
            for rec in free:
                rec["Y"] = [_mv(Vi, row) for row in rec["W"]]  # (V^-1 symmetric: Y = W V^-1)
                rec["Ya"] = np.abs(np.array(rec["Y"], float))
                rec["Wa"] = np.abs(np.array(rec["W"], float))
            for r1 in free:
                a0 = 6 * r1["r"]
                Y1 = r1["Y"]
                for a in range(6):
                    rhs[a0 + a] -= Y1[a][0] * gp[0] + Y1[a][1] * gp[1] + Y1[a][2] * gp[2]
                rhs_br[a0:a0 + 6] += amp * (r1["Ya"] @ gp_br)
                for r2 in free:
                    b0 = 6 * r2["r"]
                    if b0 > a0:
                        continue  # (lower triangle; mirrored below)
                    W2 = r2["W"]
                    for a in range(6):
                        Sa = S[a0 + a]
                        for b in range(6):
                            Sa[b0 + b] -= Y1[a][0] * W2[b][0] + Y1[a][1] * W2[b][1] + Y1[a][2] * W2[b][2]
                    S_br[a0:a0 + 6, b0:b0 + 6] += amp * (r1["Ya"] @ r2["Wa"].T)
        for r in range(nk):
            for i in range(6):
                g = 6 * r + i
                if fixed[r]:
                    for c in range(n):
                        S[g][c] = S[c][g] = mpf(0)
                    S_br[g, :] = S_br[:, g] = 0.0
                    S[g][g], rhs[g], rhs_br[g] = mpf(1), mpf(0), 0.0
                else:
                    dmp = lam * D[g] + mpf(1e-6)
                    S[g][g] += dmp
                    S_br[g, g] += float(dmp)
        for i in range(n):
            for j in range(i + 1, n):
                S[i][j] = S[j][i]
                S_br[i, j] = S_br[j, i]
        return dict(win=win, fixed=fixed, lms=lms, obs=recs, lm=lm, S=S, rhs=rhs, S_br=S_br, rhs_br=rhs_br, D=D,
                    cost=cost, count=count, gate=gate, z=zd, n_huber=n_huber, lam=lam, opts=o, n_obs=len(recs))


def components(asm):
    """The free keyframes' covisibility components (lists of window rows), from S's block pattern."""
    nk = len(asm["win"])
    free = [r for r in range(nk) if not asm["fixed"][r]]
    label = {r: r for r in free}
    for _ in free:
        for a in free:
            for b in free:
                if b < a and any(asm["S"][6 * a + i][6 * b + j] != 0 for i in range(6) for j in range(6)):
                    label[a] = label[b] = min(label[a], label[b])
    return [[r for r in free if label[r] == c] for c in sorted(set(label.values()))]


def solve_system(S, rhs, comps, dps=50):
    """S dx = rhs per component by Gaussian elimination at `dps` digits (S, rhs: mpf or doubles; S
    symmetric or its lower triangle).  Returns (dx as mpf list, fixed rows 0; {row: kappa_2 of its
    component})."""
    with mp.workdps(dps):
        n = len(rhs)
        dx, kap = [mpf(0)] * n, {}
        for comp in comps:
            idx = [6 * r + i for r in comp for i in range(6)]
            A = [[mpf(S[max(a, b)][min(a, b)]) for b in idx] for a in idx]
            x = _solve(A, [mpf(rhs[a]) for a in idx])
            for a, v in zip(idx, x):
                dx[a] = v
            k = _kappa_np(A)
            kap.update({r: k for r in comp})
        return dx, kap


def solve(asm):
    """The reference step of an assembly: dict(dx, kappa {row: kappa_2 of its component}, comps)."""
    comps = components(asm)
    dx, kap = solve_system(asm["S"], asm["rhs"], comps)
    return dict(dx=dx, kappa=kap, comps=comps)


def trial(m, asm, dx, kappa=None, dps=50):
    """The trial state of the step dx (doubles or mpf, 6 per window row) from assembly asm: records
    shaped as ba_step_ref's (kf {map row: pose, dx, kappa, applied, theta}, lm {map row: pos, dp, kappa,
    applied}); fixed keyframes and held landmarks are not applied."""
    with mp.workdps(dps):
        dx = [mpf(float(v)) if not isinstance(v, mpf) else v for v in dx]
        kappa = kappa if kappa is not None else solve(asm)["kappa"]
        kf, lm = {}, {}
        for r, k in enumerate(asm["win"]):
            p = [mpf(float(x)) for x in m["kf_pose"].reshape(-1, 7)[k]]
            d = dx[6 * r:6 * r + 6]
            if asm["fixed"][r]:
                kf[k] = dict(pose=p, dx=[mpf(0)] * 6, kappa=None, applied=False, theta=mpf(0))
                continue
            q, t, th = _exp_update(d, p[:4], p[4:])
            kf[k] = dict(pose=q + t, dx=d, kappa=kappa[r], applied=True, theta=th)
        for l, rec in asm["lm"].items():
            if rec["held"]:
                lm[l] = dict(pos=rec["pos"], dp=[mpf(0)] * 3, kappa=None, applied=False)
                continue
            qv = list(rec["gp"])
            for ob in rec["obs"]:
                if asm["fixed"][ob["r"]]:
                    continue
                d = dx[6 * ob["r"]:6 * ob["r"] + 6]
                for c in range(3):
                    qv[c] -= sum(ob["W"][a][c] * d[a] for a in range(6))
            dp = _mv(rec["Vinv"], qv)
            lm[l] = dict(pos=[rec["pos"][i] + dp[i] for i in range(3)], dp=dp, kappa=rec["kappa"], applied=True)
        return dict(kf=kf, lm=lm)


def trial_state(tr):
    return {k: r["pose"] for k, r in tr["kf"].items()}, {l: r["pos"] for l, r in tr["lm"].items()}


def decide(prev, cost, cnt, it, o):
    """The LM rules in the header's words.  prev: None at iteration 0, else the dict this returned for
    iteration it - 1.  Returns dict(step, stop, solve, eval_trial, lam, best, accepted): step 2 initial,
    1 accepted, 0 rejected, 3 re-assembled after a reject; `solve`: this iteration factors and applies a
    step (the next assembly evaluates the trial state)."""
    if it == 0:
        nx = dict(lam=o["lam"], best=cost, accepted=0)
        step, stop = 2, False
    elif prev["eval_trial"]:
        nx = dict(prev)
        if cost < prev["best"]:
            rel = (prev["best"] - cost) / prev["best"]
            nx.update(best=cost, lam=max(prev["lam"] * 0.1, K_LAMBDA_MIN), accepted=prev["accepted"] + 1)
            step, stop = 1, rel < o["rel_tol"]
        else:
            nx.update(lam=prev["lam"] * 10.0)
            step, stop = 0, nx["lam"] > 1e12
    else:
        nx = dict(prev)
        step, stop = 3, False
    if cnt == 0:
        stop = True
    last = stop or it + 1 >= o["iters"]
    nx.update(step=step, stop=last, solve=not last and step != 0)
    nx["eval_trial"] = nx["solve"]
    return nx


def replay(costs, cnts, o):
    """decide() over a run's recorded costs and counts: the step codes, the iteration count and the
    final damping a run that saw these totals must report."""
    prev, steps = None, []
    for it, (c, n) in enumerate(zip(costs, cnts)):
        prev = decide(prev, c, n, it, o)
        steps.append(prev["step"])
        if prev["stop"]:
            break
    return steps, prev


# ------------------------------------------------------------------------------------ comparing
def compare_system(asm, S, rhs, C, what):
    """An implementation's S (lower triangle) and rhs against an assembly, per entry under
    C * 2^-53 * bracket.  Returns the largest error / (2^-53 bracket) (what C would have to be)."""
    n = len(asm["rhs"])
    worst = 0.0
    with mp.workdps(60):
        for i in range(n):
            for j in range(i + 1):
                err = float(abs(mpf(float(S[i, j])) - asm["S"][i][j]))
                br = EPS * asm["S_br"][i, j]
                if br == 0.0:
                    assert err == 0.0, f"{what}: S[{i},{j}] = {S[i, j]!r}, exactly {mp.nstr(asm['S'][i][j], 17)} expected"
                    continue
                worst = max(worst, err / br)
                assert err <= C * br, (f"{what}: S[{i},{j}] (block {i // 6},{j // 6}) = {S[i, j]!r} vs "
                                       f"{mp.nstr(asm['S'][i][j], 17)}: {err / br:.3g} x the bracket (C = {C})")
            err = float(abs(mpf(float(rhs[i])) - asm["rhs"][i]))
            br = EPS * asm["rhs_br"][i]
            if br == 0.0:
                assert err == 0.0, f"{what}: rhs[{i}] = {rhs[i]!r}, exactly 0 expected"
                continue
            worst = max(worst, err / br)
            assert err <= C * br, f"{what}: rhs[{i}] = {rhs[i]!r} vs {mp.nstr(asm['rhs'][i], 17)}: {err / br:.3g} x (C = {C})"
    return worst


def compare_step(dx, S, rhs, comps, C, what):
    """dx (doubles) against the 50-digit solve of the implementation's own S, rhs, per component:
    |dx - dx_ref|_inf <= C kappa_2 2^-53 |dx_ref|_inf, a zero reference exactly zero.  Returns the largest
    ratio."""
    ref, kap = solve_system(S, rhs, comps)
    worst = 0.0
    for comp in comps:
        idx = [6 * r + i for r in comp for i in range(6)]
        scale = float(max(abs(ref[a]) for a in idx))
        err = R.err_inf([dx[a] for a in idx], [ref[a] for a in idx])
        if scale == 0.0:
            assert err == 0.0, f"{what}: component {comp}: nonzero step for a zero right-hand side"
            continue
        r = err / (kap[comp[0]] * EPS * scale)
        worst = max(worst, r)
        assert r <= C, f"{what}: component {comp}: dx off by {r:.3g} x kappa 2^-53 |dx| (kappa {kap[comp[0]]:.3g})"
    return worst


def check_cost(cost, ref_cost, exact, what, rtol=1e-12):
    if exact:
        assert mpf(float(cost)) == ref_cost, f"{what}: cost {cost!r} != {mp.nstr(ref_cost, 20)}"
    else:
        assert abs(mpf(float(cost)) - ref_cost) <= mpf(rtol) * abs(ref_cost), f"{what}: cost {cost!r} vs {mp.nstr(ref_cost, 20)}"


def bitwise_state(m0, m1, what):
    for key in ("kf_pose", "lm_pos"):
        assert np.array_equal(np.asarray(m0[key]).view(np.uint64), np.asarray(m1[key]).view(np.uint64)), \
            f"{what}: {key} changed"


def compare_trial(tr, m0, m1, C, what):
    """m1 (the state after an accepted step from m0) against trial() at the implementation's own dx:
    applied entries within C times the model, fixed / held / pose-only / outside entries bitwise."""
    kp0, kp1 = m0["kf_pose"].reshape(-1, 7), m1["kf_pose"].reshape(-1, 7)
    lp0, lp1 = m0["lm_pos"].reshape(-1, 3), m1["lm_pos"].reshape(-1, 3)
    for k in range(len(kp0)):
        if k not in tr["kf"]:
            assert np.array_equal(kp0[k].view(np.uint64), kp1[k].view(np.uint64)), f"{what}: keyframe row {k} outside the window changed"
    for l in range(len(lp0)):
        if l not in tr["lm"]:
            assert np.array_equal(lp0[l].view(np.uint64), lp1[l].view(np.uint64)), f"{what}: landmark row {l} is not optimised and changed"
    return R.compare_state(tr["kf"], tr["lm"], m0, m1, C, what)


# ------------------------------------------------------------------------------------ placed windows
_window = _placed


def _line(n, step=0.12):
    return [(step * i, 0.01 * (i % 2), 0.0) for i in range(n)]


def _runs(rng, n_lm, n_kf, lo, hi):
    """sees[k]: landmark i is seen by a run of lo..hi consecutive keyframes."""
    sees = [[] for _ in range(n_kf)]
    for i in range(n_lm):
        c = int(rng.integers(lo, hi + 1))
        a = int(rng.integers(0, n_kf - c + 1))
        for k in range(a, a + c):
            sees[k].append(i)
    return sees


def _shift_obs(s, l, k, d):
    fi = next(i for i, f in enumerate(s.kfs[k][4]) if f[1] == s.lms[l][0])
    uv, lid, fl = s.kfs[k][4][fi]
    s.kfs[k][4][fi] = (uv + np.array(d, np.float64), lid, fl)


def _basic_checks(ref, gates=True):
    a0 = ref["asm"]
    if gates:
        assert a0["gate"] >= 1e-6 and a0["z"] >= 1e-6, (a0["gate"], a0["z"])
        if "asm1" in ref:
            assert ref["asm1"]["gate"] >= 1e-6 and ref["asm1"]["z"] >= 1e-6, (ref["asm1"]["gate"], ref["asm1"]["z"])


def _margin(ref, lo=1e-6):
    b, c = ref["asm"]["cost"], ref["asm1"]["cost"]
    assert abs(c - b) / b >= lo, f"accept / reject margin {float(abs(c - b) / b):.3g}: reseed this case"


def _accepts(ref):
    assert ref["decision"]["step"] == 1, "the reference rejects the first step: reseed this case"


def _case_generic():
    rng = np.random.default_rng(1)
    pts = _frustum_points(rng, 48, 2.0, 5.0)
    s, _, _ = _window(2, _line(6), pts, _runs(rng, 48, 6, 2, 5), noise_px=0.5)
    m = s.build(6)

    def check(ref):
        _basic_checks(ref), _margin(ref), _accepts(ref)
        a = ref["asm"]
        assert len(a["win"]) == 6 and sum(a["fixed"]) == 2 and len(a["lms"]) == 48
        assert a["n_huber"] >= 4, a["n_huber"]
        assert all(2 <= r["cnt"] <= 5 for r in a["lm"].values())

    return m, dict(window=6, huber=1.0), check


FAR_FOCAL = 0.5  # keyframe 4 of far_block: a thousandth of the others' focal length


def _case_far_block():
    """Keyframe 4 sees only the ten landmarks 200 m away, through a focal length of 0.5 px (its pixel noise
    scaled alike); every keyframe sees them, so each has five observations and a V of kappa ~ (z / baseline)^2
    at most.  Its rows of J_T scale with the focal length: its diagonal block is ~1e-6 of max|S| without any
    cancellation beyond an ordinary Schur term's, and the brackets hold it to rounding level on its own
    size (checked: bar / |entry| <= 1e-8 on its diagonal), where 1e-9 max|S| is 1e-3 of it."""
    rng = np.random.default_rng(3)
    near, far = _frustum_points(rng, 30, 2.0, 5.0), _frustum_points(rng, 10, 200.0, 200.0)
    pts = np.concatenate([near, far])
    sees = [ls + list(range(30, 40)) for ls in _runs(rng, 30, 4, 2, 4)] + [list(range(30, 40))]
    s, true, rg = _window(4, _line(5), pts, sees)
    intr4 = (FAR_FOCAL, FAR_FOCAL, R.synth.CX, R.synth.CY)
    s.kfs[4][2] = np.array(intr4, np.float64)
    feats = s.kfs[4][4]
    for i, (uv, lid, fl) in enumerate(feats):
        l = next(j for j, x in enumerate(s.lms) if x[0] == lid)
        feats[i] = (_pixel(true[4], pts[l], intr4) + rg.normal(0, 0.3, 2) * (FAR_FOCAL / R.synth.FX), lid, fl)
    m = s.build(5)

    def check(ref):
        _basic_checks(ref), _margin(ref), _accepts(ref)
        a = ref["asm"]
        assert len(a["win"]) == 5 and not a["fixed"][4] and sum(1 for o in a["obs"] if o["r"] == 4) == 10
        assert all(a["lm"][l]["cnt"] == 5 and not a["lm"][l]["held"] for l in range(30, 40))
        top = max(float(abs(v)) for row in a["S"] for v in row)
        blk = max(float(abs(a["S"][24 + i][24 + j])) for i in range(6) for j in range(6))
        assert 0 < blk <= 1e-5 * top, f"far block {blk:.3g} of max|S| {top:.3g}: reseed this case"
        rel = [C_DEV_SYS * EPS * a["S_br"][24 + i, 24 + i] / float(abs(a["S"][24 + i][24 + i])) for i in range(6)]
        assert max(rel) <= 1e-8, f"the far block's diagonal is held to {max(rel):.3g} only: reseed this case"
        assert len(ref["sol"]["comps"]) == 1  # (it shares its landmarks with keyframes 2 and 3)

    return m, dict(window=5), check


# ---- exact lattice (ba_step_ref: q = (0,0,0,1), t.z = 0, fx = fy = 512, Z a power of two): pc = P + t
# and every projection an integer pixel exactly, so a residual is exactly what is placed
def _lat_scene(specs, n_kf=3, pads=0, pad_res=(0.0, 0.0)):
    """R._lattice's rule on a Scene that is returned unbuilt, with the features of placed residuals."""
    s = Scene()
    for k in range(n_kf):
        s.kf(5 + 3 * k, (0, 0, 0, 1) + R.LAT_T[k], R.LAT_INTR)
    grid = [(-64, -32), (32, 48), (96, -80), (-120, 64), (16, -96), (-48, 100), (128, 24), (-16, -8), (72, 88),
            (-100, -60), (40, -20), (-8, 72)]
    specs = list(specs) + [dict(res=[pad_res] * n_kf) for _ in range(pads)]
    for i, sp in enumerate(specs):
        Z = sp.get("Z", 2.0 if i % 2 == 0 else 4.0)
        gx, gy = sp.get("grid", grid[i % len(grid)])
        P = np.array([gx / 512.0 * Z, gy / 512.0 * Z, Z])
        l = s.lm(P)
        for k, r in enumerate(sp["res"]):
            if r is not None:
                s.see(l, k, R._lat_pixel(P, R.LAT_T[k]) + np.array(r, np.float64))
    return s


_GATE_ROWS = [
    dict(res=[(3.0, 4.0), (0.0, 5.0), (4.0, 3.0)]),               # on the gate three times
    dict(res=[(3.0, 4.0), (3.0, 4.0 + DELTA), (1.0, 1.0)]),       # 2^-20 beyond 5
    dict(res=[(3.0, 4.0), (3.0, 4.0 - DELTA), (1.0, -1.0)]),      # 2^-20 inside
    dict(res=[(3.0, 4.0), (5.0, 12.0), (-1.0, 2.0)]),             # |e| = 13
    dict(res=[(3.0, 4.0), (5.0, 12.0 + DELTA), (2.0, -1.0)]),     # 2^-20 beyond 13
    dict(res=[(3.0, 4.0), (5.0, 12.0 - DELTA), (0.0, 2.0)]),      # 2^-20 inside 13
]


def _lattice_gate(max_err, counts, n_valid, huber=None, n_huber=0):
    huber = max_err if huber is None else huber
    s = _lat_scene(_GATE_ROWS, pads=4, pad_res=(1.0, -2.0))
    m = s.build(3)
    m["placed"] = [f for f in range(len(m["feat_uv"]))
                   if any(abs(abs(complex(*r)) - g) < 1e-3 for g in (5.0, 13.0)
                          for r in [_lat_res(m, f)])]

    def check(ref):
        _basic_checks(ref), _margin(ref)
        a = ref["asm"]
        assert [a["lm"][l]["cnt"] for l in range(6)] == counts, [a["lm"][l]["cnt"] for l in range(6)]
        assert a["count"] == n_valid and a["n_obs"] == 30
        # huber == max_err: weight 1 everywhere, the cost exact in any order; huber = 5 below max_err = 13:
        # |e| = 5 on the Huber switch with weight 1, 2^-20 beyond it and the 13s with weight 5 / |e|
        assert a["n_huber"] == n_huber, a["n_huber"]
        assert len(m["placed"]) >= 9

    return m, dict(window=3, fixed=1, huber=huber, max_err=max_err), check


def _lat_res(m, f):
    """The residual placed on feature f of a lattice map (exact: integers and multiples of 2^-20)."""
    k = int(np.searchsorted(m["kf_feat_ptr"], f, side="right") - 1)
    l = int(np.nonzero(m["lm_id"] == m["feat_lm_id"][f])[0][0])
    P, t = m["lm_pos"].reshape(-1, 3)[l], m["kf_pose"].reshape(-1, 7)[k][4:]
    if P[2] + t[2] <= 1e-6:
        return (0.0, 0.0)
    fx, fy, cx, cy = m["kf_intr"].reshape(-1, 4)[k]
    x, y, z = (Fraction(float(P[i])) + Fraction(float(t[i])) for i in range(3))
    u, v = Fraction(float(fx)) * x / z + Fraction(float(cx)), Fraction(float(fy)) * y / z + Fraction(float(cy))
    uv = m["feat_uv"].reshape(-1, 2)[f]
    return (float(Fraction(float(uv[0])) - u), float(Fraction(float(uv[1])) - v))


def _case_depth_gate():
    """Four landmarks on the optical axis of the fixed keyframe 0 (t = 0: pc.z = Z exactly), one observation
    each (pose-stage only), residual (3, 4) where it projects: Z = the double 1e-6 (not in front), one ulp
    above (counted), one ulp below, and one metre behind.  This places `front`, the count and rho_gate in
    k_sba_blocks; a depth-gated observation of a free keyframe on an optimised landmark (the agreement of
    `ok` between k_sba_lm and k_sba_blocks on `front`) is not placed: one ulp in front its J_T is 5e8."""
    zs = [1e-6, float(np.nextafter(1e-6, 1.0)), float(np.nextafter(1e-6, 0.0)), -1.0]
    specs = [dict(res=[(3.0, 4.0), None, None], Z=z, grid=(0, 0)) for z in zs]
    s = _lat_scene(specs, pads=6, pad_res=(1.0, 1.0))
    m = s.build(3)
    m["placed"] = [0, 1, 2, 3]  # (keyframe 0's first four features)

    def check(ref):
        _basic_checks(ref), _margin(ref)
        a = ref["asm"]
        assert [(o["front"], o["ok"]) for o in a["obs"][:4]] == [(False, False), (True, True), (False, False), (False, False)]
        assert a["obs"][1]["en"] == 5 and a["n_obs"] == 22 and a["count"] == 19
        assert a["cost"] == 3 * 25 + 25 + 18 * 2
        assert len(a["lms"]) == 6  # the four are pose-stage only

    return m, dict(window=3, fixed=1), check


def _case_held_landmark():
    """Landmarks 0-2 have two observations, one of them 40 px off (gated); landmark 3 has three, two of
    them gated: min_point - 1 valid ones each."""
    rng = np.random.default_rng(5)
    pts = _frustum_points(rng, 24, 2.0, 5.0)
    sees = _runs(rng, 24, 5, 3, 5)
    for k in range(5):
        sees[k] = [i for i in sees[k] if i > 3]
    for i, ks in ((0, (2, 3)), (1, (2, 3)), (2, (3, 4)), (3, (2, 3, 4))):
        for k in ks:
            sees[k].append(i)
    s, _, _ = _window(6, _line(5), pts, sees)
    for l, k in ((0, 3), (1, 2), (2, 3), (3, 3), (3, 4)):
        _shift_obs(s, l, k, (24.0, 32.0))
    m = s.build(5)

    def check(ref):
        _basic_checks(ref), _margin(ref), _accepts(ref)
        a = ref["asm"]
        assert [a["lm"][l]["cnt"] for l in range(4)] == [1, 1, 1, 1]
        assert [l for l, r in a["lm"].items() if r["held"]] == [0, 1, 2, 3]
        # their valid observations are in free keyframes: still in H_TT
        assert all(not a["fixed"][o["r"]] for l in range(4) for o in a["lm"][l]["obs"])
        assert ref["asm1"]["lm"][0]["held"]

    return m, dict(window=5), check


def _case_pose_only():
    """Landmarks 0-3 are seen by one keyframe only (below min_point in the map: slots >= n_opt, read from
    the map's positions); landmarks 4-5 by the two fixed keyframes and the free keyframe 3."""
    rng = np.random.default_rng(7)
    pts = _frustum_points(rng, 26, 2.0, 5.0)
    sees = _runs(rng, 26, 5, 3, 5)
    for k in range(5):
        sees[k] = [i for i in sees[k] if i > 5]
    for i, k in ((0, 2), (1, 3), (2, 4), (3, 0)):
        sees[k].append(i)
    for i in (4, 5):
        for k in (0, 1, 3):
            sees[k].append(i)
    s, _, _ = _window(8, _line(5), pts, sees)
    m = s.build(5)

    def check(ref):
        _basic_checks(ref), _margin(ref), _accepts(ref)
        a = ref["asm"]
        assert a["lms"] == list(range(4, 26))
        assert sorted(o["l"] for o in a["obs"] if o["slot"] < 0) == [0, 1, 2, 3] and all(o["ok"] for o in a["obs"])
        assert [sorted(o["r"] for o in a["lm"][l]["obs"]) for l in (4, 5)] == [[0, 1, 3]] * 2

    return m, dict(window=5), check


def _case_dead_kf():
    """Every observation of the free keyframe 3 is 40 px off."""
    rng = np.random.default_rng(9)
    pts = _frustum_points(rng, 24, 2.0, 5.0)
    sees = _runs(rng, 24, 5, 3, 5)
    s, _, _ = _window(10, _line(5), pts, sees)
    for l in sees[3]:
        _shift_obs(s, l, 3, (-32.0, 24.0))
    m = s.build(5)

    def check(ref):
        _basic_checks(ref), _margin(ref), _accepts(ref)
        a = ref["asm"]
        assert len(sees[3]) >= 8 and not any(o["ok"] for o in a["obs"] if o["r"] == 3)
        assert all(a["S"][18 + i][j] == (mpf(1e-6) if j == 18 + i else 0) for i in range(6) for j in range(30))
        assert all(v == 0 for v in a["rhs"][18:24]) and all(v == 0 for v in ref["sol"]["dx"][18:24])

    return m, dict(window=5), check


def _case_fixed(fixed, lam, seed):
    rng = np.random.default_rng(seed)
    pts = _frustum_points(rng, 30, 2.0, 5.0)
    s, _, _ = _window(seed + 1, _line(5), pts, _runs(rng, 30, 5, 2, 5))
    m = s.build(5)

    def check(ref):
        _basic_checks(ref), _margin(ref), _accepts(ref)
        assert sum(ref["asm"]["fixed"]) == fixed and len(ref["sol"]["comps"]) == 1

    return m, dict(window=5, fixed=fixed, lam=lam), check


def _case_lm_pack_obs():
    """63 landmarks of 4 observations (252), then one of 5 (the workgroup is cut one landmark early, at
    252 observations), then 6 more of 4: 281 optimised observations."""
    rng = np.random.default_rng(13)
    pts = _frustum_points(rng, 70, 2.5, 5.0)
    sees = [[] for _ in range(5)]
    for i in range(70):
        ks = range(5) if i == 63 else [k for k in range(5) if k != i % 5]
        for k in ks:
            sees[k].append(i)
    s, _, _ = _window(14, _line(5, 0.08), pts, sees)
    m = s.build(5)

    def check(ref):
        _basic_checks(ref), _margin(ref), _accepts(ref)
        cnt = [len([o for o in ref["asm"]["obs"] if o["l"] == l]) for l in ref["asm"]["lms"]]
        assert cnt == [4] * 63 + [5] + [4] * 6 and 257 <= sum(cnt) <= 300
        assert sum(cnt[:63]) == 252 and sum(cnt[:64]) > 256

    return m, dict(window=5), check


def _case_lm_pack_lm():
    """257 landmarks of 2 observations in 3 keyframes: the landmark-count limit, not the observation one."""
    rng = np.random.default_rng(15)
    pts = _frustum_points(rng, 257, 2.5, 5.0)
    sees = [[] for _ in range(3)]
    for i in range(257):
        for k in [k for k in range(3) if k != i % 3]:
            sees[k].append(i)
    s, _, _ = _window(16, _line(3, 0.15), pts, sees)
    m = s.build(3)

    def check(ref):
        _basic_checks(ref), _margin(ref), _accepts(ref)
        assert len(ref["asm"]["lms"]) == 257 and all(r["cnt"] == 2 for r in ref["asm"]["lm"].values())

    return m, dict(window=3, fixed=1), check


def _case_wide_kf():
    """The free keyframe 2 sees 280 landmarks (as many self pairs): two strides of 256 at one workgroup
    per diagonal block, parts 2.. empty when the block is split over 3 or 8."""
    rng = np.random.default_rng(17)
    pts = _frustum_points(rng, 280, 2.5, 5.0)
    sees = [[], [], list(range(280)), []]
    for i in range(280):
        sees[(0, 1, 3)[i % 3]].append(i)
    s, _, _ = _window(18, _line(4, 0.1), pts, sees)
    m = s.build(4)

    def check(ref):
        _basic_checks(ref), _margin(ref), _accepts(ref)
        n2 = sum(1 for o in ref["asm"]["obs"] if o["r"] == 2)
        assert 257 <= n2 <= 300 and not ref["asm"]["fixed"][2], n2

    return m, dict(window=4), check


def _case_ill_landmark():
    """Landmarks 0-2 are seen only by the fixed keyframes 0 and 1, one millimetre apart and stored as they
    truly are, from 20 m and near their optical axes (so lam diag(V) adds next to nothing along the ray),
    their pixels 0.01 px off: a step of metres along the ray that the cost still accepts."""
    rng = np.random.default_rng(19)
    axis = np.array([[-0.4, 0.25, 20.0], [0.0, -0.2, 20.0], [0.5, 0.1, 20.0]])
    pts = np.concatenate([axis, _frustum_points(rng, 24, 2.0, 5.0)])
    sees = [[i + 3 for i in ls] for ls in _runs(rng, 24, 5, 3, 5)]
    sees[0] += [0, 1, 2]
    sees[1] += [0, 1, 2]
    centres = [(0, 0, 0), (0.001, 0, 0), (0.12, 0.01, 0), (0.24, 0, 0), (0.36, 0, 0)]
    s, true, rg = _window(20, centres, pts, sees)
    for k in (0, 1):
        s.kfs[k][1] = true[k].copy()
        feats = s.kfs[k][4]
        for i, (uv, lid, fl) in enumerate(feats):
            l = next(j for j, x in enumerate(s.lms) if x[0] == lid)
            if l < 3:
                feats[i] = (_pixel(true[k], pts[l]) + rg.normal(0, 0.01, 2), lid, fl)
    m = s.build(5)

    def check(ref):
        _basic_checks(ref), _margin(ref), _accepts(ref)
        a = ref["asm"]
        for l in range(3):
            assert a["lm"][l]["cnt"] == 2 and not a["lm"][l]["held"]
            assert a["lm"][l]["kappa"] >= 1e8, f"kappa(V) {a['lm'][l]['kappa']:.3g}: reseed this case"
            assert max(abs(v) for v in ref["trial"]["lm"][l]["dp"]) > 0.01

    return m, dict(window=5, lam=1e-6), check


def _thetas(ref):
    a = ref["asm"]
    return {r: float(mp.sqrt(sum(v * v for v in ref["sol"]["dx"][6 * r + 3:6 * r + 6])))
            for r in range(len(a["win"])) if not a["fixed"][r]}


def _case_step_small():
    """Keyframe 4 and the landmarks 0-11 it shares with the fixed keyframes alone are stored as they truly
    are, their pixels 1e-8 px off: its step has 0 < theta^2 < 1e-20 (se3_left_update's first branch), in a
    component of its own; keyframes 2 and 3 take ordinary steps (theta < 0.1)."""
    rng = np.random.default_rng(21)
    pts = _frustum_points(rng, 36, 2.0, 5.0)
    sees = [[i + 12 for i in ls] for ls in _runs(rng, 24, 4, 3, 4)] + [[]]
    for k in (0, 1, 4):
        sees[k] += list(range(12))
    s, true, rg = _window(22, _line(5), pts, sees)
    for k in (0, 1, 4):
        s.kfs[k][1] = true[k].copy()
        feats = s.kfs[k][4]
        for i, (uv, lid, fl) in enumerate(feats):
            l = next(j for j, x in enumerate(s.lms) if x[0] == lid)
            if l < 12:
                feats[i] = (_pixel(true[k], pts[l]) + rg.normal(0, 1e-8, 2), lid, fl)
    for l in range(12):
        s.lms[l][1] = pts[l].copy()
    m = s.build(5)

    def check(ref):
        _basic_checks(ref), _margin(ref), _accepts(ref)
        th = _thetas(ref)
        assert 0 < th[4] ** 2 < 1e-20, f"theta^2 {th[4] ** 2:.3g}: reseed this case"
        assert all(1e-6 < th[r] < 0.1 for r in (2, 3)), th
        assert [4] in ref["sol"]["comps"]

    return m, dict(window=5), check


def _case_step_large():
    """Free keyframes stored 8, 12 and 18 degrees off: steps with theta between 0.1 and about 1."""
    rng = np.random.default_rng(23)
    pts = _frustum_points(rng, 30, 2.0, 5.0)
    s, true, rg = _window(24, _line(5), pts, _runs(rng, 30, 5, 3, 5), lm_sigma=0.01)
    for k, deg in ((2, 8.0), (3, 12.0), (4, 18.0)):
        s.kfs[k][1] = _perturbed(rg, true[k], rot_deg=deg, trans_m=0.03)
    m = s.build(5)

    def check(ref):
        _basic_checks(ref), _margin(ref), _accepts(ref)
        th = _thetas(ref)
        assert all(0.1 < t < 1.2 for t in th.values()), f"thetas {th}: reseed this case"

    return m, dict(window=5, huber=1e5, max_err=1e5), check


def _case_zero_cost():
    s = _lat_scene([], pads=10)
    m = s.build(3)

    def check(ref):
        _basic_checks(ref)
        a = ref["asm"]
        assert a["cost"] == 0 and a["count"] == 30 and all(v == 0 for v in a["rhs"])
        assert all(v == 0 for v in ref["sol"]["dx"])
        assert ref["asm1"]["cost"] == 0 and ref["decision"]["step"] == 0  # not below the best cost: rejected

    return m, dict(window=3, fixed=1), check


def _case_reject():
    """Free keyframes 60, 70 and 80 degrees and 0.3 m off, lam = 1e-9: the undamped step overshoots."""
    rng = np.random.default_rng(27)
    pts = _frustum_points(rng, 30, 2.0, 5.0)
    s, true, rg = _window(28, _line(5), pts, _runs(rng, 30, 5, 3, 5), lm_sigma=0.05)
    for k, deg in ((2, 60.0), (3, 70.0), (4, 80.0)):
        s.kfs[k][1] = _perturbed(rg, true[k], rot_deg=deg, trans_m=0.3)
    m = s.build(5)

    def check(ref):
        _basic_checks(ref), _margin(ref, 1e-3)
        assert ref["decision"]["step"] == 0, "the reference accepts: reseed this case"

    return m, dict(window=5, lam=1e-9, huber=5.0, max_err=1e5), check


def _case_all_gated():
    s = _lat_scene([], pads=8, pad_res=(30.0, 40.0))
    m = s.build(3)

    def check(ref):
        a = ref["asm"]
        assert a["count"] == 0 and a["n_obs"] == 24 and a["cost"] == 24 * 25
        assert ref["decision"]["stop"] and "asm1" not in ref

    return m, dict(window=3, fixed=1), check


BUILDERS = {
    "generic": _case_generic,
    "far_block": _case_far_block,
    "lattice_gate5": lambda: _lattice_gate(5.0, [3, 2, 3, 2, 2, 2], 26),
    "lattice_gate13": lambda: _lattice_gate(13.0, [3, 3, 3, 3, 2, 3], 29),
    "lattice_huber": lambda: _lattice_gate(13.0, [3, 3, 3, 3, 2, 3], 29, huber=5.0, n_huber=3),
    "depth_gate": _case_depth_gate,
    "held_landmark": _case_held_landmark,
    "pose_only": _case_pose_only,
    "dead_kf": _case_dead_kf,
    "fixed0": lambda: _case_fixed(0, 1e-2, 11),
    "fixed3": lambda: _case_fixed(3, 1e-4, 31),
    "lm_pack_obs": _case_lm_pack_obs,
    "lm_pack_lm": _case_lm_pack_lm,
    "wide_kf": _case_wide_kf,
    "ill_landmark": _case_ill_landmark,
    "step_small": _case_step_small,
    "step_large": _case_step_large,
    "zero_cost": _case_zero_cost,
    "reject": _case_reject,
    "all_gated": _case_all_gated,
}
NAMES = list(BUILDERS)
# weight 1 everywhere and residual squares that sum exactly in any order: the cost is exact
EXACT_COST = ("lattice_gate5", "lattice_gate13", "depth_gate", "zero_cost", "all_gated")

_cases, _refs = {}, {}
ref_seconds = {}


def case(name):
    """(map, option keywords, check) of a case, built once; the map is never modified."""
    if name not in _cases:
        _cases[name] = BUILDERS[name]()
    return _cases[name]


def reference(name):
    """One iteration of a case, computed once, after the case's own check on it: dict(asm, sol, trial,
    asm1 (the assembly at the trial state; absent when the run stops at iteration 0), decision (of
    iteration 1), d0 (of iteration 0))."""
    if name not in _refs:
        t0 = time.perf_counter()
        m, kw, check = case(name)
        o = options(**kw)
        asm = assemble(m, kw, o["lam"])
        sol = solve(asm)
        ref = dict(asm=asm, sol=sol, opts=o)
        with mp.workdps(50):
            d0 = decide(None, asm["cost"], asm["count"], 0, o)
            ref["d0"] = d0
            if d0["solve"]:
                tr = trial(m, asm, sol["dx"], sol["kappa"])
                asm1 = assemble(m, kw, o["lam"], state=trial_state(tr))
                ref.update(trial=tr, asm1=asm1, decision=decide(d0, asm1["cost"], asm1["count"], 1, o))
            else:
                ref["decision"] = d0
        check(ref)
        ref_seconds[name] = time.perf_counter() - t0
        _refs[name] = ref
    return _refs[name]
