"""One LocalBA Gauss-Newton iteration in 50-digit arithmetic, and the placed windows it is asked about.

`step(m, opts)` is one iteration of LocalBA::Optimize (local_ba.cpp:110-238) as mathematics: the pose
stage (landmarks fixed), then the landmark stage on the updated poses, with the reference's
b = -J^T e sign, its +1e-6 I damping, the Huber weight and every skip rule oracle/ba_oracle.cpp
restates (feature flags, missing / bad landmark, fi >= nf, id mismatch, no camera, pc.z <= 1e-6,
|e| > max_err, the two min_* counts).  SE3::exp is the closed form (exact sin / cos, the identity at
theta = 0), the solves are plain linear solves: nothing here shares a rounding with the double-precision
restatement or the kernels.  `landmark_stage(m, poses, opts)` is the landmark stage alone from given
poses (a device's landmark update is judged from that device's own poses).

Error model of a double-precision implementation against this reference, per applied pose / landmark:

    |x - x_ref|_inf <= C * (kappa * 2^-53 * |step|_inf + 4 * 2^-53 * max(1, |x|_inf))

kappa = kappa_2 of the damped normal matrix, step = dx (6) or dp (3).  The first term is what a backward
stable solve of that system may lose; the second is the rounding of the update itself (a handful of
operations on numbers of size max(1, |x|)).  C_ORACLE is what oracle/ba_oracle.cpp needs over every
case below; the kernels get C_DEV = 16 * C_ORACLE rounded up to a power of two (reciprocals within 11
ulp, rsq within 20 ulp, unpivoted / blocked solves and tree or atomic sum orders by design).

The case builders return synth.BAMap windows of 2-6 keyframes and at most 64 landmarks, each with a
`check(ref)` that asserts on the reference that the case is what it claims (theta bin, kappa range,
counts, step applied): a reseed fails loudly instead of passing silently.
"""
import numpy as np
from mpmath import mp, mpf

from vxslam import synth

# largest C tests/test_ba_step_cpu.py measures for the restatement over all cases: 3.61 (case
# step_1e-4, a landmark whose 0.05 px residuals are rounded at 1e-16 * 300 px and whose depth is weakly
# held: the model ties the solve's loss to |step| alone), rounded up
C_ORACLE = 4.0
C_DEV = 64.0  # 16 * C_ORACLE, a power of two already
EPS = 2.0 ** -53
DELTA = 2.0 ** -20  # the placed distance from a gate (its square's distance is 2^-17 or more)

OPT_DEFAULTS = dict(window=5, iters=1, min_pose=20, min_point=2, huber=5.0, max_err=5.0)


def options(**kw):
    o = dict(OPT_DEFAULTS)
    o.update(kw)
    return o


# ------------------------------------------------------------------------------------ exact pieces
def _rot(q):
    x, y, z, w = q
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
            [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
            [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]


def _mv(M, v):
    return [sum(M[r][c] * v[c] for c in range(len(v))) for r in range(len(M))]


def _solve(H, b):
    """Gaussian elimination with partial pivoting on mpf lists."""
    n = len(b)
    A = [list(H[r]) + [b[r]] for r in range(n)]
    for k in range(n):
        p = max(range(k, n), key=lambda r: abs(A[r][k]))
        A[k], A[p] = A[p], A[k]
        for r in range(k + 1, n):
            f = A[r][k] / A[k][k]
            if f:
                for c in range(k, n + 1):
                    A[r][c] -= f * A[k][c]
    x = [mpf(0)] * n
    for r in range(n - 1, -1, -1):
        x[r] = (A[r][n] - sum(A[r][c] * x[c] for c in range(r + 1, n))) / A[r][r]
    return x


def _kappa(H):
    ev = mp.eigsy(mp.matrix(H), eigvals_only=True)
    ev = [abs(e) for e in ev]
    return float(max(ev) / min(ev))


def _exp_update(dx, q, t):
    """exp(dx) * (q, t): Sophus SE3::exp in closed form, SO3 product normalised."""
    u, w = dx[:3], dx[3:]
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    if th2 == 0:
        imag, real, c1, c2 = mpf(1) / 2, mpf(1), mpf(1) / 2, mpf(1) / 6
    else:
        th = mp.sqrt(th2)
        imag, real = mp.sin(th / 2) / th, mp.cos(th / 2)
        c1, c2 = (1 - mp.cos(th)) / th2, (th - mp.sin(th)) / (th2 * th)
    e = [imag * w[0], imag * w[1], imag * w[2], real]
    O = [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]
    O2 = [[sum(O[r][k] * O[k][c] for k in range(3)) for c in range(3)] for r in range(3)]
    V = [[(1 if r == c else 0) + c1 * O[r][c] + c2 * O2[r][c] for c in range(3)] for r in range(3)]
    ax, ay, az, aw = e
    bx, by, bz, bw = q
    qn = [aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
          aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz]
    n = mp.sqrt(sum(c * c for c in qn))
    Vu, Rt = _mv(V, u), _mv(_rot(e), t)
    return [c / n for c in qn], [Vu[i] + Rt[i] for i in range(3)], mp.sqrt(th2)


class _Track:
    def __init__(self):
        self.gate = float("inf")
        self.z = float("inf")


def _residual(q, t, R, intr, P, uv, o, tr):
    """(e, pc, |e|, weight) of one observation or None when it is skipped by pc.z or the gate."""
    pc = [R[r][0] * P[0] + R[r][1] * P[1] + R[r][2] * P[2] + t[r] for r in range(3)]
    tr.z = min(tr.z, float(abs(pc[2] - mpf(1e-6))))
    if pc[2] <= mpf(1e-6):
        return None
    fx, fy, cx, cy = intr
    e = [uv[0] - (fx * pc[0] / pc[2] + cx), uv[1] - (fy * pc[1] / pc[2] + cy)]
    en = mp.sqrt(e[0] * e[0] + e[1] * e[1])
    tr.gate = min(tr.gate, float(abs(en - o["max_err"])))
    if en > o["max_err"]:
        return None
    w = mpf(1) if en <= o["huber"] else mpf(o["huber"]) / en
    Jp = [[fx / pc[2], 0, -fx * pc[0] / (pc[2] * pc[2])], [0, fy / pc[2], -fy * pc[1] / (pc[2] * pc[2])]]
    return e, pc, w, Jp


def _select(m, o):
    ids = [int(i) for i in m["kf_id"]]
    order = sorted(range(len(ids)), key=lambda i: ids[i])
    ref = m.get("ref_kf_id")
    max_id = ids[order[-1]] if ref is None else int(ref)
    win = [i for i in reversed(order) if ids[i] <= max_id][:max(1, o["window"])][::-1]
    lm_row = {int(i): r for r, i in enumerate(m["lm_id"])}
    fp = m["kf_feat_ptr"]
    named = set()
    for k in win:
        for f in range(int(fp[k]), int(fp[k + 1])):
            if m["feat_flags"][f] & 1:
                l = lm_row.get(int(m["feat_lm_id"][f]))
                if l is not None:
                    named.add(l)
    op = m["lm_obs_ptr"]
    lms = sorted(l for l in named if not m["lm_bad"][l] and int(op[l + 1] - op[l]) >= o["min_point"])
    assert len(win) >= 2 and lms, "the window takes the reference's early return"
    return win, lm_row, lms


def _mp_rows(a):
    return [[mpf(float(x)) for x in row] for row in np.asarray(a, np.float64)]


def _pose_stage(m, o, win, lm_row, tr):
    pose, intr, P = _mp_rows(m["kf_pose"]), _mp_rows(m["kf_intr"]), _mp_rows(m["lm_pos"])
    uv, fp = m["feat_uv"].reshape(-1, 2), m["kf_feat_ptr"]
    out, cost, total = {}, mpf(0), 0
    for k in win:
        q, t = pose[k][:4], pose[k][4:]
        rec = dict(pose=q + t, dx=[mpf(0)] * 6, kappa=None, obs=0, applied=False, theta=mpf(0))
        out[k] = rec
        if not m["kf_has_cam"][k]:
            continue
        R = _rot(q)
        H = [[mpf(0)] * 6 for _ in range(6)]
        b = [mpf(0)] * 6
        for f in range(int(fp[k]), int(fp[k + 1])):
            fl = int(m["feat_flags"][f])
            if not fl & 1 or fl & 2:
                continue
            l = lm_row.get(int(m["feat_lm_id"][f]))
            if l is None or m["lm_bad"][l]:
                continue
            r = _residual(q, t, R, intr[k], P[l], [mpf(float(uv[f, 0])), mpf(float(uv[f, 1]))], o, tr)
            if r is None:
                continue
            e, pc, w, Jp = r
            S = [[1, 0, 0, 0, pc[2], -pc[1]], [0, 1, 0, -pc[2], 0, pc[0]], [0, 0, 1, pc[1], -pc[0], 0]]
            J = [[sum(Jp[a][i] * S[i][c] for i in range(3)) for c in range(6)] for a in range(2)]
            for i in range(6):
                for j in range(6):
                    H[i][j] += w * (J[0][i] * J[0][j] + J[1][i] * J[1][j])
                b[i] -= w * (J[0][i] * e[0] + J[1][i] * e[1])
            cost += w * (e[0] * e[0] + e[1] * e[1])
            rec["obs"] += 1
        total += rec["obs"]
        if rec["obs"] < o["min_pose"]:
            continue
        for i in range(6):
            H[i][i] += mpf(1e-6)
        dx = _solve(H, b)
        qn, tn, th = _exp_update(dx, q, t)
        rec.update(pose=qn + tn, dx=dx, kappa=_kappa(H), applied=True, theta=th, H=H, b=b)
    return out, cost, total


def _landmark_stage(m, o, win, lm_row, lms, pose, tr):
    intr, P = _mp_rows(m["kf_intr"]), _mp_rows(m["lm_pos"])
    uv, fp, op = m["feat_uv"].reshape(-1, 2), m["kf_feat_ptr"], m["lm_obs_ptr"]
    kf_row = {int(m["kf_id"][k]): k for k in win}
    rots = {k: _rot(pose[k][:4]) for k in win}
    out = {}
    for l in lms:
        rec = dict(pos=P[l], dp=[mpf(0)] * 3, kappa=None, obs=0, applied=False)
        out[l] = rec
        H = [[mpf(0)] * 3 for _ in range(3)]
        b = [mpf(0)] * 3
        for ob in range(int(op[l]), int(op[l + 1])):
            k = kf_row.get(int(m["obs_kf_id"][ob]))
            if k is None or not m["kf_has_cam"][k]:
                continue
            fi = int(m["obs_feat_idx"][ob])
            if fi >= int(fp[k + 1] - fp[k]):
                continue
            f = int(fp[k]) + fi
            fl = int(m["feat_flags"][f])
            if not fl & 1 or fl & 2 or int(m["feat_lm_id"][f]) != int(m["lm_id"][l]):
                continue
            R = rots[k]
            r = _residual(pose[k][:4], pose[k][4:], R, intr[k], P[l], [mpf(float(uv[f, 0])), mpf(float(uv[f, 1]))], o, tr)
            if r is None:
                continue
            e, _, w, Jp = r
            J = [[sum(Jp[a][i] * R[i][c] for i in range(3)) for c in range(3)] for a in range(2)]
            for i in range(3):
                for j in range(3):
                    H[i][j] += w * (J[0][i] * J[0][j] + J[1][i] * J[1][j])
                b[i] -= w * (J[0][i] * e[0] + J[1][i] * e[1])
            rec["obs"] += 1
        if rec["obs"] < o["min_point"]:
            continue
        for i in range(3):
            H[i][i] += mpf(1e-6)
        dp = _solve(H, b)
        rec.update(pos=[P[l][i] + dp[i] for i in range(3)], dp=dp, kappa=_kappa(H), applied=True)
    return out


def step(m, opts, dps=50):
    """One iteration.  Returns dict(win, lms, kf={row: pose, dx, kappa, obs, applied, theta, H, b},
    lm={row: pos, dp, kappa, obs, applied}, cost, obs, gate, z): `gate` / `z` are the smallest distances
    of any evaluated residual from max_err and of any depth from 1e-6."""
    with mp.workdps(dps):
        o = options(**opts)
        win, lm_row, lms = _select(m, o)
        tr = _Track()
        kf, cost, total = _pose_stage(m, o, win, lm_row, tr)
        lm = _landmark_stage(m, o, win, lm_row, lms, {k: kf[k]["pose"] for k in win}, tr)
        return dict(win=win, lms=lms, kf=kf, lm=lm, cost=cost, obs=total, gate=tr.gate, z=tr.z)


def landmark_stage(m, poses, opts, dps=50):
    """The landmark stage of step() from `poses` (n_kf x 7 doubles) and m's landmark positions."""
    with mp.workdps(dps):
        o = options(**opts)
        win, lm_row, lms = _select(m, o)
        pose = _mp_rows(np.asarray(poses, np.float64).reshape(-1, 7))
        return _landmark_stage(m, o, win, lm_row, lms, {k: pose[k] for k in win}, _Track())


def advanced(m, kf_pose, lm_pos):
    """m with another state: the start of the next iteration."""
    n = m.copy()
    n["kf_pose"] = np.ascontiguousarray(np.asarray(kf_pose, np.float64).reshape(-1, 7))
    n["lm_pos"] = np.ascontiguousarray(np.asarray(lm_pos, np.float64).reshape(-1, 3))
    return n


# ------------------------------------------------------------------------------------ comparing
def err_inf(x, x_ref):
    """|x - x_ref|_inf of doubles against mpf values, as a double."""
    with mp.workdps(60):
        return float(max(abs(mpf(float(a)) - b) for a, b in zip(x, x_ref)))


def bound(rec, key, step_key):
    """The error model's bracket for one applied record (multiply by C)."""
    st = float(max(abs(v) for v in rec[step_key]))
    xm = float(max(abs(v) for v in rec[key]))
    return rec["kappa"] * EPS * st + 4 * EPS * max(1.0, xm)


def compare_state(ref_kf, ref_lm, m0, m1, C, what):
    """m1 (an implementation's state after the iteration that started at m0) against reference
    records: applied entries within C times the model, skipped ones bitwise unchanged.  Returns the
    largest ratio error / bracket (what C = 1 would have to be)."""
    worst = 0.0
    for key, step_key, recs, a0, a1 in (("pose", "dx", ref_kf, m0["kf_pose"].reshape(-1, 7), m1["kf_pose"].reshape(-1, 7)),
                                        ("pos", "dp", ref_lm, m0["lm_pos"].reshape(-1, 3), m1["lm_pos"].reshape(-1, 3))):
        for row, rec in recs.items():
            if not rec["applied"]:
                assert np.array_equal(a0[row].view(np.uint64), a1[row].view(np.uint64)), \
                    f"{what}: skipped {key} row {row} changed: {a0[row]} -> {a1[row]}"
                continue
            moved = any(v != 0 for v in rec[step_key])
            if moved:
                assert not np.array_equal(a0[row], a1[row]), f"{what}: {key} row {row} was not updated"
            r = err_inf(a1[row], rec[key]) / bound(rec, key, step_key)
            worst = max(worst, r)
            assert r <= C, (f"{what}: {key} row {row} off by {r:.3g} x the model (C = {C}); kappa "
                            f"{rec['kappa']:.3g}, step {float(max(abs(v) for v in rec[step_key])):.3g}")
    return worst


_lm_cache = {}


def check_iteration(ref, opts, m0, m1, obs, cost, what, exact, C, cost_rtol):
    """One iteration of an implementation (state m0 -> m1, its obs and cost) against step()'s `ref`:
    identical counts and decisions, the cost exact or within cost_rtol, skipped entries bitwise, applied
    poses against ref, applied landmarks against landmark_stage() on m1's own poses.  Returns the
    largest error / bracket ratio."""
    assert obs == ref["obs"], f"{what}: obs {obs} != {ref['obs']}"
    if exact:
        assert mpf(cost) == ref["cost"], f"{what}: cost {cost!r} != {mp.nstr(ref['cost'], 20)}"
    else:
        assert abs(mpf(cost) - ref["cost"]) <= mpf(cost_rtol) * abs(ref["cost"]), \
            f"{what}: cost {cost!r} vs {mp.nstr(ref['cost'], 20)}"
    key = (m0["kf_pose"].tobytes(), m0["lm_pos"].tobytes(), m0["feat_uv"].tobytes(), m1["kf_pose"].tobytes(),
           tuple(sorted(opts.items())))
    if key not in _lm_cache:
        _lm_cache[key] = landmark_stage(m0, m1["kf_pose"], opts)
    lm = _lm_cache[key]
    for field in ("applied", "obs"):
        got, want = {l: r[field] for l, r in lm.items()}, {l: r[field] for l, r in ref["lm"].items()}
        assert got == want, f"{what}: the landmark stage decides differently from these poses ({field})"
    untouched_rows(m0, m1, ref)
    return compare_state(ref["kf"], lm, m0, m1, C, what)


def untouched_rows(m0, m1, ref):
    """Everything outside the window / the optimised set stays bitwise."""
    kp0, kp1 = m0["kf_pose"].reshape(-1, 7), m1["kf_pose"].reshape(-1, 7)
    for k in range(len(kp0)):
        if k not in ref["kf"]:
            assert np.array_equal(kp0[k], kp1[k]), f"keyframe row {k} outside the window changed"
    lp0, lp1 = m0["lm_pos"].reshape(-1, 3), m1["lm_pos"].reshape(-1, 3)
    for l in range(len(lp0)):
        if l not in ref["lm"]:
            assert np.array_equal(lp0[l], lp1[l]), f"landmark row {l} outside the optimised set changed"


# ------------------------------------------------------------------------------------ hand-built maps
class Scene:
    """Keyframes, landmarks and observations placed by hand -> synth.BAMap."""

    def __init__(self):
        self.kfs, self.lms = [], []

    def kf(self, kid, pose, intr=(synth.FX, synth.FY, synth.CX, synth.CY), cam=1):
        self.kfs.append([int(kid), np.array(pose, np.float64), np.array(intr, np.float64), cam, []])
        return len(self.kfs) - 1

    def lm(self, pos, bad=0):
        self.lms.append([1000 + 17 * len(self.lms), np.array(pos, np.float64), bad, []])
        return len(self.lms) - 1

    def see(self, l, k, uv, flags=1, lm_id=None, listed=True):
        self.kfs[k][4].append((np.array(uv, np.float64), self.lms[l][0] if lm_id is None else lm_id, flags))
        if listed:
            self.lms[l][3].append((self.kfs[k][0], len(self.kfs[k][4]) - 1))

    def build(self, window, ref_kf_id=None):
        m = synth.BAMap()
        kfs, lms = self.kfs, self.lms
        m["kf_id"] = np.array([k[0] for k in kfs], np.uint64)
        m["kf_pose"] = np.ascontiguousarray(np.stack([k[1] for k in kfs]))
        m["kf_intr"] = np.ascontiguousarray(np.stack([k[2] for k in kfs]))
        m["kf_has_cam"] = np.array([k[3] for k in kfs], np.uint8)
        cnt = np.array([len(k[4]) for k in kfs], np.int64)
        m["kf_feat_ptr"] = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        fl = [f for k in kfs for f in k[4]]
        m["feat_uv"] = np.ascontiguousarray(np.stack([f[0] for f in fl]))
        m["feat_lm_id"] = np.array([f[1] for f in fl], np.uint64)
        m["feat_flags"] = np.array([f[2] for f in fl], np.uint8)
        m["lm_id"] = np.array([x[0] for x in lms], np.uint64)
        m["lm_pos"] = np.ascontiguousarray(np.stack([x[1] for x in lms]))
        m["lm_bad"] = np.array([x[2] for x in lms], np.uint8)
        oc = np.array([len(x[3]) for x in lms], np.int64)
        m["lm_obs_ptr"] = np.concatenate([[0], np.cumsum(oc)]).astype(np.int64)
        ol = [ob for x in lms for ob in x[3]]
        m["obs_kf_id"] = np.array([ob[0] for ob in ol], np.uint64)
        m["obs_feat_idx"] = np.array([ob[1] for ob in ol], np.uint64)
        m["ref_kf_id"] = int(max(k[0] for k in kfs)) if ref_kf_id is None else int(ref_kf_id)
        m["window"] = window
        return m


def _pose_of(rotvec, centre):
    q = synth.quat_from_rotvec(np.array(rotvec, np.float64))
    return np.concatenate([q, -synth.quat_to_mat(q) @ np.array(centre, np.float64)])


def _pixel(pose, P, intr=(synth.FX, synth.FY, synth.CX, synth.CY)):
    pc = synth.quat_to_mat(pose[:4]) @ P + pose[4:]
    return np.array([intr[0] * pc[0] / pc[2] + intr[2], intr[1] * pc[1] / pc[2] + intr[3]])


def _perturbed(rng, pose, rot_deg=0.05, trans_m=0.002):
    dq = synth.quat_from_rotvec(rng.normal(0, np.deg2rad(rot_deg) / np.sqrt(3), 3))
    q = synth.quat_mul(dq, pose[:4])
    return np.concatenate([q / np.linalg.norm(q), pose[4:] + rng.normal(0, trans_m / np.sqrt(3), 3)])


def _placed(seed, centres, points, sees, *, noise_px=0.3, lm_sigma=0.002, outside=()):
    """A noisy scene: true poses at `centres` (small rotations), true `points`, keyframe k observing
    the landmarks sees[k]; stored poses and positions perturbed.  `outside`: keyframes (by index) that
    get an id below the window.  Returns (Scene, true poses) before build()."""
    rng = np.random.default_rng(seed)
    s = Scene()
    true = [_pose_of(rng.normal(0, 0.01, 3), c) for c in centres]
    for i, T in enumerate(true):
        s.kf((50 + 3 * i) if i not in outside else 10 + i, _perturbed(rng, T))
    pts = np.asarray(points, np.float64)
    for P in pts:
        s.lm(P + rng.normal(0, lm_sigma / np.sqrt(3), 3))
    for k, ls in enumerate(sees):
        for l in ls:
            s.see(l, k, _pixel(true[k], pts[l]) + np.clip(rng.normal(0, noise_px, 2), -1.0, 1.0))
    return s, true, rng


def _frustum_points(rng, n, z_lo, z_hi):
    u, v, z = rng.uniform(60, 580, n), rng.uniform(60, 420, n), rng.uniform(z_lo, z_hi, n)
    return np.stack([(u - synth.CX) / synth.FX * z, (v - synth.CY) / synth.FY * z, z], -1)


# ------------------------------------------------------------------------------------ the cases
def _all_applied(ref):
    assert all(r["applied"] for r in ref["kf"].values()), "a pose step is skipped by the reference"


def _thetas(ref):
    return sorted(float(r["theta"]) for r in ref["kf"].values() if r["applied"])


def _case_generic():
    m = synth.make_ba_map(11, 4, 120)

    def check(ref):
        _all_applied(ref)
        assert ref["gate"] >= 1e-6 and min(r["obs"] for r in ref["kf"].values()) >= 40

    return m, dict(window=4), check


# name -> (seed, rot_deg, trans_m, theta bins some keyframe's step must fall in, both sides of 0.1?,
# lm_sigma, noise_px); se3_left_update switches series at theta^2 = 1e-2 behind a wave-wide vote
STEP_CASES = {
    "step_1e-4": (40, 0.005, 1e-4, [(1e-6, 1e-3)], False, 1e-4, 0.05),
    "step_0.05": (41, 3.0, 0.02, [(0.03, 0.08)], False, 0.01, 0.5),
    "step_mixed": (44, 5.5, 0.03, [(0.08, 0.1), (0.1, 0.12)], True, 0.01, 0.5),
    "step_0.3": (40, 20.0, 0.05, [(0.2, 0.7)], False, 0.01, 0.5),
}


def _case_step(seed, rot_deg, trans_m, bins, both, lm_sigma=0.01, noise_px=0.5):
    m = synth.make_ba_map(seed, 4, 60, rot_deg=rot_deg, trans_m=trans_m, lm_sigma=lm_sigma, noise_px=noise_px,
                          frac_outlier=0.0)

    def check(ref):
        _all_applied(ref)
        th = _thetas(ref)
        for lo, hi in bins:
            assert any(lo <= t < hi for t in th), f"no step in [{lo}, {hi}): thetas {th}: reseed this case"
        if both:
            assert th[0] < 0.1 <= th[-1], f"thetas {th} are on one side of 0.1: reseed this case"
        assert ref["gate"] >= 1e-6

    return m, dict(window=4, min_pose=10, max_err=1e5, huber=1e5), check


def _case_big_step(seed, spread_px):
    """A step of theta in [1, 2.5): keyframe A sees four points within a few pixels of each other, its
    observations tens of pixels off (kept by max_err = 1e5), so the roll that fits them is large."""
    rng = np.random.default_rng(60)
    u, v = 320 + rng.uniform(-15, 15, 4), 240 + rng.uniform(-15, 15, 4)
    near = np.stack([(u - synth.CX) / synth.FX * 3.0, (v - synth.CY) / synth.FY * 3.0, np.full(4, 3.0)], -1)
    pts = np.concatenate([near, _frustum_points(rng, 6, 2.0, 4.0)])
    s, _, rg = _placed(seed, [(0, 0, 0), (0.1, 0, 0)], pts, [list(range(4)), list(range(10))])
    for i, (uv, lid, fl) in enumerate(s.kfs[0][4]):
        s.kfs[0][4][i] = (uv + rg.normal(0, spread_px, 2), lid, fl)
    m = s.build(2)

    def check(ref):
        _all_applied(ref)
        th = float(ref["kf"][0]["theta"])
        assert 1.0 <= th < 2.5, f"theta {th}: reseed this case"
        assert float(ref["kf"][1]["theta"]) < 0.1  # the vote is wave-wide: both branches in one wave

    return m, dict(window=2, min_pose=4, max_err=1e5, huber=1e5), check


def _case_half_gated():
    """About half of the observations beyond the 5 px gate, none within 1e-6 of it."""
    m = synth.make_ba_map(31, 4, 60, rot_deg=0.8, trans_m=0.02, frac_outlier=0.0)

    def check(ref):
        n = sum(1 for k in ref["win"] for f in range(int(m["kf_feat_ptr"][k]), int(m["kf_feat_ptr"][k + 1]))
                if m["feat_flags"][f] == 1)
        assert 0.25 * n <= ref["obs"] <= 0.75 * n, f"{ref['obs']} of {n} accepted: reseed this case"
        assert ref["gate"] >= 1e-6
        assert any(r["applied"] for r in ref["kf"].values())

    return m, dict(window=4, min_pose=5), check


def _ill_pose(seed, points, n_a, min_pose, kappa_lo):
    """Two keyframes 10 cm apart: B sees every point, A the first n_a of them."""
    n = len(points)
    s, _, _ = _placed(seed, [(0, 0, 0), (0.1, 0, 0)], points, [list(range(n_a)), list(range(n))])
    m = s.build(2)

    def check(ref):
        _all_applied(ref)
        a = ref["kf"][0]
        assert a["obs"] == n_a == min_pose, (a["obs"], n_a)
        assert a["kappa"] >= kappa_lo, f"kappa {a['kappa']:.3g} < {kappa_lo:.3g}"
        assert ref["gate"] >= 1e-6 and any(r["applied"] for r in ref["lm"].values())

    return m, dict(window=2, min_pose=min_pose), check


def _case_pose_obs(n_a, kappa_lo):
    pts = _frustum_points(np.random.default_rng(70 + n_a), 8, 1.5, 4.0)
    return _ill_pose(80 + n_a, pts, n_a, n_a, kappa_lo)


def _case_collinear():
    sv = np.array([0.0, 0.25, 0.45, 0.7, 0.95, 1.2])
    pts = np.array([-0.5, -0.2, 2.5])[None, :] + sv[:, None] * np.array([1.0, 0.3, 0.4])[None, :]
    return _ill_pose(91, pts, 6, 6, 1e8)


def _case_coplanar():
    rng = np.random.default_rng(92)
    x, y = rng.uniform(-0.8, 0.8, 6), rng.uniform(-0.6, 0.6, 6)
    return _ill_pose(93, np.stack([x, y, 3.0 + 0.3 * x + 0.2 * y], -1), 6, 6, 1e3)


def _case_far():
    return _ill_pose(94, _frustum_points(np.random.default_rng(95), 6, 200.0, 200.0), 6, 6, 1e7)


def _case_ill_landmarks():
    """Keyframes: 0 one metre ahead of the others, 1 and 2 one millimetre apart, 3 ten centimetres
    aside, 4 outside the window.  Landmarks 0-11 ordinary; then
      12  seen by 1 and 2 only, 50 m away (millimetre parallax)
      13  three observations, one gated out: exactly min_point accepted, moves
      14  two observations, one gated out: below min_point, stays
      15  two observations in the window and one outside it: moves on the two
      16  one observation in the window and one outside it: stays
      17  0.8 m ahead: behind keyframe 0, seen by 1 and 3: moves on the two"""
    rng0 = np.random.default_rng(96)
    pts = list(_frustum_points(rng0, 12, 2.5, 5.0))
    pts += [np.array([1.0, -0.5, 50.0]), np.array([0.2, 0.1, 3.0]), np.array([-0.3, 0.2, 3.5]),
            np.array([0.1, -0.2, 4.0]), np.array([-0.2, -0.1, 3.2]), np.array([0.02, 0.01, 0.8])]
    centres = [(0, 0, 1.0), (0, 0, 0), (0.001, 0, 0), (0.1, 0, 0), (-0.1, 0, 0)]
    base = list(range(12))
    sees = [base + [13], base + [12, 13, 14, 15, 16, 17], base + [12, 13, 14, 15], base + [17], [15, 16]]
    s, true, rng = _placed(97, centres, pts, sees, outside=(4,))
    # the gated-out observations: 40 px off
    for l, k in ((13, 0), (14, 2)):
        fi = next(i for i, f in enumerate(s.kfs[k][4]) if f[1] == s.lms[l][0])
        uv, lid, fl = s.kfs[k][4][fi]
        s.kfs[k][4][fi] = (uv + np.array([24.0, 32.0]), lid, fl)
    # behind keyframe 0: listed by the landmark, named by a feature of keyframe 0
    s.see(17, 0, [300.0, 200.0])
    m = s.build(4)

    def check(ref):
        _all_applied(ref)
        rows = {i: ref["lm"][i] for i in range(12, 18)}
        assert [rows[i]["obs"] for i in range(12, 18)] == [2, 2, 1, 2, 1, 2], [rows[i]["obs"] for i in range(12, 18)]
        assert [rows[i]["applied"] for i in range(12, 18)] == [True, True, False, True, False, True]
        assert rows[12]["kappa"] >= 1e6, rows[12]["kappa"]
        assert ref["gate"] >= 1e-6 and ref["z"] >= 0.1

    return m, dict(window=4, min_pose=8), check


# ---- exact lattice: q = (0,0,0,1), t with few mantissa bits and t.z = 0, fx = fy = 512, cx = 320,
# cy = 240, landmarks with Z a power of two and X/Z, Y/Z multiples of 1/512: pc = P + t and every
# projection is an integer pixel exactly, in any evaluation order, so a residual is exactly what is placed
LAT_INTR = (512.0, 512.0, 320.0, 240.0)
LAT_T = [(0.0, 0.0, 0.0), (-0.25, 0.0, 0.0), (0.125, -0.125, 0.0)]


def _lat_pixel(P, t):
    x, y, z = P[0] + t[0], P[1] + t[1], P[2] + t[2]
    if z <= 1e-6:  # never projected
        return np.array([320.0, 240.0])
    u, v = 512.0 * (x / z) + 320.0, 512.0 * (y / z) + 240.0
    assert u == round(u) and v == round(v) and abs(u) < 2 ** 40, (P, t, u, v)
    return np.array([u, v])


def _lattice(residuals, n_kf=2, pads=0, pad_res=(0.0, 0.0)):
    """Landmark i is seen by keyframe k with residuals[i][k] (None: not seen); `pads` more landmarks seen
    by every keyframe with pad_res.  Landmark i sits at depth residuals[i]'s optional third entry."""
    s = Scene()
    for k in range(n_kf):
        s.kf(5 + 3 * k, (0, 0, 0, 1) + LAT_T[k], LAT_INTR)
    grid = [(-64, -32), (32, 48), (96, -80), (-120, 64), (16, -96), (-48, 100), (128, 24), (-16, -8), (72, 88),
            (-100, -60), (40, -20), (-8, 72)]
    specs = list(residuals) + [dict(res=[pad_res] * n_kf) for _ in range(pads)]
    for i, sp in enumerate(specs):
        Z = sp.get("Z", 2.0 if i % 2 == 0 else 4.0)
        gx, gy = sp.get("grid", grid[i % len(grid)])
        P = np.array([gx / 512.0 * Z, gy / 512.0 * Z, Z])
        l = s.lm(P)
        for k, r in enumerate(sp["res"]):
            if r is not None:
                s.see(l, k, _lat_pixel(P, LAT_T[k]) + np.array(r, np.float64))
    return s.build(n_kf)


# landmark rows of the decision lattice
L_ON, L_OUT, L_IN, L_H1, L_H2, L_ZREJ, L_ZACC = range(7)
_DECISIONS = [
    dict(res=[(3.0, 4.0), (0.0, 5.0)]),                 # on the 5 px gate twice: kept, weight 1
    dict(res=[(3.0, 4.0), (3.0, 4.0 + DELTA)]),         # second one 2^-20 beyond 5
    dict(res=[(3.0, 4.0), (3.0, 4.0 - DELTA)]),         # second one 2^-20 inside
    dict(res=[(3.0, 4.0), (5.0, 12.0)]),                # |e| = 13
    dict(res=[(3.0, 4.0), (5.0, 12.0 + DELTA)]),        # 2^-20 beyond 13
    dict(res=[(3.0, 4.0), (0.0, 5.0)], Z=1e-6, grid=(0, 0)),       # pc.z = the double 1e-6: rejected
    dict(res=[(3.0, 4.0), (0.0, 5.0)], Z=2.0 ** -19, grid=(0, 0)),  # pc.z = 2^-19: accepted
]


def _expect_lm(ref, rows, moved, obs):
    got = [ref["lm"][r]["applied"] for r in rows]
    assert got == moved, (got, moved)
    got = [ref["lm"][r]["obs"] for r in rows]
    assert got == obs, (got, obs)


def _case_lattice_gate5():
    m = _lattice(_DECISIONS, pads=3)

    def check(ref):
        assert not any(r["applied"] for r in ref["kf"].values())
        _expect_lm(ref, range(7), [True, False, True, False, False, False, True], [2, 1, 2, 1, 1, 0, 2])
        assert [ref["kf"][k]["obs"] for k in ref["win"]] == [9, 6] and ref["obs"] == 15
        assert ref["cost"] == 225 - 8 * DELTA + DELTA * DELTA  # weight 1 everywhere; exact in any order

    return m, dict(window=2, min_pose=100), check


def _case_lattice_gate13():
    m = _lattice(_DECISIONS, pads=3)

    def check(ref):
        assert not any(r["applied"] for r in ref["kf"].values())
        _expect_lm(ref, range(7), [True, True, True, True, False, False, True], [2, 2, 2, 2, 1, 0, 2])
        assert [ref["kf"][k]["obs"] for k in ref["win"]] == [9, 8] and ref["obs"] == 17
        assert float(ref["lm"][L_H1]["kappa"]) > 0

    return m, dict(window=2, min_pose=100, huber=5.0, max_err=13.0), check


def _case_lattice_min_pose():
    """Keyframe 0 accepts exactly min_pose observations and moves; keyframe 1 has one of its own gated
    out (2^-20 beyond the gate), min_pose - 1, and stays bitwise."""
    res = [dict(res=[(1.0, -2.0), (2.0, 1.0)]), dict(res=[(-2.0, 1.0), (3.0, 4.0 + DELTA)]),
           dict(res=[(0.0, 3.0), (-1.0, -1.0)]), dict(res=[(2.0, 2.0), (1.0, -3.0)]),
           dict(res=[(-3.0, 0.0), (0.0, 2.0)]), dict(res=[(1.0, 1.0), (-2.0, -2.0)]),
           dict(res=[(2.0, 3.0), (2.0, 0.0)]), dict(res=[(0.0, -1.0), (-1.0, 3.0)])]
    m = _lattice(res)

    def check(ref):
        assert [ref["kf"][k]["obs"] for k in ref["win"]] == [8, 7]
        assert [ref["kf"][k]["applied"] for k in ref["win"]] == [True, False]
        assert all(r["applied"] for r in ref["lm"].values() if r["obs"] >= 2)

    return m, dict(window=2, min_pose=8), check


def _case_tiny():
    m = _lattice([], n_kf=3, pads=10)

    def check(ref):
        _all_applied(ref)
        assert all(r["applied"] for r in ref["lm"].values())
        assert ref["cost"] == 0 and ref["obs"] == 30
        assert all(v == 0 for r in ref["kf"].values() for v in r["dx"])
        assert all(v == 0 for r in ref["lm"].values() for v in r["dp"])

    return m, dict(window=3, min_pose=10), check


def _case_all_gated():
    m = _lattice([], n_kf=2, pads=8, pad_res=(30.0, 40.0))

    def check(ref):
        assert ref["obs"] == 0 and ref["cost"] == 0
        assert not any(r["applied"] for r in ref["kf"].values()) and not any(r["applied"] for r in ref["lm"].values())

    return m, dict(window=2, min_pose=3), check


BUILDERS = {
    "generic": _case_generic,
    "half_gated": _case_half_gated,
    "tiny": _case_tiny,
    "pose_obs1": lambda: _case_pose_obs(1, 1e10),
    "pose_obs2": lambda: _case_pose_obs(2, 1e8),
    "pose_obs3": lambda: _case_pose_obs(3, 1e2),
    "pose_collinear": _case_collinear,
    "pose_coplanar": _case_coplanar,
    "pose_far": _case_far,
    "ill_landmarks": _case_ill_landmarks,
    "lattice_gate5": _case_lattice_gate5,
    "lattice_gate13": _case_lattice_gate13,
    "lattice_min_pose": _case_lattice_min_pose,
    "all_gated": _case_all_gated,
}
for _name, _args in STEP_CASES.items():
    BUILDERS[_name] = (lambda a: lambda: _case_step(*a))(_args)
BUILDERS["step_1.5"] = lambda: _case_big_step(3, 1.0)

NAMES = list(BUILDERS)
# exact cases: every accepted residual has weight 1 and integer squares, the cost is exact in any order
EXACT_COST = ("tiny", "lattice_gate5", "lattice_min_pose", "all_gated")
# second-iteration cases (reference gate distance >= 1e-6 in both iterations)
TWO_ITER = ("generic", "step_mixed", "half_gated", "pose_obs3")

_cases, _refs = {}, {}


def case(name):
    """(map, option keywords, check) of a case, built once; the map is never modified."""
    if name not in _cases:
        _cases[name] = BUILDERS[name]()
    return _cases[name]


def reference(name):
    """step() of a case, computed once, after the case's own check on it."""
    if name not in _refs:
        m, opts, check = case(name)
        ref = step(m, opts)
        check(ref)
        _refs[name] = ref
    return _refs[name]
