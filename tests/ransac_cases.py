"""Cases that place the two RANSAC loop replays (the one replay() of csrc/ransac_common.hpp, with one
model per hypothesis in csrc/ransac.hip and ten in csrc/essential.hip) and the essential gate (k_em_gate)
in every situation their block structure distinguishes, plus the plain references they are held to.
Shared by tests/test_ransac_replay_cpu.py and tests/test_gpu_ransac_replay.py; no GPU import.

Both uses turn RANSACPointSetRegistrator::run's sequential loop into blocks of 64 records: a prefix
max and a ballot find the entries that beat every earlier count, the ballot bits are walked in order
and each shrinks the budget (RANSACUpdateNumIters).  PnP has one record per hypothesis (block =
h // 64, lane = h % 64); the essential replay flattens (hypothesis, model) to f = 10 h + m, so the
hypotheses h with 10 h < 64 j <= 10 h + 9 (6, 12, 19, 25, ...) straddle a block boundary.

Nothing here looks at GPU output.  A case is a (builder, builder arguments, sampler seed, confidence,
H) tuple found by `reseed` (`search_*`) from the oracle's hypotheses and numpy counts; `classify_*`
names the situations a case realises and tests/test_ransac_replay_cpu.py holds every committed case
to its name ("reseed this case" when synth or the oracle change).  confidence is a double and
max_iterations an int, and both are tuned freely: confidence = 1 - (1 - w^k)^B puts the shrunk budget
of a record with inlier ratio w exactly on B.
"""
import math

import numpy as np

from vxslam import synth

M64 = (1 << 64) - 1
DBL_MIN = 2.2250738585072014e-308
BLOCK = 64          # records per replay block (one wave)
K_MODELS = 10       # essential.hip kMaxModels: record slots per hypothesis
FIRST_CHUNK = 128   # essential.hip kFirstChunk: hypotheses of the first k_em_hyp launch when gated
MAX_HYP = 4096      # kMaxHyp of both kernels


# ------------------------------------------------------------------------------------------ samplers
def mix(x):
    """splitmix64 finaliser of the oracle's counter stream (mix64)"""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def sample(seed, h, n, k):
    """the first k distinct indices of hypothesis h's 64 draws, None when there are fewer"""
    idx = []
    for a in range(64):
        i = ((mix((int(seed) + h * 64 + a) & M64) >> 32) * n) >> 32
        if i not in idx:
            idx.append(i)
        if len(idx) == k:
            return idx
    return None


def sample4(seed, h, n):
    return sample(seed, h, n, 4)


def sample5(seed, h, n):
    return sample(seed, h, n, 5)


# ------------------------------------------------------------------------------------ budget formula
def update_iters(p, ep, max_iters, points):
    """RANSACUpdateNumIters (OpenCV calib3d ptsetreg.cpp) in doubles, modelPoints = points (4 or 5)"""
    p = min(max(p, 0.0), 1.0)
    ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, DBL_MIN)
    x = 1.0 - ep
    denom = 1.0 - ((x * x) * (x * x) * x if points == 5 else (x * x) * (x * x))
    if denom < DBL_MIN:
        return 0
    num, denom = math.log(num), math.log(denom)
    return max_iters if denom >= 0 or -num >= max_iters * -denom else int(np.rint(num / denom))


def update_iters_mp(p, n, c, max_iters, points):
    """The same formula at 50 digits: (value, margin).  1 - p, ep = (n - c) / n, 1 - ep, its power
    and 1 - power are taken as the doubles every IEEE implementation computes (+ - * / only, bit
    for bit the same on the CPU and the GPU); the two logarithms, their quotient, the clamp
    comparison and the rounding are mpmath's.  margin = distance of the quotient from the nearest
    half-integer and from max_iters: while it is far above one ulp of a log, the integer does not
    depend on the last bits of any log implementation."""
    import mpmath

    with mpmath.workdps(50):
        p = min(max(float(p), 0.0), 1.0)
        ep = min(max(float(n - c) / float(n), 0.0), 1.0)
        num = max(1.0 - p, DBL_MIN)
        x = 1.0 - ep
        denom = 1.0 - ((x * x) * (x * x) * x if points == 5 else (x * x) * (x * x))
        if denom < DBL_MIN:
            return 0, math.inf
        if denom >= 1.0:
            return max_iters, math.inf
        q = mpmath.log(mpmath.mpf(num)) / mpmath.log(mpmath.mpf(denom))
        margin = min(abs(q - max_iters), abs(q - mpmath.floor(q) - mpmath.mpf(1) / 2))
        return (max_iters if q >= max_iters else int(mpmath.nint(q))), float(margin)


def update_iters_exact(p, n, c, max_iters, points):
    """The formula on the exact rational inlier ratio c / n (no double rounding anywhere but in p)"""
    import mpmath

    with mpmath.workdps(50):
        p = min(max(float(p), 0.0), 1.0)
        if c >= n:
            return 0
        if c <= 0:
            return max_iters
        num = mpmath.mpf(1) - mpmath.mpf(p) if p < 1.0 else mpmath.mpf(DBL_MIN)
        q = mpmath.log(num) / mpmath.log(1 - (mpmath.mpf(c) / n) ** points)
        return max_iters if q >= max_iters else int(mpmath.nint(q))


def confidence_for(n, c, budget, points):
    """the confidence at which a record with c of n inliers shrinks the budget to `budget` (the
    quotient lands on the integer itself, half a unit from either rounding boundary)"""
    return 1.0 - math.exp(budget * math.log1p(-(c / n) ** points))


# ------------------------------------------------------------------------------------------ builders
def low_inlier_pnp(seed, n, frac):
    """synth.make_pnp_problem with 60-75 % wrong matches: records far apart, budgets in the hundreds"""
    return synth.make_pnp_problem(seed, n, outlier_frac=frac)


def low_inlier_two_view(seed, n, frac):
    return synth.make_two_view(seed, n, outlier_frac=frac)


def _shift(rng, m):
    """m pixel shifts of 300 .. 500 px in a random direction"""
    a = rng.uniform(0, 2 * np.pi, m)
    return (rng.uniform(300, 500, m)[:, None] * np.stack([np.cos(a), np.sin(a)], -1)).astype(np.float32)


def exact_pnp(seed, n, inliers):
    """Noise-free correspondences; the rows outside `inliers` have their pixel moved by >= 300 px, so
    no pose fits them together with a true one"""
    d = synth.make_pnp_problem(seed, n, outlier_frac=0.0, noise_px=0.0)
    out = np.ones(n, bool)
    out[list(inliers)] = False
    rng = np.random.default_rng(seed + 7919)
    d["img"][out] += _shift(rng, int(out.sum()))
    d["outlier"] = out
    return d


def exact_two_view(seed, n, inliers):
    """Noise-free matches; the rows outside `inliers` have their second pixel moved by >= 300 px.  (A
    move along the epipolar line stays an inlier of the true E: the kept count is the reference's.)"""
    d = synth.make_two_view(seed, n, outlier_frac=0.0, noise_px=0.0)
    out = np.ones(n, bool)
    out[list(inliers)] = False
    rng = np.random.default_rng(seed + 7919)
    d["pts_curr"][out] += _shift(rng, int(out.sum()))
    d["outlier"] = out
    return d


def collinear_mix_pnp(seed, n, n_line):
    """make_pnp_problem whose first n_line world points lie on one line (pixels unchanged): a triple
    drawn from them gives P3P nothing, so invalid hypotheses (valid = 0) sit between valid ones"""
    d = synth.make_pnp_problem(seed, n, outlier_frac=0.3)
    d["obj"][:n_line, 0] = np.linspace(-1, 1, n_line, dtype=np.float32)
    d["obj"][:n_line, 1] = 0.0
    d["obj"][:n_line, 2] = 3.0
    return d


def planar_scene(seed, n_plane=22, n_off=6, n_wrong=12):
    """Two views of a mostly planar scene: n_plane matches on the plane (0.2, -0.1, 1) . X = 3 m, n_off
    off-plane points with z in [1.5, 6] m, n_wrong wrong matches (uniform random second pixel); no
    pixel noise, float32 pixels, rows permuted.  Five coplanar matches give the true E and its planar
    twin among the five-point solutions, and only the true one also fits the off-plane points: a later
    model of a sample often beats an earlier one."""
    rng = np.random.default_rng(seed)
    n = n_plane + n_off + n_wrong
    fx, fy, cx, cy = synth.FX, synth.FY, synth.CX, synth.CY
    uv = np.stack([rng.uniform(40, 600, n), rng.uniform(40, 440, n)], -1)
    ray = np.stack([(uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy, np.ones(n)], -1)
    z = 3.0 / (ray @ np.array([0.2, -0.1, 1.0]))
    z[n_plane:] = rng.uniform(1.5, 6.0, n - n_plane)
    rv = rng.normal(0, 1, 3)
    R = synth.quat_to_mat(synth.quat_from_rotvec(rv / np.linalg.norm(rv) * np.deg2rad(4.0)))
    t = np.array([0.2, 0.05, 0.03])
    p2 = (ray * z[:, None]) @ R.T + t
    uv2 = np.stack([fx * p2[:, 0] / p2[:, 2] + cx, fy * p2[:, 1] / p2[:, 2] + cy], -1)
    wrong = np.arange(n) >= n_plane + n_off
    uv2[wrong] = np.stack([rng.uniform(0, 640, n_wrong), rng.uniform(0, 480, n_wrong)], -1)
    perm = rng.permutation(n)
    return {"pts_last": uv[perm].astype(np.float32), "pts_curr": uv2[perm].astype(np.float32),
            "intr": np.array([fx, fy, cx, cy], np.float64), "R": R, "t": t, "outlier": wrong[perm]}


def no_baseline(seed, n):
    """the same pixels in both views: the five-point solver has no solution, nothing is ever kept"""
    d = synth.make_two_view(seed, n, outlier_frac=0.0)
    d["pts_curr"] = d["pts_last"].copy()
    return d


BUILDERS = {"low_pnp": low_inlier_pnp, "exact_pnp": exact_pnp, "collinear_pnp": collinear_mix_pnp,
            "low_2v": low_inlier_two_view, "exact_2v": exact_two_view, "planar": planar_scene,
            "no_baseline": no_baseline}


def build(case):
    """the problem of a committed case: case = (builder, builder args, sampler seed, confidence, H)"""
    return BUILDERS[case[0]](*case[1])


# ------------------------------------------------------------------------------------- count streams
def pnp_inliers(R, t, d, thr=2.0):
    pc = d["obj"].astype(np.float64) @ R.T + t
    fx, fy, cx, cy = d["intr"]
    with np.errstate(divide="ignore", invalid="ignore"):
        uv = np.stack([fx * (pc[:, 0] / pc[:, 2]) + cx, fy * (pc[:, 1] / pc[:, 2]) + cy], -1)
    e = ((uv - d["img"].astype(np.float64)) ** 2).sum(1)
    return (pc[:, 2] > 0) & (e <= thr * thr)


def pnp_stream(oracle, d, seed, length, thr=2.0):
    """count of every hypothesis 0 .. length - 1 (None: no model): the oracle's hypothesis, numpy inliers"""
    out = []
    for h in range(length):
        m = oracle.pnp_hypothesis(d["obj"], d["img"], d["intr"], int(seed), h)
        out.append(None if m is None else int(pnp_inliers(m[0], m[1], d, thr).sum()))
    return out


def normalised(d):
    fx, fy, cx, cy = d["intr"]
    p1 = d["pts_last"].astype(np.float64)
    p2 = d["pts_curr"].astype(np.float64)
    return (np.stack([(p1[:, 0] - cx) / fx, (p1[:, 1] - cy) / fy], -1),
            np.stack([(p2[:, 0] - cx) / fx, (p2[:, 1] - cy) / fy], -1))


def sampson(E, x1, x2):
    Ex1 = x1 @ E[:, :2].T + E[:, 2]
    Etx2 = x2 @ E[:2, :] + E[2, :]
    x2tEx1 = x2[:, 0] * Ex1[:, 0] + x2[:, 1] * Ex1[:, 1] + Ex1[:, 2]
    return x2tEx1 ** 2 / (Ex1[:, 0] ** 2 + Ex1[:, 1] ** 2 + Etx2[:, 0] ** 2 + Etx2[:, 1] ** 2)


def ess_stream(oracle, d, seed, length, threshold=1.0):
    """the model counts of every hypothesis 0 .. length - 1, one list per hypothesis (empty: no sample
    or no solution): numpy sampler, the oracle's five-point solver, numpy Sampson counts"""
    n = len(d["pts_last"])
    x1, x2 = normalised(d)
    thr = threshold / ((d["intr"][0] + d["intr"][1]) * 0.5)
    rows = []
    for h in range(length):
        idx = sample5(seed, h, n) if n >= 5 else None
        Es = oracle.five_point(x1[idx], x2[idx]) if idx is not None else []
        rows.append([int((sampson(E, x1, x2) <= thr * thr).sum()) for E in Es])
    return rows


# ------------------------------------------------------------------------------------ reference loops
def pnp_loop(counts, n, confidence, H):
    """RANSACPointSetRegistrator::run over a PnP count stream.  Returns (best, run, good, records):
    records = [(h, count, budget before, budget after)] of every hypothesis taken."""
    niters, best, good, h = (H if n >= 4 else 0), -1, 0, 0
    records = []
    while h < niters:
        c = counts[h]
        if c is not None and c > max(good, 3):
            before = niters
            best, good = h, c
            niters = update_iters(confidence, (n - c) / n, niters, 4)
            records.append((h, c, before, niters))
        h += 1
    return best, h, good, records


def ess_loop(rows, n, confidence, H, hlimit=None):
    """The same loop over (hypothesis, model) counts: every model of a started sample is scored.
    Returns (best (h, m) or None, run, good, records [(h, m, count, before, after)]); with hlimit, the
    loop over the first hlimit hypotheses only (what k_em_gate replays)."""
    niters, best, good, h = (H if n >= 5 else 0), None, 0, 0
    records = []
    while h < niters and (hlimit is None or h < hlimit):
        for m, c in enumerate(rows[h]):
            if c > max(good, 4):
                before = niters
                best, good = (h, m), c
                niters = update_iters(confidence, (n - c) / n, niters, 5)
                records.append((h, m, c, before, niters))
        h += 1
    return best, h, good, records


def gate_value(rows, n, confidence, H):
    """k_em_gate's result: the budget left after the first FIRST_CHUNK hypotheses, 0 when it is spent"""
    _, h, _, records = ess_loop(rows, n, confidence, H, FIRST_CHUNK)
    budget = records[-1][4] if records else (H if n >= 5 else 0)
    return budget if budget > FIRST_CHUNK else 0


def ess_block_loop(rows, n, confidence, H, fixed, hlimit=MAX_HYP):
    """ransac_common.hpp's replay() with essential.hip's ten models lane by lane on the CPU: blocks of 64 flattened records, an exclusive
    prefix max, the ballot of the entries above it, the walk over the ballot bits.  fixed=False is the
    loop as it was (it ends as soon as base >= min(budget, hlimit) * 10 and loads no entry of a
    hypothesis at or beyond the budget); fixed=True goes on while the block can still hold models of
    the last hypothesis started and loads those.  Returns (h, m, run, good, rounds, budget): budget is what
    k_em_gate reads (0 when the walk stopped at a record beyond the budget)."""
    def count(h, m):
        return rows[h][m] if h < len(rows) and m < len(rows[h]) else -1

    niters, best, good, last_h, stop, base, rounds = (H if n >= 5 else 0), -1, 0, -1, False, 0, 0
    while not stop:
        lim = min(niters, hlimit)
        if base >= (max(lim, last_h + 1) if fixed else lim) * K_MODELS:
            break
        rounds += 1
        c = []
        for lane in range(BLOCK):
            h, m = divmod(base + lane, K_MODELS)
            c.append(count(h, m) if (h < niters or (fixed and h == last_h)) and h < hlimit else -1)
        excl, bits = -1, []
        for lane in range(BLOCK):
            if c[lane] > max(excl, good, 4):
                bits.append(lane)
            excl = max(excl, c[lane])
        for k in bits:
            hk = (base + k) // K_MODELS
            if hk != last_h and hk >= niters:
                stop = True
                break
            best, last_h, good = base + k, hk, c[k]
            niters = update_iters(confidence, (n - c[k]) / n, niters, 5)
        base += BLOCK
    budget = 0 if stop else niters
    if best < 0:
        return -1, -1, niters, good, rounds, budget
    hb = best // K_MODELS
    return hb, best - hb * K_MODELS, max(niters, hb + 1), good, rounds, budget


# --------------------------------------------------------------------------------------- classifiers
PNP_TAGS = ("carry", "multi_late", "lane0", "lane63", "rec63_rec0", "tie_block", "tie_later", "run0", "run1", "run63",
            "beyond_same_max", "beyond_other_max", "beyond_same_shrink", "beyond_other_shrink",
            "last_same_max", "last_other_max", "last_same_shrink", "last_other_shrink",
            "all_low", "n4", "invalid_mix", "budget0")


def classify_pnp(counts, n, confidence, H):
    """The situations of the PnP replay that (counts, n, confidence, H) realises (counts must reach index
    H where there is one):
      carry          kept in block >= 2 with records in at least two earlier blocks
      multi_late     two or more records in one block other than block 0
      lane0, lane63  lane of the kept hypothesis (lane 0 of a block other than block 0)
      rec63_rec0     a record at lane 63 and the next record at lane 0 of the following block
      tie_block / tie_later   a later hypothesis inside the budget with the kept count, in the kept
                     hypothesis's block / in a later one (the lower index stays kept)
      run0 / run1 / run63     hypotheses_run mod 64
      beyond_{same,other}_{max,shrink}   hypothesis `budget` itself beats the kept count and is not
                     taken; it lies in the last record's block / in a block without a record; the
                     budget is max_iterations / a shrunk one
      last_{same,other}_{max,shrink}     the kept hypothesis is budget - 1 of the budget in force when
                     it was taken; the previous record lies in its block / its block has no other
                     record; that budget is max_iterations / a shrunk one
      all_low        every count <= 3: nothing kept, run = H
      n4             n = 4 and the kept count is 4
      invalid_mix    hypotheses without a model before and after a valid one inside the run
      budget0        the formula returns 0 (all inliers): run = kept + 1"""
    best, run, good, rec = pnp_loop(counts, n, confidence, H)
    tags = set()
    blocks = [r[0] // BLOCK for r in rec]
    if best < 0:
        if H > 0 and n >= 4 and run == H:
            tags.add("all_low")
        return tags
    kb = best // BLOCK
    if kb >= 2 and len({b for b in blocks if b < kb}) >= 2:
        tags.add("carry")
    if any(b >= 1 and blocks.count(b) >= 2 for b in blocks):
        tags.add("multi_late")
    if best % BLOCK == 0 and kb >= 1:
        tags.add("lane0")
    if best % BLOCK == BLOCK - 1:
        tags.add("lane63")
    if any(a[0] % BLOCK == BLOCK - 1 and b[0] == a[0] + 1 for a, b in zip(rec, rec[1:])):
        tags.add("rec63_rec0")
    for h in range(best + 1, run):
        if counts[h] == good:
            tags.add("tie_block" if h // BLOCK == kb else "tie_later")
    if run % BLOCK in (0, 1, BLOCK - 1):
        tags.add("run%d" % (run % BLOCK))
    budget = rec[-1][3]
    if budget == run and budget < len(counts) and counts[budget] is not None and counts[budget] > good:
        where = "same" if budget // BLOCK == kb else "other" if budget // BLOCK not in blocks else None
        if where:
            tags.add("beyond_%s_%s" % (where, "max" if budget == H else "shrink"))
    if best == rec[-1][2] - 1:
        prev = blocks[:-1]
        where = "same" if prev and prev[-1] == kb else "other" if kb not in prev else None
        if where:
            tags.add("last_%s_%s" % (where, "max" if rec[-1][2] == H else "shrink"))
    if n == 4 and good == 4:
        tags.add("n4")
    inv = [h for h in range(run) if counts[h] is None]
    val = [h for h in range(run) if counts[h] is not None]
    if inv and val and inv[0] < val[-1] and val[0] < inv[-1]:
        tags.add("invalid_mix")
    if good == n and run == best + 1:
        tags.add("budget0")
    return tags


ESS_TAGS = ("straddle", "straddle_left", "straddle_right", "straddle_next", "carry3", "lane0", "lane63", "tie_model",
            "tie_later", "beyond", "last", "all_low", "n5", "budget0",
            "gate0", "gate129", "gateH", "gate_stopped", "gate_edge")


def straddles(h):
    """hypothesis h's ten record slots cross a 64-record block boundary"""
    return (K_MODELS * h) // BLOCK != (K_MODELS * h + K_MODELS - 1) // BLOCK


def classify_ess(rows, n, confidence, H):
    """The situations of the essential replay and gate that (rows, n, confidence, H) realises.  "Left"
    and "right" are the two blocks a straddled hypothesis h lies in.
      straddle        a record of h on the left shrinks the budget to <= h and the kept model is a
                      strictly better one of h on the right (the case the old block loop lost)
      straddle_left   such a record on the left and the kept model, also of h, on the left too
      straddle_right  h's first record already on the right, shrinking the budget to <= h, and a
                      better model of h after it
      straddle_next   a record of h on the left shrinks the budget to <= h + 1 and a model of h + 1
                      in h's right block beats the kept count: not taken
      carry3          records in three or more blocks
      lane0, lane63   lane of the kept record (lane 0 of a block other than block 0)
      tie_model / tie_later   a later model of the kept hypothesis / of a later hypothesis inside the
                      run with the kept count
      beyond          a model of hypothesis `budget` beats the kept count: not taken
      last            the kept hypothesis is budget - 1 of the budget in force when it was started,
                      after a record of an earlier hypothesis
      all_low, n5, budget0    as for PnP (counts <= 4; n = 5; the formula returns 0)
      gate0 / gate129 / gateH / gate_stopped   after the first 128 hypotheses the budget is in
                      (run, 128] with the loop still going / 129 / H (> 128) / the loop had stopped
      gate_edge       a record in hypothesis 127 or 128 with the loop going beyond 128"""
    best, run, good, rec = ess_loop(rows, n, confidence, H)
    tags = set()
    if best is None:
        if H > 0 and n >= 5 and run == H:
            tags.add("all_low")
        return tags
    flat = [K_MODELS * r[0] + r[1] for r in rec]
    blocks = [f // BLOCK for f in flat]
    kh, km = best
    kf = K_MODELS * kh + km
    mine = [(r, f // BLOCK) for r, f in zip(rec, flat) if r[0] == kh]
    if straddles(kh):
        left, right = (K_MODELS * kh) // BLOCK, (K_MODELS * kh) // BLOCK + 1
        shrunk_left = [r for r, b in mine if b == left and r[4] <= kh and (r[0], r[1]) != best]
        if shrunk_left and kf // BLOCK == right:
            tags.add("straddle")
        if shrunk_left and kf // BLOCK == left:
            tags.add("straddle_left")
        if len(mine) >= 2 and mine[0][1] == right and mine[0][0][4] <= kh:
            tags.add("straddle_right")
        if any(b == left and r[4] <= kh + 1 for r, b in mine) and kh + 1 < len(rows) and any(
                c > good and (K_MODELS * (kh + 1) + m) // BLOCK == right for m, c in enumerate(rows[kh + 1])):
            tags.add("straddle_next")
    if len(set(blocks)) >= 3:
        tags.add("carry3")
    if kf % BLOCK == 0 and kf > 0:
        tags.add("lane0")
    if kf % BLOCK == BLOCK - 1:
        tags.add("lane63")
    if good in rows[kh][km + 1:]:
        tags.add("tie_model")
    if any(good in rows[h] for h in range(kh + 1, run)):
        tags.add("tie_later")
    budget = rec[-1][4]
    if budget == run and budget < len(rows) and any(c > good for c in rows[budget]):
        tags.add("beyond")
    started = [r for r in rec if r[0] == kh][0][3]
    if kh == started - 1 and len({r[0] for r in rec}) >= 2:
        tags.add("last")
    if n == 5 and good == 5:
        tags.add("n5")
    if good == n and run == kh + 1:
        tags.add("budget0")
    if H > FIRST_CHUNK:
        _, h128, _, rec128 = ess_loop(rows, n, confidence, H, FIRST_CHUNK)
        b128 = rec128[-1][4] if rec128 else H
        if h128 < FIRST_CHUNK:
            tags.add("gate_stopped")
        elif b128 <= FIRST_CHUNK:
            tags.add("gate0")
        elif b128 == FIRST_CHUNK + 1:
            tags.add("gate129")
        elif b128 == H:
            tags.add("gateH")
        if run > FIRST_CHUNK and any(r[0] in (FIRST_CHUNK - 1, FIRST_CHUNK) for r in rec):
            tags.add("gate_edge")
    return tags


# -------------------------------------------------------------------------------------------- search
def _prefix_records(flat_counts, floor):
    """(index, count) of the entries that beat every earlier one and `floor`"""
    out, top = [], floor
    for i, c in enumerate(flat_counts):
        if c is not None and c > top:
            out.append((i, c))
            top = c
    return out


def _candidates(pre, n, length, points, per):
    """(confidence, H) settings worth classifying for a stream whose prefix records are `pre` (index in
    records, `per` records per hypothesis): budgets placed by max_iterations and by confidence on and
    just after each record, and on the block-boundary residues after it"""
    hs = sorted({i // per for i, _ in pre})
    Hs = {h + d for h in hs for d in (0, 1)} | {length - 1}
    Hs = sorted((H for H in Hs if 0 < H < length), reverse=True)
    confs = {0.5, 0.9, 0.99, 0.999, 1.0 - 1e-12}
    for i, c in pre:
        if c >= n:
            continue
        h = i // per
        later = [j // per for j, _ in pre if j // per > h]
        targets = {t + d for t in later[:3] for d in (0, 1)}
        targets |= {b for b in range(h + 1, h + 2 * BLOCK + 2) if b % BLOCK in (0, 1, BLOCK - 1)}
        for b in targets:
            if h < b < length:
                confs.add(confidence_for(n, c, b, points))
    return [(cf, H) for cf in sorted(confs) for H in Hs if 0.0 < cf < 1.0]


def search_pnp(oracle, want, builder, args_of, scene_seeds, sampler_seeds, length=330, found=None):
    """First case of every situation in `want`: for each (scene seed, sampler seed) the count stream is
    computed once (oracle + numpy) and classified under every candidate (confidence, H).  Returns
    {tag: (builder, args, sampler seed, confidence, H)}."""
    found = {} if found is None else found
    for s in scene_seeds:
        args = args_of(s)
        d = BUILDERS[builder](*args)
        n = len(d["obj"])
        for seed in sampler_seeds:
            counts = pnp_stream(oracle, d, seed, length)
            pre = _prefix_records(counts, 3)
            for cf, H in _candidates(pre, n, length, 4, 1):
                for t in classify_pnp(counts, n, cf, H) & (set(want) - set(found)):
                    found[t] = (builder, args, seed, cf, H)
            if set(want) <= set(found):
                return found
    return found


def shift_seed(seed, k):
    """the sampler seed whose hypothesis h is hypothesis h + k of `seed` (the counter stream advances
    by 64 per hypothesis): moves any stretch of a stream to any lane"""
    return (int(seed) + 64 * k) & M64


def search_rec63_rec0(oracle, builder, args, seed, length=30000, confidence=0.99):
    """rec63_rec0 by moving a stream: two consecutive hypotheses g, g + 1 with rising counts, g beating
    the 63 hypotheses before it, put on lanes 63 and 0 by starting the stream at g - 63"""
    d = BUILDERS[builder](*args)
    n = len(d["obj"])
    c = pnp_stream(oracle, d, seed, length)
    for g in range(BLOCK - 1, length - 2 * BLOCK):
        if c[g] is not None and c[g + 1] is not None and c[g + 1] > c[g] > max(3, *(x or 0 for x in c[g - 63:g])):
            case = (builder, args, shift_seed(seed, g - 63), confidence, 2 * BLOCK)
            if "rec63_rec0" in classify_pnp(c[g - 63:g + 2 * BLOCK], n, confidence, 2 * BLOCK):
                return case
    return None


def search_ess(oracle, want, builder, args_of, scene_seeds, sampler_seeds, length=48, found=None):
    """search_pnp's counterpart over (hypothesis, model) streams"""
    found = {} if found is None else found
    for s in scene_seeds:
        args = args_of(s)
        d = BUILDERS[builder](*args)
        n = len(d["pts_last"])
        for seed in sampler_seeds:
            rows = ess_stream(oracle, d, seed, length)
            flat = [(r[m] if m < len(r) else None) for r in rows for m in range(K_MODELS)]
            pre = _prefix_records(flat, 4)
            for cf, H in _candidates(pre, n, length, 5, K_MODELS):
                for t in classify_ess(rows, n, cf, H) & (set(want) - set(found)):
                    found[t] = (builder, args, seed, cf, H)
            if set(want) <= set(found):
                return found
    return found


def search_straddles(oracle, scene_seeds=range(40), sampler_seeds=range(60), confs=(0.5, 0.9), H=40):
    """Every planar problem on which the old block loop and the sequential loop keep different models"""
    out = []
    for s in scene_seeds:
        d = planar_scene(s)
        n = len(d["pts_last"])
        for seed in sampler_seeds:
            rows = ess_stream(oracle, d, seed, H)
            for cf in confs:
                best, run, good, _ = ess_loop(rows, n, cf, H)
                if best is not None and ess_block_loop(rows, n, cf, H, False)[:4] != (best[0], best[1], run, good):
                    out.append(("planar", (s,), seed, cf, H))
    return out


def reseed(oracle, kind, tag):
    """The search that found the committed case of a situation, per situation: kind "pnp" or "ess".
    Returns the (builder, arguments, sampler seed, confidence, H) tuple to commit, or None."""
    if kind == "pnp":
        special = {"all_low": ("low_pnp", lambda s: (s, 24, 1.0), 70), "n4": ("exact_pnp", lambda s: (s, 4, (0, 1, 2, 3)), 12),
                   "budget0": ("exact_pnp", lambda s: (s, 24, tuple(range(24))), 12),
                   "invalid_mix": ("collinear_pnp", lambda s: (s, 24, 10), 70)}
        if tag == "rec63_rec0":
            return search_rec63_rec0(oracle, "low_pnp", (0, 48, 0.7), 0)
        if tag in special:
            b, args_of, length = special[tag]
            return search_pnp(oracle, [tag], b, args_of, range(3), range(5), length).get(tag)
        return search_pnp(oracle, [tag], "low_pnp", lambda s: (s, 48, 0.7), range(12), range(40)).get(tag)
    special = {"all_low": ("no_baseline", lambda s: (s, 24), 40), "n5": ("exact_2v", lambda s: (s, 5, (0, 1, 2, 3, 4)), 12),
               "budget0": ("exact_2v", lambda s: (s, 16, tuple(range(16))), 12)}
    if tag == "straddle":
        return (search_straddles(oracle) or [None])[0]
    if tag in special:
        b, args_of, length = special[tag]
        return search_ess(oracle, [tag], b, args_of, range(3), range(5), length).get(tag)
    if tag.startswith("gate"):
        return search_ess(oracle, [tag], "low_2v", lambda s: (s, 48, 0.7), range(6), range(30), 300).get(tag)
    return search_ess(oracle, [tag], "planar", lambda s: (s,), range(40), range(40)).get(tag)


# ------------------------------------------------------------------------------- budget formula sweep
SWEEP_N = range(8, 65)
SWEEP_CONFIDENCE = (0.5, 0.9, 0.99, 0.999, 0.9999)
SWEEP_H = {4: 512, 5: 256}        # max_iterations of the swept problems, per model size
SWEEP_RECORD_BYTES = {4: 104, 5: 768}  # HypRec / EmRec (csrc/ransac.hip, csrc/essential.hip)
SWEEP_CALL_BYTES = 256 << 20      # hypothesis records of one batch call stay under this
MARGIN = 1e-9


def sweep(points):
    """[(n, k, confidence, expected, margin)]: every n of SWEEP_N and confidence of SWEEP_CONFIDENCE with
    every inlier count k (points <= k <= n) whose budget formula lies below H = SWEEP_H[points], and
    the two k below the first of them (where the clamp -num >= max_iters * -denom answers);
    expected = the 50-digit formula at (n, k), margin as update_iters_mp defines it."""
    H = SWEEP_H[points]
    out = []
    for n in SWEEP_N:
        for cf in SWEEP_CONFIDENCE:
            vals = [(k,) + update_iters_mp(cf, n, k, H, points) for k in range(points, n + 1)]
            first = next(i for i, v in enumerate(vals) if v[1] < H)
            out += [(n, k, cf, e, mg) for k, e, mg in vals[max(first - 2, 0):]]
    return out


def sweep_problem(points, n, k, scene_seed, sampler_seed=0):
    """An exact problem with k of n inliers whose hypothesis 0 samples inliers only: the inlier set is
    that sample plus the lowest other rows"""
    first = sample(sampler_seed, 0, n, points)
    inl = first + [i for i in range(n) if i not in first][:k - points]
    return (exact_pnp if points == 4 else exact_two_view)(scene_seed, n, inl)


def sweep_batches(points):
    """sweep() cut into lists whose P x H hypothesis records fit SWEEP_CALL_BYTES: one batch call each"""
    rows = sweep(points)
    per = SWEEP_CALL_BYTES // (SWEEP_RECORD_BYTES[points] * SWEEP_H[points])
    return [rows[i:i + per] for i in range(0, len(rows), per)]


_SWEEP_REF = {}


def sweep_reference(oracle, points):
    """The sweep run once through the sequential reference (cached for the session):
    [(rows, args, out, mask, expected)] per batch call; args are the batch arguments, out / mask the
    oracle's results, expected[i] = the 50-digit formula at the kept count the oracle reports, or
    None where best + 1 exceeds it (the case is skipped: the run then ends at the kept hypothesis)."""
    if points in _SWEEP_REF:
        return _SWEEP_REF[points]
    H = SWEEP_H[points]
    ref = []
    for rows in sweep_batches(points):
        ps = [sweep_problem(points, n, k, n) for n, k, _, _, _ in rows]
        offs = np.cumsum([0] + [r[0] for r in rows]).astype(np.int32)
        intr = np.stack([p["intr"] for p in ps])
        if points == 4:
            opts = np.stack([oracle.pnp_options(r[0], max_iterations=H, confidence=r[2], seed=0, refine_iterations=0)
                             for r in rows])
            args = (offs, np.concatenate([p["obj"] for p in ps]), np.concatenate([p["img"] for p in ps]), intr, opts)
            out, mask = oracle.pnp_ransac_batch(*args)
            kept = out["n_inliers"]
        else:
            opts = np.stack([oracle.essential_options(max_iterations=H, confidence=r[2], seed=0) for r in rows])
            args = (offs, np.concatenate([p["pts_last"] for p in ps]), np.concatenate([p["pts_curr"] for p in ps]),
                    intr, opts)
            out, mask = oracle.essential_ransac_batch(*args)
            kept = out["n_ransac_inliers"]
        expected = []
        for r, o, g in zip(rows, out, kept):
            e = update_iters_mp(r[2], r[0], int(g), H, points)[0] if o["ok"] else None
            expected.append(e if e is not None and o["best_hypothesis"] + 1 <= e else None)
        ref.append((rows, args, out, mask, expected))
    _SWEEP_REF[points] = ref
    return ref


# ------------------------------------------------------------------------------------ committed cases
# situation -> (builder, builder arguments, sampler seed, confidence, max_iterations), found by the
# search functions above (oracle + numpy only); tests/test_ransac_replay_cpu.py checks each name.
_LOW = ("low_pnp", (0, 48, 0.7))
PNP_CASES = {
    "carry": _LOW + (1, 0.9979961629207261, 329),
    "multi_late": _LOW + (1, 0.9684133215063727, 329),
    "lane0": _LOW + (1, 0.8707210878418417, 329),
    "lane63": ("low_pnp", (1, 48, 0.7), 7, 0.137745952867107, 329),
    "rec63_rec0": _LOW + (1159936, 0.99, 128),
    "tie_block": _LOW + (0, 0.99, 329),
    "tie_later": _LOW + (0, 0.999, 329),
    "run0": _LOW + (0, 0.5484374059243364, 329),
    "run1": _LOW + (0, 0.5540122527647766, 329),
    "run63": _LOW + (0, 0.5427928734983907, 329),
    "beyond_same_max": _LOW + (0, 0.13819665655663116, 38),
    "beyond_other_max": _LOW + (0, 0.6810981296144862, 92),
    "beyond_same_shrink": _LOW + (0, 0.13819665655663116, 329),
    "beyond_other_shrink": _LOW + (0, 0.6810981296144862, 329),
    "last_same_max": _LOW + (0, 0.14156307586695682, 39),
    "last_other_max": _LOW + (0, 0.13819665655663116, 33),
    "last_same_shrink": _LOW + (0, 0.14156307586695682, 329),
    "last_other_shrink": _LOW + (0, 0.6850351897427025, 329),
    "all_low": ("low_pnp", (0, 24, 1.0), 0, 0.5, 69),
    "n4": ("exact_pnp", (0, 4, (0, 1, 2, 3)), 0, 0.5, 11),
    "invalid_mix": ("collinear_pnp", (0, 24, 10), 0, 0.9, 69),
    "budget0": ("exact_pnp", (0, 24, tuple(range(24))), 0, 0.5, 11),
}

# the planar problems on which the block loop as it was keeps another model than the sequential loop
STRADDLE_CASES = (
    ("planar", (2,), 44, 0.5, 40),
    ("planar", (31,), 5, 0.5, 40),
    ("planar", (16,), 53, 0.24791558903339017, 40),
    ("planar", (20,), 9, 0.24791558903339017, 40),
)

_GATE = ("low_2v", (0, 48, 0.7))
ESS_CASES = {
    "straddle_left": ("planar", (0,), 14, 0.02510692843927176, 47),
    "straddle_right": ("planar", (38,), 34, 0.24791558903339017, 47),
    "straddle_next": ("planar", (3,), 23, 0.01688649809314835, 47),
    "carry3": ("planar", (0,), 1, 0.9997465423814741, 47),
    "lane0": ("planar", (1,), 21, 0.9992354874190721, 47),
    "lane63": ("planar", (0,), 12, 0.43257602268427064, 47),
    "tie_model": ("planar", (0,), 0, 7.593750000001176e-05, 47),
    "tie_later": ("planar", (0,), 0, 0.99, 47),
    "beyond": ("planar", (0,), 0, 0.0001518692334960825, 47),
    "last": ("planar", (0,), 0, 0.0003282347798110319, 47),
    "all_low": ("no_baseline", (0, 24), 0, 0.5, 39),
    "n5": ("exact_2v", (0, 5, (0, 1, 2, 3, 4)), 0, 0.5, 11),
    "budget0": ("exact_2v", (0, 16, tuple(range(16))), 0, 0.5, 11),
    "gate0": _GATE + (0, 0.07774088554370129, 299),
    "gate129": _GATE + (0, 0.07832380720621746, 299),
    "gateH": _GATE + (0, 0.11822591700336915, 199),
    "gate_stopped": _GATE + (0, 1.2264330200739693e-05, 299),
    "gate_edge": _GATE + (4, 0.11841875494668941, 299),
}
