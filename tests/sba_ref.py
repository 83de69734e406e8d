"""Inputs and the high-precision reference for the tests of the Schur BA's dense pose solve
(tests/test_sba_solve_cpu.py, tests/test_gpu_sba_solve.py).  numpy only.

synth.make_ba_map's covisibility is a clean band (each landmark seen by 2-5 consecutive keyframes),
so at 16 x 16 tile granularity its factor has no fill and its windows never fall into unequal
components.  The helpers here edit a returned map (no generator draw of make_ba_map changes) into
the shapes a real map has: a loop closure (close_loop), a window of two components of chosen sizes
(split_window).  solve_ext is a plain Cholesky in np.longdouble (x87 80-bit), the reference the
solve's output dx is compared with; check_solution holds the two bars.

The bars, per connected component of n rows (a small component's error cannot hide behind a large one),
residuals in longdouble:
  backward  |S dx - rhs|_inf / (|S|_inf |dx|_inf + |rhs|_inf) <= (3 n + 1) 2^-53
            the first-order bound of a Cholesky solve in FP64 (Higham, Accuracy and Stability of
            Numerical Algorithms, thm 10.4: |dA| <= gamma_(3n+1) |L||L^T|, and | |L||L^T| |_2 <=
            n |A|_2), a cap no correct FP64 factorisation exceeds
  forward   max|dx - x_ext| / max|x_ext| <= 16 max(e64, n 2^-53)
            e64: the same quantity for numpy.linalg.solve on the same S and rhs.  The tiled
            right-looking factor is in LAPACK's error class (n eps cond); its four-wide MFMA k-slices
            and refined pivot reciprocals cost a constant factor, not an order of magnitude.
A component whose reference solution is exactly zero (no rhs) must come back exactly zero.
"""
import functools

import numpy as np

from vxslam import synth

EPS64 = 2.0 ** -53
FWD_FACTOR = 16.0
SEED = 900


# --------------------------------------------------------------------------- map edits
def _kf_rows_of_landmarks(m):
    """per landmark index: the sorted keyframe rows that hold it, by the keyframes' features
    (feat_flags & 1) and by the landmark's own observation list"""
    row_of = {int(k): r for r, k in enumerate(m["kf_id"])}
    lm_of = {int(v): i for i, v in enumerate(m["lm_id"])}
    rows = [set() for _ in range(len(m["lm_id"]))]
    fp = m["kf_feat_ptr"]
    for r in range(len(m["kf_id"])):
        for f in range(int(fp[r]), int(fp[r + 1])):
            if m["feat_flags"][f] & 1:
                l = lm_of.get(int(m["feat_lm_id"][f]))
                if l is not None:
                    rows[l].add(r)
    for l in range(len(rows)):
        for o in range(int(m["lm_obs_ptr"][l]), int(m["lm_obs_ptr"][l + 1])):
            rows[l].add(row_of[int(m["obs_kf_id"][o])])
    return [sorted(s) for s in rows]


def split_window(m, after_kf):
    """lm_bad on every landmark held on both sides of the boundary after keyframe row `after_kf`:
    rows <= after_kf and rows > after_kf share no landmark afterwards.  Returns how many were set."""
    n = 0
    for l, rows in enumerate(_kf_rows_of_landmarks(m)):
        if rows and rows[0] <= after_kf < rows[-1] and not m["lm_bad"][l]:
            m["lm_bad"][l] = 1
            n += 1
    return n


def close_loop(m, src_kfs, dst_kf, n_add, seed=0xC105E, last_kf=None):
    """A revisit: n_add landmarks seen from the keyframe rows `src_kfs` get one more observation in row
    `dst_kf`, on dst_kf's landmark-less features (feat_flags == 0) — feat_uv is the projection under the
    map's current pose and position plus 0.5 px noise, feat_lm_id / feat_flags = 1 are set and the entry
    goes into the landmark's observation list in keyframe order.  Landmarks: good, optimisable (>= 2
    observations), not yet in dst_kf, projecting inside the image, the lowest indices first; with
    `last_kf` only landmarks that no keyframe row after it holds (a short track: the long-range block
    then touches the oldest rows alone).  Returns the number placed."""
    rng = np.random.default_rng(seed)
    lm_of = {int(v): i for i, v in enumerate(m["lm_id"])}
    fp = m["kf_feat_ptr"]
    held = _kf_rows_of_landmarks(m)
    cand = set()
    for r in src_kfs:
        for f in range(int(fp[r]), int(fp[r + 1])):
            if m["feat_flags"][f] == 1:
                l = lm_of.get(int(m["feat_lm_id"][f]))
                if l is not None and not m["lm_bad"][l] and dst_kf not in held[l] and \
                        m["lm_obs_ptr"][l + 1] - m["lm_obs_ptr"][l] >= 2 and \
                        (last_kf is None or held[l][-1] <= last_kf):
                    cand.add(l)
    free = [f for f in range(int(fp[dst_kf]), int(fp[dst_kf + 1])) if m["feat_flags"][f] == 0]
    pose = m["kf_pose"][dst_kf]
    R, t = synth.quat_to_mat(pose[:4]), pose[4:]
    fx, fy, cx, cy = m["kf_intr"][dst_kf]
    placed = 0
    for l in sorted(cand):
        if placed == n_add or placed == len(free):
            break
        pc = R @ m["lm_pos"][l] + t
        if pc[2] < 0.3:
            continue
        uv = np.array([fx * pc[0] / pc[2] + cx, fy * pc[1] / pc[2] + cy])
        if not (20 < uv[0] < 2 * cx - 20 and 20 < uv[1] < 2 * cy - 20):
            continue
        f = free[placed]
        m["feat_uv"][f] = uv + np.clip(rng.normal(0, 0.5, 2), -1.5, 1.5)
        m["feat_lm_id"][f] = m["lm_id"][l]
        m["feat_flags"][f] = 1
        o0, o1 = int(m["lm_obs_ptr"][l]), int(m["lm_obs_ptr"][l + 1])
        at = o0 + int(np.searchsorted(m["obs_kf_id"][o0:o1], m["kf_id"][dst_kf]))
        m["obs_kf_id"] = np.insert(m["obs_kf_id"], at, m["kf_id"][dst_kf])
        m["obs_feat_idx"] = np.insert(m["obs_feat_idx"], at, np.uint64(f - int(fp[dst_kf])))
        m["lm_obs_ptr"][l + 1:] += 1
        placed += 1
    return placed


# --------------------------------------------------------------------------- the cases
# name -> (keyframes, landmarks, edits, option overrides); fixed = 2 gauge keyframes unless overridden,
# f = free keyframes.  Every window is the whole map (n_old_kf = 0), so keyframe rows are window rows.
CASES = {
    "a-1tile": (3, 300, (), {}),                      # f=1: 6 rows, one tile, 10 padding rows
    "b-2tiles": (5, 500, (), {}),                     # f=3: 18 rows, a keyframe block straddles the tile boundary
    "c-3tiles-nopad": (10, 1000, (), {}),             # f=8: 48 rows, three tiles exactly
    "d-5tiles": (14, 1500, (), {}),                   # f=12: the block form spills into a second block
    "e-loop14": (14, 1500, (("loop", (2, 3), 13, 30),), {}),
    "e-loop26": (26, 2800, (("loop", (2, 3), 25, 30),), {}),
    # the issue's 14-keyframe loop fills no tile (the newest keyframe's tile row is already full in S:
    # its landmarks reach keyframe 6, its band keyframe 9); tracks that end at keyframe 3 leave tile
    # (4, 1) to the fill alone
    "e-loop14-short": (14, 1500, (("loop", (2, 3), 13, 20, ("last_kf", 3)),), {}),
    "f-split-1-11": (14, 1500, (("split", 2),), {}),
    "f-split-3-9": (14, 1500, (("split", 4),), {}),
    # 5 banded free keyframes (2 tiles) | 19 with a loop closure inside (8 tiles, fill)
    "f-band-loop26": (26, 2800, (("split", 6), ("loop", (7, 8), 25, 30)), {}),
    "h-camless-kf5": (14, 1500, (("nocam", 5),), {}),  # held fixed: a hole in the band's free rows
    "h-isolated-kf5": (14, 1500, (("nofeat", 5),), {}),  # free, no observation: S = 1e-6 I alone, rhs 0
    "i-gaugefree": (14, 1500, (), dict(fixed=0, lam=1e-2)),
}
LOOP_CASES = ("e-loop14", "e-loop14-short", "e-loop26", "f-band-loop26")
# components' free-keyframe counts, in order of their first keyframe
COMPONENTS = {"a-1tile": [1], "b-2tiles": [3], "c-3tiles-nopad": [8], "d-5tiles": [12], "e-loop14": [12],
              "e-loop14-short": [12], "e-loop26": [24], "f-split-1-11": [1, 11], "f-split-3-9": [3, 9], "f-band-loop26": [5, 19],
              "h-camless-kf5": [11], "h-isolated-kf5": [11, 1], "i-gaugefree": [14]}


@functools.lru_cache(maxsize=None)
def _case_map(name):
    nk, nl, edits, _ = CASES[name]
    m = synth.make_ba_map(SEED, nk, nl, n_old_kf=0)
    for e in edits:
        if e[0] == "loop":
            assert close_loop(m, list(e[1]), e[2], e[3], **dict(e[4:])) == e[3], (name, "loop observations not all placed")
        elif e[0] == "split":
            assert split_window(m, e[1]) > 0
        elif e[0] == "nocam":
            m["kf_has_cam"][e[1]] = 0
        elif e[0] == "nofeat":
            m["feat_flags"][int(m["kf_feat_ptr"][e[1]]):int(m["kf_feat_ptr"][e[1] + 1])] = 0
    return m


def case(name):
    """(a fresh copy of the case's map, its option keywords without `iters`)"""
    nk, _, _, over = CASES[name]
    kw = dict(window=nk, fixed=2, lam=1e-4)
    kw.update(over)
    return _case_map(name).copy(), kw


def free_keyframes(m, kw):
    """window rows the solve moves: not a gauge keyframe, and with a camera"""
    return [r for r in range(kw["window"]) if r >= kw["fixed"] and m["kf_has_cam"][r]]


# --------------------------------------------------------------------------- patterns
def symmetrise(S):
    """the full matrix from the lower triangle (vx_sba_plan_system fills only that)"""
    return np.tril(S) + np.tril(S, -1).T


def block_pattern(S):
    """(nk, nk) bool: which 6 x 6 keyframe blocks of the symmetric S hold a nonzero"""
    nk = S.shape[0] // 6
    return np.abs(S).reshape(nk, 6, nk, 6).max(axis=(1, 3)) > 0


def components(blocks, free):
    """the free keyframes' covisibility components (lists of rows), ordered by first keyframe"""
    label = {r: r for r in free}
    for _ in free:
        for a in free:
            for b in free:
                if blocks[a, b]:
                    label[a] = label[b] = min(label[a], label[b])
    return [[r for r in free if label[r] == c] for c in sorted(set(label.values()))]


def tile_pattern(blocks, comp):
    """One component's 16 x 16 tiles: (nzS, nzL) lower-triangular bool (nt, nt) — the tiles S's blocks
    touch (keyframe q of the component owns rows 6q..6q+5; diagonal tiles always, the padding rows'
    identity included) and the tiles of its Cholesky factor, by symbolic right-looking elimination:
    column k's nonzero tiles i >= j > k make (i, j) nonzero.  Fill = nzL & ~nzS."""
    nc = 6 * len(comp)
    nt = max(1, -(-nc // 16))
    el = np.kron(blocks[np.ix_(comp, comp)], np.ones((6, 6), bool))
    pad = np.zeros((16 * nt, 16 * nt), bool)
    pad[:nc, :nc] = el
    nzS = np.tril(pad.reshape(nt, 16, nt, 16).any(axis=(1, 3)) | np.eye(nt, dtype=bool))
    nzL = nzS.copy()
    for k in range(nt):
        below = [i for i in range(k + 1, nt) if nzL[i, k]]
        for i in below:
            for j in below:
                if j <= i:
                    nzL[i, j] = True
    return nzS, nzL


def tile_rows(comp, t):
    """matrix rows of tile row / column t of a component (padding rows left out)"""
    return [6 * comp[e // 6] + e % 6 for e in range(16 * t, 16 * t + 16) if e < 6 * len(comp)]


# --------------------------------------------------------------------------- solves
def _cholesky_solve(A, b, dtype):
    A = np.array(A, dtype)
    n = A.shape[0]
    L = np.zeros((n, n), dtype)
    for j in range(n):
        d = A[j, j] - (L[j, :j] * L[j, :j]).sum(dtype=dtype)
        assert d > 0, ("not positive definite at row", j)
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - (L[j + 1:, :j] * L[j, :j]).sum(axis=1, dtype=dtype)) / L[j, j]
    x = np.array(b, dtype)
    for i in range(n):
        x[i] = (x[i] - (L[i, :i] * x[:i]).sum(dtype=dtype)) / L[i, i]
    for i in range(n - 1, -1, -1):
        x[i] = (x[i] - (L[i + 1:, i] * x[i + 1:]).sum(dtype=dtype)) / L[i, i]
    return x


def solve_ext(S, rhs):
    """S x = rhs by a plain Cholesky with forward and back substitution in np.longdouble: the reference"""
    assert np.finfo(np.longdouble).eps < 2e-19, "np.longdouble is not the x87 80-bit format here"
    return _cholesky_solve(S, rhs, np.longdouble)


def solve_chol64(S, rhs):
    """the same plain Cholesky in FP64 (an independent FP64 factorisation for the CPU check of the bars)"""
    return _cholesky_solve(S, rhs, np.float64)


def errors(S, rhs, x, x_ext):
    """(backward error, forward error) of x for S x = rhs, residual and norms in longdouble; the
    forward error is None when the reference solution is exactly zero"""
    Se, xe = np.array(S, np.longdouble), np.array(x, np.longdouble)
    res = np.abs(Se @ xe - np.array(rhs, np.longdouble)).max()
    den = np.abs(Se).sum(axis=1).max() * np.abs(xe).max() + np.abs(rhs).max()
    bwd = float(res / den) if den > 0 else (0.0 if res == 0 else np.inf)
    scale = np.abs(x_ext).max()
    fwd = float(np.abs(xe - x_ext).max() / scale) if scale > 0 else None
    return bwd, fwd


def check_solution(S, rhs, dx, comps, label=""):
    """Both bars (module docstring) for the step dx of the symmetric system S, rhs, per component
    (lists of keyframe rows).  Returns one record per component: rows n, backward error and its cap,
    forward error, numpy.linalg.solve's e64 and the ratio forward / max(e64, n 2^-53)."""
    out = []
    for comp in comps:
        idx = np.concatenate([np.arange(6 * r, 6 * r + 6) for r in comp])
        A, b, x = S[np.ix_(idx, idx)], rhs[idx], dx[idx]
        n = len(idx)
        x_ext = solve_ext(A, b)
        bwd, fwd = errors(A, b, x, x_ext)
        _, e64 = errors(A, b, np.linalg.solve(A, b), x_ext)
        cap = (3 * n + 1) * EPS64
        rec = dict(label=label, n=n, bwd=bwd, cap=cap, fwd=fwd, e64=e64, ratio=None)
        print("sba-solve", label, f"n={n} bwd={bwd:.3e} cap={cap:.3e}", end=" ")
        assert np.isfinite(x).all(), (label, n)
        if fwd is None:
            print("zero reference solution")
            assert not x.any(), (label, n, "nonzero step for a zero right-hand side")
        else:
            floor = max(e64, n * EPS64)
            rec["ratio"] = fwd / floor
            print(f"fwd={fwd:.3e} e64={e64:.3e} ratio={rec['ratio']:.3f}")
            assert fwd <= FWD_FACTOR * floor, (label, n, fwd, e64)
        assert bwd <= cap, (label, n, bwd, cap)
        out.append(rec)
    return out
