"""Edge cases of the Hamming kNN-2 + ratio matcher and a plain numpy reference of the whole operation.

The reference (`ref_knn2`, `ref_match`) is ORBMatcher::Match restated with array operations only:
unpacked bits, an integer distance matrix, the two smallest (distance, train index) pairs per query in
lexicographic order, then one float32 product and one strict float32 compare.  Everything is integers
plus that one product, so every comparison made with it is exact.

The builders are seeded and deterministic.  Positions refer to k_knn_rows' layout (csrc/match.hip): RT
threads, thread `tid` holding train rows tid, tid + RT, ... four per pass (a pass is 4 RT rows), the
threads merged per lane over the RT / 64 waves and then over the 64 lanes by DPP rows of 16; and to the
chunked kernels' 64-row chunks, merged 32 at a time.
"""
from fractions import Fraction

import numpy as np

MATCH_DTYPE = np.dtype([("query_idx", "<i4"), ("train_idx", "<i4"), ("distance", "<f4")])
RATIOS = (0.0, 0.3, 0.6, 0.75, 0.8, 1.0, 1.25)
GRID_NT = (2, 3, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 2500)
SHAPES = {"8x512": (8, 512), "4x256": (4, 256), "16x512": (16, 512), "16x1024": (16, 1024), "8x256": (8, 256),
          "4x128": (4, 128)}
CHUNK, MERGE_BATCH = 64, 32  # k_knn_partial's rows per chunk, k_knn_merge's chunks per batch


# ------------------------------------------------------------------------------------------ reference
def hamming(q, t):
    """(nq, nt) integer Hamming distances of two (n, 32) uint8 sets"""
    q = np.asarray(q, np.uint8).reshape(-1, 32)
    t = np.asarray(t, np.uint8).reshape(-1, 32)
    qb = np.unpackbits(q, axis=1).astype(np.float32)  # (0 / 1 sums up to 256: exact in float32)
    tb = np.unpackbits(t, axis=1).astype(np.float32)
    d = qb.sum(1)[:, None] + tb.sum(1)[None, :] - 2.0 * (qb @ tb.T)
    return d.astype(np.int64)


def ref_knn2(q, t):
    """idx (nq, 2) int32 and dist (nq, 2) int32: the two smallest (distance, train index) pairs of every
    query in lexicographic order, -1 / -1 where the train set has no such row"""
    q = np.asarray(q, np.uint8).reshape(-1, 32)
    t = np.asarray(t, np.uint8).reshape(-1, 32)
    nq, nt = len(q), len(t)
    idx = np.full((nq, 2), -1, np.int32)
    dist = np.full((nq, 2), -1, np.int32)
    if nq == 0 or nt == 0:
        return idx, dist
    best = np.full((nq, 2), np.iinfo(np.int64).max, np.int64)  # distance * 2^32 + index orders the pairs
    for t0 in range(0, nt, 1 << 16):
        d = hamming(q, t[t0:t0 + (1 << 16)])
        key = d * (1 << 32) + (t0 + np.arange(d.shape[1], dtype=np.int64))[None, :]
        best = np.sort(np.concatenate([best, key], axis=1), axis=1)[:, :2]
    have = best != np.iinfo(np.int64).max
    idx[have] = (best[have] & 0xffffffff).astype(np.int32)
    dist[have] = (best[have] >> 32).astype(np.int32)
    return idx, dist


def keep_f32(d1, d2, ratio):
    """the reference's rule: one float32 product, one strict float32 compare"""
    return np.asarray(d1).astype(np.float32) < np.float32(ratio) * np.asarray(d2).astype(np.float32)


def matches_from_knn2(idx, dist, ratio):
    keep = (idx[:, 1] >= 0) & keep_f32(dist[:, 0], dist[:, 1], ratio)
    out = np.zeros(int(keep.sum()), MATCH_DTYPE)
    out["query_idx"] = np.nonzero(keep)[0]
    out["train_idx"] = idx[keep, 0]
    out["distance"] = dist[keep, 0]
    return out


def ref_match(q, t, ratio):
    """the kept matches in ascending query order (none when either set is empty or the train set has one row)"""
    return matches_from_knn2(*ref_knn2(q, t), ratio)


# other ways to write the ratio test, which the kernel must NOT be using: each differs from keep_f32 on a
# few (d1, d2) pairs, found by differing_pairs()
def keep_f64(d1, d2, ratio):
    return np.asarray(d1, np.float64) < np.float64(np.float32(ratio)) * np.asarray(d2, np.float64)


def keep_le(d1, d2, ratio):
    return np.asarray(d1).astype(np.float32) <= np.float32(ratio) * np.asarray(d2).astype(np.float32)


def keep_div(d1, d2, ratio):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.asarray(d1).astype(np.float32) / np.asarray(d2).astype(np.float32) < np.float32(ratio)


def keep_exact(d1, d2, ratio):
    r = Fraction(str(ratio))
    return np.asarray(d1, np.int64) * r.denominator < r.numerator * np.asarray(d2, np.int64)


def all_pairs():
    """every (d1, d2) with 0 <= d1 <= d2 <= 256, as two int arrays"""
    d2, d1 = np.meshgrid(np.arange(257), np.arange(257))
    m = d1 <= d2
    return d1[m], d2[m]


def differing_pairs(rule, ratio):
    """set of (d1, d2) on which `rule` decides differently from the float32 rule"""
    d1, d2 = all_pairs()
    m = rule(d1, d2, ratio) != keep_f32(d1, d2, ratio)
    return set(zip(d1[m].tolist(), d2[m].tolist()))


def boundary_pairs(ratio, width=2.0):
    """set of (d1, d2) with |d1 - ratio * d2| <= width"""
    d1, d2 = all_pairs()
    m = np.abs(d1 - float(ratio) * d2) <= width
    return set(zip(d1[m].tolist(), d2[m].tolist()))


def sharp_m(ratio):
    """the d2 - d1 of every pair that is at the boundary of `ratio` or told apart by one of the other rules"""
    pairs = boundary_pairs(ratio)
    for rule in (keep_f64, keep_le, keep_div, keep_exact):
        pairs |= differing_pairs(rule, ratio)
    return sorted({b - a for a, b in pairs})


# ------------------------------------------------------------------------------------------ builders
def _bits_to_rows(bits):
    return np.packbits(np.asarray(bits, np.uint8).reshape(-1, 256), axis=1)


def _flip(row, bits):
    b = np.unpackbits(row)
    b[bits] ^= 1
    return np.packbits(b)


def ratio_grid_params(m):
    """(nt, pos) of family member m: nt cycles through GRID_NT, pos through first / last / a seeded index"""
    nt = GRID_NT[m % len(GRID_NT)]
    which = (m // len(GRID_NT)) % 3
    pos = (0, nt - 1, int(np.random.default_rng(0x6A1D + m).integers(nt)))[which]
    return nt, pos


def ratio_grid(m, nt=None, pos=None):
    """(q, t) realising every pair (d1, d2 = d1 + m), 0 <= d1 <= 256 - m: train row `pos` is all zeros, the
    other nt - 1 rows have ones in the first m bits; query j has j ones among the last 256 - m bits"""
    if nt is None:
        nt, pos = ratio_grid_params(m)
    assert 0 <= m <= 256 and nt >= 2 and 0 <= pos < nt
    rng = np.random.default_rng(0x6A1D0000 + m)
    tb = np.zeros((nt, 256), np.uint8)
    tb[:, :m] = 1
    tb[pos] = 0
    nq = 257 - m
    qb = np.zeros((nq, 256), np.uint8)
    for j in range(nq):
        qb[j, m + rng.permutation(256 - m)[:j]] = 1
    return _bits_to_rows(qb), _bits_to_rows(tb)


def _relations(rt, nt):
    """(name, picker): picker(rng) -> (p, p') with p < p', one structural relation of the two kernels each"""
    P = 4 * rt

    def at(mod, res, delta, lim=None):
        hi = nt - delta if lim is None else min(lim, nt - delta)

        def pick(rng):
            r = res[int(rng.integers(len(res)))] if isinstance(res, (list, tuple)) else res
            n = (hi - r + mod - 1) // mod
            assert n > 0, (mod, r, delta, hi)
            p = r + mod * int(rng.integers(n))
            return p, p + delta
        return pick

    R = [(f"same thread, same pass, rows {j} apart", at(1, 0, rt * j, rt)) for j in (1, 2, 3)]
    R.append(("same thread, next pass", at(1, 0, P)))
    if rt > 64:
        R.append(("same lane, other wave", at(rt, list(range(rt - 64)), 64)))
    R += [
        ("adjacent lanes of a quad", at(4, [0, 2], 1)),
        ("lanes 0 / 2 of a quad", at(4, [0, 1], 2)),
        ("across a quad", at(4, 3, 1)),
        ("across an 8-lane half row", at(8, [0, 1, 2, 3], 4)),
        ("across a 16-lane row's halves", at(16, list(range(8)), 8)),
        ("lanes 15 / 16", at(64, 15, 1)),
        ("lanes 31 / 32", at(64, 31, 1)),
        ("lanes 47 / 48", at(64, 47, 1)),
        ("DPP rows 0 and 1", at(64, list(range(16)), 16)),
        ("DPP rows 0 and 2", at(64, list(range(16)), 32)),
        ("DPP rows 0 and 3", at(64, list(range(16)), 48)),
        ("DPP rows 1 and 3", at(64, list(range(16, 32)), 32)),
        ("DPP rows 2 and 3", at(64, list(range(32, 48)), 16)),
        ("lane 63 / lane 0 of the next wave, chunk boundary", at(64, 63, 1)),
        ("last thread / thread 0 of the next row slot", at(rt, rt - 1, 1)),
        ("same chunk", at(CHUNK, list(range(40)), 20)),
        ("adjacent chunks", at(1, 0, CHUNK)),
        ("chunks 32 apart", at(1, 0, CHUNK * MERGE_BATCH)),
        ("chunks 31 / 32: adjacent merge batches", at(CHUNK * MERGE_BATCH, list(range(CHUNK * (MERGE_BATCH - 1),
                                                                                   CHUNK * MERGE_BATCH)), CHUNK)),
        ("anywhere", lambda rng: tuple(sorted(int(x) for x in rng.choice(nt, 2, replace=False)))),
    ]
    return R


def planted_pairs(kind, rt=512, seed=0, nq=600):
    """About 600 random queries against about 2 500 random train rows (more where a pass of 4 rt rows needs
    it).  Query k's two nearest rows are planted at positions (near_k, far_k), disjoint over k:
      kind "second": q_k with 8 bits flipped at near_k, with 9 bits flipped at far_k — ratio 0.8 does not keep
                     it (8 < 7.2 is false), and a kernel that lost far_k would (8 < 0.8 * 40 or more);
      kind "tie":    two different sets of 8 bits — ratio 1.25 keeps it with train_idx = min(near_k, far_k).
    The position pairs walk through every relation of _relations(rt, nt) in both orders (near < far and
    near > far); rows 0 and nt - 1 are one pair, near at row 0 for an even seed and at nt - 1 for an odd one.
    Every other row is at distance >= 40 from every query (asserted by the caller with the reference:
    `planted_ok`).  Returns dict(q, t, near, far, relation)."""
    assert kind in ("second", "tie")
    nt = max(2500, 4 * rt + 452)
    rng = np.random.default_rng([0x91A7, seed, rt, kind == "tie"])
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    rel = _relations(rt, nt)
    used = {0, nt - 1}
    near, far, names = [], [], []
    for k in range(nq):
        if k == 0:
            name, (p, p2) = "rows 0 and nt - 1", (0, nt - 1)
            order = seed & 1
        else:
            # (a relation with few positions, such as the last thread's, runs out: the next one takes its turn)
            order = ((k - 1) // len(rel)) & 1
            for step in range(len(rel)):
                name, pick = rel[(k - 1 + step) % len(rel)]
                for _ in range(200):
                    p, p2 = pick(rng)
                    if p not in used and p2 not in used:
                        break
                else:
                    continue
                break
            else:
                raise AssertionError("no free positions")
            used |= {p, p2}
        a, b = (p, p2) if order == 0 else (p2, p)
        bits = rng.permutation(256)
        t[a] = _flip(q[k], bits[:8])
        t[b] = _flip(q[k], bits[8:17] if kind == "second" else bits[8:16])
        near.append(a)
        far.append(b)
        names.append(name + (" (near < far)" if a < b else " (near > far)"))
    return dict(q=q, t=t, near=np.array(near, np.int32), far=np.array(far, np.int32), relation=names)


def planted_ok(case, kind):
    """the input condition of planted_pairs, by the reference: the planted rows are the two nearest at
    distances (8, 9) or (8, 8), every other row is at 40 or more"""
    d = hamming(case["q"], case["t"])
    k = np.arange(len(d))
    ok = np.all(d[k, case["near"]] == 8) and np.all(d[k, case["far"]] == (9 if kind == "second" else 8))
    d[k, case["near"]] = 1000
    d[k, case["far"]] = 1000
    return bool(ok and d.min() >= 40)


def identity(nt):
    """q = t, nt random rows: every train position is the winner exactly once"""
    t = np.random.default_rng(0x1DE0 + nt).integers(0, 256, (nt, 32), dtype=np.uint8)
    return t.copy(), t


def noisy(nq, nt, seed):
    """nq queries whose two nearest of nt random rows are at small random distances d1 <= d2 <= 24 (decisions
    of both signs at every ratio), on random rows"""
    rng = np.random.default_rng([0x9015E, seed, nq, nt])
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    if nt >= 2:
        for k in range(nq):
            a, b = rng.choice(nt, 2, replace=False)
            d = np.sort(rng.integers(0, 25, 2))
            q[k] = _flip(t[a], rng.permutation(256)[:d[0]])
            if k < nt // 2:  # (a second row close by, while rows are left to overwrite)
                t[b] = _flip(q[k], rng.permutation(256)[:d[1]])
    return q, t


def extremes():
    """list of (name, q, t): the largest and smallest keys, the smallest train sets, query counts around a
    workgroup's 8 and one past 256 workgroups' worth"""
    rng = np.random.default_rng(0xE87)
    r = rng.integers(0, 256, (4, 32), dtype=np.uint8)
    out = [
        ("complement twice: d1 = d2 = 256", r[:1], np.stack([~r[0], ~r[0]])),
        ("complement: 256, 256, 255", r[:1], np.stack([~r[0], ~r[0], _flip(~r[0], [77])])),
        ("complement alone among 513", r[:1], np.repeat((~r[0])[None], 513, axis=0)),
        ("duplicates of the query: d1 = d2 = 0", r[1:2], np.stack([r[2], r[1], r[1], r[3], r[1]])),
        ("duplicates only, 2049 rows", r[1:2], np.repeat(r[1][None], 2049, axis=0)),
        ("nt = 1", *noisy(5, 1, 1)),
        ("nt = 2", *noisy(5, 2, 2)),
    ]
    out += [(f"nq = {n}", *noisy(n, 100, 10 + n)) for n in (1, 7, 8, 9)]
    out.append(("nq = 8 * 256 + 1", *noisy(8 * 256 + 1, 300, 3)))
    return out
