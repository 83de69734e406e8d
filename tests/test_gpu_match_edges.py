"""The matcher (csrc/match.hip) at its edges: ratio-test boundaries, the second neighbour, ties, every entry point,
device counts below capacity, the largest train set and every kernel variant.

Every assertion is np.array_equal against the oracle's restatement of ORBMatcher::Match, which
tests/test_match_edges_cpu.py pins against an independent numpy reference on these same inputs
(tests/match_cases.py), together with the coverage conditions: the ratio_grid family realises every (d1, d2) pair,
so every pair at a ratio's boundary and every pair that tells the reference's float32 product + strict compare from a
compare in double, by division, in exact arithmetic or with <=.  Integers and one float32 product: no tolerance.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import match_cases as MC

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _dev(rows, cap=None, count=None):
    """rows in a device buffer of `cap` rows (default: as many, at least one) with an int32 device count:
    the (ptr, count_ptr, cap) triple and the tensors that own the memory"""
    import torch

    rows = np.ascontiguousarray(rows, np.uint8).reshape(-1, 32)
    cap = max(len(rows), 1) if cap is None else cap
    buf = np.zeros((cap, 32), np.uint8)
    buf[:len(rows)] = rows
    d = torch.from_numpy(buf).to("cuda:0")
    n = torch.tensor([len(rows) if count is None else count], dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    return (d.data_ptr(), n.data_ptr(), cap), (d, n)


@pytest.fixture(scope="module")
def grid():
    return [MC.ratio_grid(m) for m in range(257)]


@pytest.fixture(scope="module")
def planted():
    """planted_pairs of both kinds for the default shape (rows 0 / nt - 1: near first in one, last in the other)"""
    return {kind: MC.planted_pairs(kind, 512, seed=int(kind == "tie")) for kind in ("second", "tie")}


@pytest.fixture(scope="module")
def sixteen():
    """16 (q, t) pairs of different sizes, each from another seed or m, one with an empty query side and one with
    an empty train side"""
    pairs = []
    for s in range(8):
        c = MC.planted_pairs("second" if s < 4 else "tie", 512, seed=s)
        pairs.append((c["q"], c["t"]))
    pairs += [MC.ratio_grid(m) for m in (0, 1, 51, 128, 204, 256)]
    e = np.zeros((0, 32), np.uint8)
    pairs.insert(3, (e, MC.identity(513)[1]))
    pairs.insert(9, (MC.identity(513)[0], e))
    assert len(pairs) == 16
    return pairs


def _oracle_pairs(oracle, pairs, ratio):
    return [oracle.match(q, t, ratio) if len(q) and len(t) else np.zeros(0, MC.MATCH_DTYPE) for q, t in pairs]


# ------------------------------------------------------------------------------------------ ratio boundary
@pytest.mark.parametrize("ratio", MC.RATIOS)
def test_ratio_boundary(ctx, oracle, grid, ratio):
    """Every m of the ratio_grid family (all 257: none dropped for any ratio) through Context.match."""
    for m, (q, t) in enumerate(grid):
        got, ref = ctx.match(q, t, ratio), oracle.match(q, t, ratio)
        assert np.array_equal(got, ref), (m, MC.ratio_grid_params(m), len(got), len(ref))


# ------------------------------------------------------------------------------------------ second neighbour, ties
@pytest.mark.parametrize("ratio", [0.8, 1.25])
def test_second_neighbour_and_ties(ctx, oracle, planted, ratio):
    for kind, c in planted.items():
        got = ctx.match(c["q"], c["t"], ratio)
        ref = oracle.match(c["q"], c["t"], ratio)
        bad = sorted(set(ref["query_idx"].tolist()) ^ set(got["query_idx"].tolist()))
        assert np.array_equal(got, ref), (kind, [c["relation"][k] for k in bad[:5]],
                                          [c["relation"][k] for k in np.nonzero(got["train_idx"] != ref["train_idx"])[0][:5]]
                                          if len(got) == len(ref) else None)
        # (what the case is built for: a lost second neighbour keeps a "second" query at 0.8; a tie goes to the lower row)
        assert len(got) == (0 if ratio == 0.8 else len(c["q"]))
        if kind == "tie" and ratio == 1.25:
            assert np.array_equal(got["train_idx"], np.minimum(c["near"], c["far"]))
    for nt in (513, 2049):
        q, t = MC.identity(nt)
        got = ctx.match(q, t, ratio)
        assert np.array_equal(got, oracle.match(q, t, ratio)) and np.array_equal(got["train_idx"], np.arange(nt))
    for name, q, t in MC.extremes():
        assert np.array_equal(ctx.match(q, t, ratio), oracle.match(q, t, ratio)), name


# ------------------------------------------------------------------------------------------ entry points
@pytest.mark.parametrize("ratio", [0.8, 1.25])
def test_ratio_reaches_match_device_async(ctx, oracle, planted, ratio):
    for kind, c in planted.items():
        (tq, kq), (tt, kt) = _dev(c["q"]), _dev(c["t"])
        ctx.match_device_async(tq, tt, ratio)
        assert np.array_equal(ctx.match_fetch(), oracle.match(c["q"], c["t"], ratio)), kind


@pytest.mark.parametrize("ratio", [0.6, 0.8, 1.25])
def test_ratio_reaches_match_batch_async(ctx, oracle, sixteen, ratio):
    """16 pairs of different sizes in one call: the capacities are the largest pair's, every other pair's counts
    lie below them, and two pairs have an empty side."""
    dev = [(_dev(q), _dev(t)) for q, t in sixteen]
    ctx.match_batch_async([(a[0], b[0]) for a, b in dev], ratio)
    ref = _oracle_pairs(oracle, sixteen, ratio)
    for i in range(16):
        assert np.array_equal(ctx.match_batch_fetch(i), ref[i]), i
    assert sum(len(r) for r in ref) > 0 and not len(ref[3]) and not len(ref[9])


@pytest.mark.parametrize("ratio", [0.6, 0.8, 1.25])
def test_ratio_reaches_match_knn2_ratio_batch(ctx, oracle, sixteen, ratio):
    got = ctx.match_batch(sixteen, ratio)
    ref = _oracle_pairs(oracle, sixteen, ratio)
    assert len(got) == 16
    for i in range(16):
        assert np.array_equal(got[i], ref[i]), i


def test_ratio_reaches_seq_match(ctx, oracle, planted):
    import vxslam

    for kind, c in planted.items():
        (tq, kq), (tt, kt) = _dev(c["q"]), _dev(c["t"])
        for ratio in (0.8, 1.25):
            sq = vxslam.Seq()
            sq.match(ctx, tq, tt, ratio)
            for rep in range(2):
                sq.run()
                assert np.array_equal(ctx.match_fetch(), oracle.match(c["q"], c["t"], ratio)), (kind, ratio, rep)
            sq.close()


def test_graph_replay_keeps_the_ratio_apart(oracle):
    """vx_match_device_async on the same buffers (after a first call that sizes the context's scratch, whose
    addresses are part of the key): 0.8 eager, captured and replayed, then 0.6, 0.8, 0.6 — each result the oracle's
    at that call's ratio (the ratio is part of the graph's key)."""
    import vxslam

    q, t = MC.ratio_grid(51)  # d2 = d1 + 51: the decision flips at d1 = 77 under 0.6 and at d1 = 204 under 0.8
    ref = {r: oracle.match(q, t, r) for r in (0.6, 0.8, 1.0)}
    assert 0 < len(ref[0.6]) < len(ref[0.8]) < len(q)
    c = vxslam.Context(0)
    try:
        (tq, kq), (tt, kt) = _dev(q), _dev(t)
        for ratio in (1.0, 0.8, 0.8, 0.8, 0.6, 0.8, 0.6):
            c.match_device_async(tq, tt, ratio)
            assert np.array_equal(c.match_fetch(), ref[ratio]), ratio
        captured, launched = c.graph_counts()
        assert captured >= 2 and launched >= 2, (captured, launched)  # (both ratios captured, 0.8 replayed twice)
    finally:
        c.close()


# ------------------------------------------------------------------------------------------ counts below capacity
@pytest.mark.parametrize("nq,nt,cap", [(0, 500, 512), (500, 0, 512), (1, 1, 64), (9, 513, 2048), (2049, 2500, 4254)])
def test_device_count_below_capacity(ctx, oracle, nq, nt, cap):
    """Buffers of `cap` rows with the counts on the device: the train buffer's rows past its count are exact copies of
    queries, the query buffer's rows past its count exact copies of train rows (random rows where that set is empty) —
    a kernel that read one of them would find a distance 0.  Single, and batched next to a pair that takes the same
    buffers whole (counts = cap), so the counts are seen to be per pair."""
    q, t = MC.noisy(nq, nt, 40 + cap)
    rnd = np.random.default_rng(cap).integers(0, 256, (cap, 32), dtype=np.uint8)
    qbuf = np.concatenate([q, np.resize(t if nt else rnd, (cap - nq, 32))])
    tbuf = np.concatenate([t, np.resize(q if nq else rnd, (cap - nt, 32))])
    assert np.array_equal(qbuf[:nq], q) and np.array_equal(tbuf[:nt], t)
    (tq, kq), (tt, kt) = _dev(qbuf, cap, nq), _dev(tbuf, cap, nt)
    (fq, kfq), (ft, kft) = _dev(qbuf, cap, cap), _dev(tbuf, cap, cap)
    for ratio in (0.8, 1.25):
        ref = oracle.match(q, t, ratio) if nq and nt else np.zeros(0, MC.MATCH_DTYPE)
        full = oracle.match(qbuf, tbuf, ratio)
        ctx.match_device_async(tq, tt, ratio)
        assert np.array_equal(ctx.match_fetch(), ref), ("single", ratio)
        ctx.match_batch_async([(tq, tt), (fq, ft)], ratio)
        assert np.array_equal(ctx.match_batch_fetch(0), ref), ("batched", ratio)
        assert np.array_equal(ctx.match_batch_fetch(1), full), ("batched, whole buffers", ratio)


# ------------------------------------------------------------------------------------------ largest train set
def test_largest_train_set(ctx, oracle):
    """2^22 train rows (the 22-bit index field next to distances up to 256): the two nearest rows at the last two
    indices, in both orders, and at the first and the last; one row more is refused."""
    import vxslam

    n = 1 << 22
    rng = np.random.default_rng(0x400000)
    big = rng.integers(0, 256, (n + 1, 32), dtype=np.uint8)
    t = big[:n]
    q = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    # (near row, far row), (bits flipped in each): query 3's two nearest rows are planted there, the other seven
    # queries meet random rows only; kept under 0.8 (3 < 7.2), not kept (8 < 7.2 is false), a tie, kept (0 < 3.2)
    for (a, b), (da, db) in zip([(n - 1, n - 2), (n - 2, n - 1), (0, n - 1), (n - 1, 0)], [(3, 9), (8, 9), (8, 8), (0, 4)]):
        saved = t[[a, b]].copy()
        bits = rng.permutation(256)
        t[a], t[b] = MC._flip(q[3], bits[:da]), MC._flip(q[3], bits[da:da + db])
        for ratio in (0.8, 1.25):
            got, ref = ctx.match(q, t, ratio), oracle.match(q, t, ratio)
            assert np.array_equal(got, ref), (a, b, ratio, got, ref)
        hit = ref[ref["query_idx"] == 3]  # (under 1.25 every planted query is kept)
        assert len(hit) == 1 and hit["train_idx"][0] == (min(a, b) if da == db else a) and hit["distance"][0] == da
        t[[a, b]] = saved
    with pytest.raises(vxslam.VxError) as e:
        ctx.match(q, big, 0.8)
    assert e.value.code == vxslam.VX_ERR_INVALID


# ------------------------------------------------------------------------------------------ kernel variants
VARIANTS = [("VX_MATCH_SHAPE", s) for s in MC.SHAPES] + [("VX_MATCH_CHUNKED", "1")] + [("VX_MATCH_GRID", g) for g in "013"]
_abnormal = []  # the first child that did not exit with 0: no further child is started after it


@pytest.fixture(scope="module")
def variant_cases(oracle):
    """per RT: the list of (q, t, ratio) a child runs and the oracle's results, computed once"""
    cache = {}

    def build(rt):
        if rt not in cache:
            cases = []
            for kind in ("second", "tie"):
                c = MC.planted_pairs(kind, rt, seed=int(kind == "tie"))
                cases += [(c["q"], c["t"], r) for r in (0.8, 1.25)]
            cases += [(*MC.identity(2049), r) for r in (0.8, 1.25)]
            cases += [(q, t, r) for _, q, t in MC.extremes() for r in (0.8, 1.25)]
            cases += [(*MC.ratio_grid(m), r) for m in (0, 1, 51, 128, 256) for r in (0.8, 0.6, 1.25)]
            cache[rt] = cases, [oracle.match(q, t, r) for q, t, r in cases]
        return cache[rt]
    return build


@pytest.mark.parametrize("var,value", VARIANTS, ids=[f"{k[9:].lower()}-{v}" for k, v in VARIANTS])
def test_kernel_variant(oracle, variant_cases, tmp_path, var, value):
    """Each k_knn_rows shape, the chunked kernels and the grid caps, in a fresh process each (the variables are read
    once per process): planted_pairs for that shape's RT, identity, extremes and five ratio_grid members — equal to the
    oracle, hence to one another."""
    assert not _abnormal, f"no child started: {_abnormal[0]} did not exit with 0"
    rt = MC.SHAPES[value][1] if var == "VX_MATCH_SHAPE" else 512
    cases, ref = variant_cases(rt)
    src, dst = str(tmp_path / "cases.npz"), str(tmp_path / "results.npz")
    arrays = {"n": np.int64(len(cases))}
    for i, (q, t, r) in enumerate(cases):
        arrays[f"q_{i}"], arrays[f"t_{i}"], arrays[f"ratio_{i}"] = q, t, np.float64(r)
    np.savez(src, **arrays)
    env = {k: v for k, v in os.environ.items() if not k.startswith("VX_MATCH_")}
    env[var] = value
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(HERE, "match_variant_child.py"), src, dst]
    try:
        p = subprocess.run(cmd, env=env, timeout=120, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _abnormal.append(f"{var}={value} (no exit within 120 s)")
        raise
    if p.returncode != 0:
        _abnormal.append(f"{var}={value} (exit {p.returncode})")
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    got = np.load(dst)
    for i, (q, t, r) in enumerate(cases):
        assert np.array_equal(got[f"m_{i}"], ref[i]), (var, value, i, len(q), len(t), r)
