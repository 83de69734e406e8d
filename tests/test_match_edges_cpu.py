"""The matcher's edge cases (tests/match_cases.py) on the CPU: the oracle's restatement of ORBMatcher::Match
against an independent numpy reference on every input the GPU module (tests/test_gpu_match_edges.py) relies
on, and the coverage conditions that keep that module from passing vacuously — computed here, not quoted.

All comparisons are exact: integers and one float32 product.
"""
import numpy as np
import pytest

import match_cases as MC


def _pin(oracle, q, t, what):
    """oracle.knn2 and oracle.match (every ratio) against the reference; returns the reference's top-2"""
    idx, dist = MC.ref_knn2(q, t)
    oi, od = oracle.knn2(q, t)
    assert np.array_equal(oi, idx) and np.array_equal(od, dist), what
    for r in MC.RATIOS:
        assert np.array_equal(oracle.match(q, t, r), MC.matches_from_knn2(idx, dist, r)), (what, r)
    return idx, dist


@pytest.fixture(scope="module")
def realised(oracle):
    """the (d1, d2) pairs the ratio_grid family realises, by the reference's top-2 — the oracle pinned on
    every member on the way"""
    got = set()
    for m in range(257):
        q, t = MC.ratio_grid(m)
        nt, pos = MC.ratio_grid_params(m)
        assert len(t) == nt and len(q) == 257 - m
        idx, dist = _pin(oracle, q, t, f"ratio_grid m={m}")
        assert np.array_equal(dist[:, 0], np.arange(257 - m)) and np.array_equal(dist[:, 1], np.arange(257 - m) + m)
        if m:
            assert np.all(idx[:, 0] == pos)
        got |= set(map(tuple, dist.tolist()))
    return got


def test_ratio_grid_realises_every_pair(realised):
    d1, d2 = MC.all_pairs()
    assert len(d1) == 33153 and realised == set(zip(d1.tolist(), d2.tolist()))
    nts = {MC.ratio_grid_params(m) for m in range(257)}
    assert {nt for nt, _ in nts} == set(MC.GRID_NT)
    for nt in MC.GRID_NT:  # every size with the zero row first, last and in between (in between: nt > 2)
        pos = {p for n, p in nts if n == nt}
        assert 0 in pos and nt - 1 in pos and (nt <= 3 or any(0 < p < nt - 1 for p in pos)), (nt, pos)


@pytest.mark.parametrize("ratio", MC.RATIOS)
def test_ratio_grid_covers_boundaries_and_rule_differences(realised, ratio):
    assert MC.boundary_pairs(ratio) <= realised
    for rule in (MC.keep_f64, MC.keep_exact, MC.keep_div, MC.keep_le):
        assert MC.differing_pairs(rule, ratio) <= realised, rule.__name__
    # (every m the GPU module may restrict a ratio to holds all of these)
    ms = set(MC.sharp_m(ratio))
    assert {b - a for a, b in MC.boundary_pairs(ratio)} <= ms


def test_rule_differences_are_not_empty():
    """the pairs that tell the float32 rule from the others: without them a kernel comparing in double,
    exactly, by division or with <= would pass"""
    n = {(rule.__name__, r): len(MC.differing_pairs(rule, r)) for r in MC.RATIOS
         for rule in (MC.keep_f64, MC.keep_exact, MC.keep_div, MC.keep_le)}
    assert (n["keep_f64", 0.8], n["keep_f64", 0.6], n["keep_f64", 0.3]) == (51, 33, 17)
    assert (n["keep_exact", 0.6], n["keep_exact", 0.3]) == (18, 8)
    assert (n["keep_div", 0.6], n["keep_div", 0.3]) == (18, 8)
    assert (n["keep_le", 0.8], n["keep_le", 1.0]) == (52, 257)
    assert MC.differing_pairs(MC.keep_exact, 0.6) == MC.differing_pairs(MC.keep_div, 0.6)


@pytest.mark.parametrize("rt", sorted({rt for _, rt in MC.SHAPES.values()}))
@pytest.mark.parametrize("kind", ["second", "tie"])
def test_planted_pairs(oracle, kind, rt):
    c = MC.planted_pairs(kind, rt, seed=int(kind == "tie"))
    assert MC.planted_ok(c, kind)
    nt = len(c["t"])
    # disjoint positions; every relation in both orders; rows 0 and nt - 1 are a pair
    pos = np.concatenate([c["near"], c["far"]])
    assert len(set(pos.tolist())) == 2 * len(c["q"])
    names = {n.rsplit(" (", 1)[0] for n in c["relation"]} - {"rows 0 and nt - 1"}
    assert len(names) >= 24
    for n in names:
        assert n + " (near < far)" in c["relation"] and n + " (near > far)" in c["relation"], n
    assert {int(c["near"][0]), int(c["far"][0])} == {0, nt - 1}
    lo, hi = np.minimum(c["near"], c["far"]), np.maximum(c["near"], c["far"])
    P = 4 * rt
    assert np.any((hi - lo) % rt == 0) and np.any((hi - lo == P)) and np.any((lo % 64 == 63) & (hi == lo + 1))
    assert np.any(hi - lo == MC.CHUNK * MC.MERGE_BATCH) and np.any(lo // MC.CHUNK == hi // MC.CHUNK)
    for b in (15, 31, 47):
        assert np.any((lo % 64 == b) & (hi == lo + 1)), b
    idx, dist = _pin(oracle, c["q"], c["t"], f"planted {kind} rt={rt}")
    if kind == "second":
        assert np.array_equal(idx[:, 0], c["near"]) and np.array_equal(idx[:, 1], c["far"])
        assert len(MC.matches_from_knn2(idx, dist, 0.8)) == 0 and len(MC.matches_from_knn2(idx, dist, 1.25)) == len(idx)
    else:
        assert np.array_equal(idx[:, 0], lo) and np.array_equal(idx[:, 1], hi)
        m = MC.matches_from_knn2(idx, dist, 1.25)
        assert len(MC.matches_from_knn2(idx, dist, 0.8)) == 0 and np.array_equal(m["train_idx"], lo)


@pytest.mark.parametrize("nt", [513, 2049])
def test_identity(oracle, nt):
    q, t = MC.identity(nt)
    idx, dist = _pin(oracle, q, t, f"identity {nt}")
    assert np.array_equal(idx[:, 0], np.arange(nt)) and not dist[:, 0].any() and dist[:, 1].min() > 0


def test_extremes(oracle):
    cases = MC.extremes()
    for name, q, t in cases:
        _pin(oracle, q, t, name)
    by = {name: (q, t) for name, q, t in cases}
    assert {len(q) for q, _ in by.values()} >= {1, 7, 8, 9, 8 * 256 + 1} and {len(t) for _, t in by.values()} >= {1, 2}
    assert MC.ref_knn2(*by["complement twice: d1 = d2 = 256"])[1].tolist() == [[256, 256]]
    assert MC.ref_knn2(*by["duplicates of the query: d1 = d2 = 0"])[0].tolist() == [[1, 2]]
    # decisions of both signs at the interior ratios, so that the keep test is exercised either way
    q, t = by["nq = 8 * 256 + 1"]
    for r in (0.3, 0.6, 0.75, 0.8):
        assert 0 < len(MC.ref_match(q, t, r)) < len(q), r
