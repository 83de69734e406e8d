"""vx_relocalize_* (csrc/reloc.hip) without a GPU: declarations, exports and bindings; sizeof and field offsets of
both records against the numpy dtypes (a small C++ program compiled against include/vx_slam.h); the numpy
restatement of the pool and record rules (tests/reloc_ref.py) pinned on hand-written lists; the adapter's
candidate choice (Tracking::RelocCandidates through tests/cpp/reloc_driver: host logic, no device)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import vxslam

import reloc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "visionx-slam_amd", "build", "reloc_driver")
NAMES = ["vx_relocalize_async", "vx_relocalize_fetch", "vx_relocalize_matches", "vx_relocalize_table_limit"]
MATCH = [("query_idx", "<i4"), ("train_idx", "<i4"), ("distance", "<f4")]


def test_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "vx_slam.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", vxslam.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert re.search(r" T %s$" % n, out, flags=re.M), n
        assert n in vxslam.EXPORTS, n
        assert hasattr(vxslam.lib(), n), n
    assert re.search(r"#define\s+VX_MAX_RELOC_CANDIDATES\s+16\b", hdr)
    for t in ("vx_reloc_candidate", "vx_reloc_candidate_result", "vx_reloc_result"):
        assert re.search(r"\}\s*%s;" % t, hdr), t
    assert "tracking.cpp:332-455" in hdr and "tracking.cpp:477-499" in hdr   # what it ports, and the TODO it answers
    assert vxslam.MAX_RELOC_CANDIDATES == 16
    for n in ("relocalize_async", "relocalize_fetch", "relocalize_matches"):
        assert hasattr(vxslam.Context, n), n
    L = vxslam.lib()
    L.vx_prof_name.restype = C.c_char_p
    names = [L.vx_prof_name(i).decode() for i in range(L.vx_prof_count())]
    for n in ("reloc_pairs", "reloc_pool", "reloc_final"):
        assert names.count(n) == 1, n
    assert names.index("rig_kf_commit") < names.index("reloc_pairs")   # the existing stages keep their numbers


def test_null_arguments_need_no_device():
    L = vxslam.lib()
    assert L.vx_relocalize_async(None, None, 1, None, None, C.c_float(0.8), None, None) == vxslam.VX_ERR_INVALID
    assert L.vx_relocalize_fetch(None, None, None, None, None, None, 0) == vxslam.VX_ERR_INVALID
    assert L.vx_relocalize_matches(None, 0, None, None, None) == vxslam.VX_ERR_INVALID
    assert L.vx_relocalize_table_limit(None, None) == vxslam.VX_ERR_INVALID


PROGRAM = r"""
#include <cstddef>
#include <cstdio>
#include "vx_slam.h"
#define F(T, f) std::printf(#T " " #f " %zu\n", offsetof(T, f))
int main() {
    std::printf("vx_reloc_candidate size %zu\n", sizeof(vx_reloc_candidate));
    F(vx_reloc_candidate, kf_id); F(vx_reloc_candidate, frame);
    std::printf("vx_reloc_candidate_result size %zu\n", sizeof(vx_reloc_candidate_result));
    F(vx_reloc_candidate_result, n_matches); F(vx_reloc_candidate_result, n_good_matches); F(vx_reloc_candidate_result, n_pairs);
    F(vx_reloc_candidate_result, n_bad_index); F(vx_reloc_candidate_result, open); F(vx_reloc_candidate_result, n_kept);
    F(vx_reloc_candidate_result, n_inliers); F(vx_reloc_candidate_result, min_distance); F(vx_reloc_candidate_result, parallax);
    std::printf("vx_reloc_result size %zu\n", sizeof(vx_reloc_result));
    F(vx_reloc_result, status); F(vx_reloc_result, n_cand); F(vx_reloc_result, n_pool); F(vx_reloc_result, best_cand);
    F(vx_reloc_result, parallax); F(vx_reloc_result, pnp); F(vx_reloc_result, cand);
    return 0;
}
"""


def test_record_layouts_equal_the_dtypes(tmp_path):
    src, exe = os.path.join(tmp_path, "layout.cpp"), os.path.join(tmp_path, "layout")
    open(src, "w").write(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
    got = {}
    for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines():
        t, f, v = line.split()
        got[(t, f)] = int(v)
    for t, dt in (("vx_reloc_candidate", vxslam.RELOC_CANDIDATE_DTYPE),
                  ("vx_reloc_candidate_result", vxslam.RELOC_CANDIDATE_RESULT_DTYPE), ("vx_reloc_result", vxslam.RELOC_RESULT_DTYPE)):
        assert got.pop((t, "size")) == dt.itemsize, t
        for name in dt.names:
            assert got.pop((t, name)) == dt.fields[name][1], (t, name)
    assert not got                                                 # every field of the C records is in a dtype
    assert vxslam.RELOC_RESULT_DTYPE.itemsize == 808 and vxslam.RELOC_CANDIDATE_RESULT_DTYPE.itemsize == 40
    assert vxslam.RELOC_RESULT_DTYPE["cand"].shape == (16,) and vxslam.RELOC_RESULT_DTYPE["pnp"] == vxslam.PNP_RESULT_DTYPE


# ---------------------------------------------------------------------------- reloc_ref on hand-written lists
def cand(rows, pair_match=None, n_good=None):
    m = np.array(rows, MATCH)
    pm = np.arange(len(m), dtype=np.int32) if pair_match is None else np.array(pair_match, np.int32)
    return {"matches": m, "pair_match": pm, "n_good_matches": len(m) if n_good is None else n_good}


def pool(cands):
    p = R.pool_ref(cands, min_matches=2)
    return list(zip(p["pool_cand"].tolist(), p["pool_match"].tolist(), p["pool_train"].tolist())), p


def test_equal_distance_across_candidates_goes_to_the_lower_candidate():
    a = cand([(0, 5, 7.0), (1, 6, 9.0)])
    b = cand([(0, 5, 7.0), (1, 8, 9.0)])
    got, p = pool([a, b])
    assert got == [(0, 0, 5), (0, 1, 6), (1, 1, 8)] and p["n_kept"] == [2, 1] and p["n_concat"] == 4


def test_smaller_distance_in_a_later_candidate_wins():
    a = cand([(0, 5, 7.0), (1, 6, 9.0)])
    b = cand([(0, 6, 8.5), (1, 5, 7.5)])
    c = cand([(3, 5, 6.0), (4, 9, 1.0)])
    got, _ = pool([a, b, c])
    assert got == [(1, 0, 6), (2, 0, 5), (2, 1, 9)]                # the survivors keep the concatenation order


def test_same_train_index_twice_in_one_candidate_goes_to_the_lower_pair():
    a = cand([(0, 5, 7.0), (1, 5, 7.0), (2, 4, 3.0), (3, 5, 6.5), (4, 4, 3.0)])
    got, _ = pool([a])
    assert got == [(0, 2, 4), (0, 3, 5)]
    # pool_match indexes the candidate's match list, through its pair_match
    b = cand([(9, 1, 50.0), (0, 5, 7.0), (1, 5, 7.0)], pair_match=[1, 2], n_good=3)
    got, _ = pool([b])
    assert got == [(0, 1, 5)]


def test_a_closed_candidate_contributes_nothing_wherever_it_stands():
    o1 = cand([(0, 5, 7.0), (1, 6, 9.0)])
    o2 = cand([(0, 7, 2.0), (1, 6, 9.5)])
    closed = cand([(0, 5, 0.0), (1, 6, 0.0), (2, 7, 0.0)], n_good=1)   # nearer everywhere, but below min_matches
    want = [(0, 0, 5), (0, 1, 6), (1, 0, 7)]
    for order in ([closed, o1, o2], [o1, closed, o2], [o1, o2, closed]):
        got, p = pool(order)
        idx = [i for i, k in enumerate(order) if k is not closed]
        at = [i for i, k in enumerate(order) if k is closed][0]
        assert got == [(idx[c], m, t) for c, m, t in want], at
        assert p["open"] == [k is not closed for k in order] and p["n_kept"][at] == 0


def test_an_empty_pool():
    closed = cand([(0, 5, 0.0)], n_good=1)
    no_pairs = cand([(0, 5, 1.0), (1, 6, 1.0)], pair_match=[])
    for cands, status in (([closed, closed], R.FEW_MATCHES), ([no_pairs], R.FEW_PAIRS), ([closed, no_pairs], R.FEW_PAIRS)):
        got, p = pool(cands)
        assert got == [] and p["n_pool"] == 0 and p["pool_cand"].dtype == np.uint8 and p["pool_match"].dtype == np.int32
        rec = R.record_ref(p, [1.5] * len(cands), 0, 0, True, [], min_inliers=1)
        assert rec == {"status": status, "ran": False, "n_inliers": [0] * len(cands), "best_cand": -1, "parallax": 0.0}


def test_the_record_rules():
    a = cand([(0, 5, 7.0), (1, 6, 9.0), (2, 7, 1.0)])
    b = cand([(0, 8, 7.0), (1, 9, 9.0), (2, 10, 1.0)])
    _, p = pool([a, b])
    par = [2.5, 3.5]
    ok = R.record_ref(p, par, 1, 4, True, [1, 1, 0, 0, 1, 1], min_inliers=4)
    assert ok == {"status": R.OK, "ran": True, "n_inliers": [2, 2], "best_cand": 0, "parallax": 2.5}    # a tie: the lower index
    assert R.record_ref(p, par, 1, 4, True, [1, 0, 0, 1, 1, 1], min_inliers=4)["best_cand"] == 1
    assert R.record_ref(p, par, 1, 3, True, [1, 1, 1, 0, 0, 0], min_inliers=4)["status"] == R.PNP_FAILED
    assert R.record_ref(p, par, 0, 6, True, [1] * 6, min_inliers=4)["status"] == R.PNP_FAILED
    assert R.record_ref(p, par, 1, 6, False, [1] * 6, min_inliers=4)["status"] == R.BAD_ROTATION
    few = R.record_ref(p, par, 1, 6, True, [1] * 6, min_inliers=7)
    assert few["status"] == R.FEW_PAIRS and not few["ran"] and few["n_inliers"] == [0, 0]
    assert R.record_ref(p, par, 1, 6, True, [1] * 6, min_inliers=6)["ran"]                              # n_pool == min_inliers runs
    assert R.max_iterations_ref(6) == 12 and R.max_iterations_ref(60) == 100 and R.max_iterations_ref(6, 33) == 33
    assert (R.OK, R.FEW_MATCHES, R.FEW_PAIRS, R.PNP_FAILED, R.BAD_ROTATION) == (
        vxslam.TRACK_OK, vxslam.TRACK_FEW_MATCHES, vxslam.TRACK_FEW_PAIRS, vxslam.TRACK_PNP_FAILED, vxslam.TRACK_BAD_ROTATION)


# ---------------------------------------------------------------------------- the adapter's candidate choice
def candidates(max_candidates, *kfs):
    assert os.path.exists(DRIVER), f"{DRIVER} missing: run __graft_entry__.build()"
    out = subprocess.run([DRIVER, "candidates", str(max_candidates), *kfs], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    return [int(x) for x in out.stdout.split()]


def test_adapter_candidate_choice():
    kfs = ["1:r", "5:h", "7:r", "9:r", "11:h", "2:r", "30:r"]
    assert candidates(3, *kfs) == [30, 9, 7]                        # the highest ids with a resident frame, latest first
    assert candidates(16, *kfs) == [30, 9, 7, 2, 1]                 # fewer than asked for: all of them
    assert candidates(1, *kfs) == [30]
    assert candidates(0, *kfs) == [] and candidates(4, "3:h", "4:h") == [] and candidates(4) == []
    assert candidates(16, *["%d:r" % i for i in range(40)]) == list(range(39, 23, -1))
