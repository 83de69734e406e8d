"""vx_dmap_create_keyframes_rig (csrc/keyframe_rig.hip) without a GPU: the declaration, export and
binding, RIG_KEYFRAME_DTYPE against the header's struct, and the numpy restatement
(tests/keyframe_rig_ref.py) — its chaining equals N single keyframe_ref.create_keyframe calls with the
ids carried, and a fault in any camera leaves the map dict untouched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import vxslam
from vxslam import synth

import keyframe_ref as R
import keyframe_rig_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "vx_dmap_create_keyframes_rig"


def test_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "vx_slam.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", vxslam.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\b%s\s*\(" % NAME, hdr)
    assert re.search(r" T %s$" % NAME, out, flags=re.M)
    assert NAME in vxslam.EXPORTS and hasattr(vxslam.lib(), NAME)
    assert hasattr(vxslam.DMap, "create_keyframes_rig")
    assert re.search(r"#define\s+VX_KF_ERR_RIG_REPEAT\s+\(1 << 6\)", hdr) and vxslam.KF_ERR_RIG_REPEAT == 64
    assert (RR.ERR_ID_RANGE, RR.ERR_RIG_REPEAT) == (vxslam.KF_ERR_ID_RANGE, vxslam.KF_ERR_RIG_REPEAT)
    # the four kernels are profiling stages with stable names, after the existing ones
    L = vxslam.lib()
    L.vx_prof_name.restype = C.c_char_p
    names = [L.vx_prof_name(i).decode() for i in range(L.vx_prof_count())]
    for n in ("rig_kf_feat", "rig_kf_match", "rig_kf_count", "rig_kf_commit"):
        assert names.count(n) == 1, n
    assert names.index("frame_capture_batch") < names.index("rig_kf_feat")
    assert len(names) <= 64  # vx_prof_enable64's mask
    # no context: refused without touching a device
    assert L.vx_dmap_create_keyframes_rig(None, None, 1, None, C.c_uint64(0), None, None) == vxslam.VX_ERR_INVALID


SIZES = {"uint64_t": 8, "int64_t": 8, "int32_t": 4, "double": 8}


def struct_layout(hdr, name):
    """(field names, offsets, size) of a typedef struct of the header under the C ABI's natural alignment"""
    body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names, offs, at, align = [], [], 0, 1
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, rest = re.match(r"(?:const\s+)?(\w+)\s*(.*)", decl).groups()
        for f in rest.split(","):
            f = f.strip()
            size = 8 if f.startswith("*") else SIZES[typ]
            at = (at + size - 1) // size * size
            names.append(f.lstrip("* "))
            offs.append(at)
            at += size
            align = max(align, size)
    return names, offs, (at + align - 1) // align * align


def test_dtype_mirrors_the_struct():
    hdr = open(os.path.join(ROOT, "include", "vx_slam.h")).read()
    names, offs, size = struct_layout(hdr, "vx_rig_keyframe")
    T = vxslam.RIG_KEYFRAME_DTYPE
    assert list(T.names) == names
    assert [T.fields[n][1] for n in T.names] == offs
    assert T.itemsize == size == 104
    for n in ("pose7", "intr4", "curr", "d_matches", "d_n_matches", "depth"):
        assert T.fields[n][0] == np.dtype("<u8"), n
    # the parser itself against a struct whose size the library pins
    assert struct_layout(hdr, "vx_rig_camera")[2] == vxslam.RIG_CAMERA_DTYPE.itemsize


def test_the_rules_are_stated_once():
    """the single-camera kernels and the rig kernels run the same program text"""
    csrc = os.path.join(ROOT, "visionx-slam_amd", "csrc")
    rd = lambda f: open(os.path.join(csrc, f)).read()
    for f in ("keyframe.hip", "keyframe_rig.hip"):
        src = rd(f)
        assert '#include "keyframe_bodies.hpp"' in src and '#include "keyframe_commit_body.inc"' in src, f
        assert "feat_body(" in src and "match_body(" in src, f
    for rule in ("a.feat_fl[g] = 0;", "VX_KF_ERR_DUP_QUERY);", "a.winner[mt.train_idx] == k",
                 "m->kf_valid_cnt.push_back(n_new)", "h.next_landmark_id = b.first_id() +"):
        hits = [f for f in os.listdir(csrc) if rule in rd(f)]
        assert len(hits) == 1, (rule, hits)
    # ... and the host side fills their argument record and sizes a depth image by one statement each
    for rule in ("a.first_id = ", "a.has_depth = ", "a.nf_last = ", "a.n_obs0 = ",                # KfArgs' filler
                 "(size_t)row_stride * (rows - 1) + (size_t)cols * depth_elem(type)",            # depth_bytes
                 "row_stride < (int64_t)cols * depth_elem(depth_type)"):                         # check_depth
        hits = [f for f in os.listdir(csrc) if rule in rd(f)]
        assert hits == ["keyframe_bodies.hpp"], (rule, hits)
    hits = [f for f in os.listdir(csrc) if "size_t align64(" in rd(f)]
    assert hits == ["vx_internal.hpp"], hits


def rig_scene(sizes, depth, last, seed=64):
    """a 6-keyframe / 300-landmark map with one more last keyframe per camera (distinct ids), and the
    cameras: (map, cameras, first free landmark id)"""
    m = synth.make_cull_scene(seed, 6, 300, special=False)
    scenes = [R.scene(n, True) for n in sizes]
    base = int(m["kf_id"].max()) + 1
    lasts = RR.with_last_keyframes(m, scenes, base)
    cams = [RR.camera(d, base + 100 + i, lasts[i], depth=depth[i], last=last[i]) for i, d in enumerate(scenes)]
    return m, cams, int(m["lm_id"].max()) + 1


def test_chaining_equals_single_calls():
    m, cams, first = rig_scene([300, 65, 63, 1], [True, False, True, False], [True, True, False, False])
    single = m.copy()
    want, nxt = [], first
    for k in cams:
        r = R.create_keyframe(single, k["kf_id"], k["pose7"], k["intr4"], k["uv"], k["last_kf_id"], k["matches"],
                              k["depth"], nxt)
        assert r["error_bits"] == 0
        want.append(r)
        nxt += len(r["landmarks"])
    got = RR.create_keyframes_rig(m, cams, first)
    assert got["error_bits"] == [0, 0, 0, 0] and got["next_landmark_id"] == nxt
    assert got["first"] == [first + sum(len(w["landmarks"]) for w in want[:i]) for i in range(4)]
    assert got["landmarks"].tobytes() == np.concatenate([w["landmarks"] for w in want]).tobytes()
    # not vacuous: depth landmarks, triangulated ones, and a camera that makes none
    assert want[0]["n_depth"] > 0 and want[0]["n_triangulated"] > 0 and want[1]["n_triangulated"] > 0
    assert want[2]["n_depth"] > 0 and want[2]["n_triangulated"] == 0 and len(want[3]["landmarks"]) == 0
    assert set(m.keys()) == set(single.keys())
    for k in m:
        assert np.array_equal(m[k], single[k]), k


@pytest.mark.parametrize("case", ["dup_query_middle", "train_range_last", "repeat_last", "repeat_kf", "last_is_new",
                                  "kf_live", "id_range"])
def test_a_fault_leaves_the_dict_untouched(case):
    m, cams, first = rig_scene([300, 65, 63], [True, True, False], [True, True, True])
    want = [0, 0, 0]
    if case == "dup_query_middle":
        mt = cams[1]["matches"].copy()
        mt["query_idx"][5] = mt["query_idx"][2]
        cams[1]["matches"] = mt
        want[1] = R.ERR_DUP_QUERY
    elif case == "train_range_last":
        mt = cams[2]["matches"].copy()
        mt["train_idx"][-1] = len(cams[2]["uv"])
        cams[2]["matches"] = mt
        want[2] = R.ERR_MATCH_RANGE
    elif case == "repeat_last":
        cams[2]["last_kf_id"] = cams[0]["last_kf_id"]
        want[0] = want[2] = RR.ERR_RIG_REPEAT
    elif case == "repeat_kf":
        cams[1]["kf_id"] = cams[0]["kf_id"]
        want[0] = want[1] = RR.ERR_RIG_REPEAT
    elif case == "last_is_new":
        cams[2]["last_kf_id"] = cams[0]["kf_id"]
        want[2] = R.ERR_NO_LAST
    elif case == "kf_live":
        cams[0]["kf_id"] = int(m["kf_id"][0])
        want[0] = R.ERR_KF_LIVE
    else:
        first = int(m["lm_id"].max()) - 3  # the range's first ids are in the map
        want = [RR.ERR_ID_RANGE] * 3
    before = m.copy()
    got = RR.create_keyframes_rig(m, cams, first)
    assert got["error_bits"] == want and got["landmarks"] is None and got["next_landmark_id"] == first
    assert set(m.keys()) == set(before.keys())
    for k in m:
        assert np.array_equal(m[k], before[k]), k
