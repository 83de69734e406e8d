"""vx_track_rig_* and vx_frame_capture_batch_async (csrc/track_rig.hip, csrc/frame.hip) without a GPU: the
declarations, exports and bindings, and the packed block's layout function (vx_track_rig_layout: a pure
host function) against a restatement of vx_track_frame_fetch's offset arithmetic."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import vxslam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["vx_track_rig_async", "vx_track_rig_fetch", "vx_track_rig_pairs", "vx_track_rig_keypoints",
         "vx_track_rig_matches", "vx_track_rig_layout", "vx_track_rig_block", "vx_frame_capture_batch_async"]


def a16(x):
    return (int(x) + 15) & ~15


def part(cp0, cp1, ckp):
    """vx_track_frame_fetch's offsets inside one block (csrc/track_frame.hip): result | pair_match0 | mask0 |
    pair_match1 | mask1 | keypoint rows, each part on a 16-byte boundary"""
    o_pm0 = a16(vxslam.TRACK_FRAME_RESULT_DTYPE.itemsize)
    o_mask0 = o_pm0 + a16(cp0 * 4)
    o_pm1 = o_mask0 + a16(cp0)
    o_mask1 = o_pm1 + a16(cp1 * 4)
    o_kp = o_mask1 + a16(cp1)
    return o_pm0, o_mask0, o_pm1, o_mask1, o_kp, o_kp + a16(ckp * vxslam.KEYPOINT_DTYPE.itemsize)


def test_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "vx_slam.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", vxslam.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert re.search(r" T %s$" % n, out, flags=re.M), n
        assert n in vxslam.EXPORTS, n
        assert hasattr(vxslam.lib(), n), n
    assert re.search(r"#define\s+VX_MAX_RIG_CAMERAS\s+16\b", hdr) and re.search(r"\}\s*vx_rig_camera;", hdr)
    assert vxslam.MAX_RIG_CAMERAS == 16
    for n in ("track_rig_async", "track_rig_fetch", "track_rig_matches", "frame_capture_batch"):
        assert hasattr(vxslam.Context, n), n
    assert hasattr(vxslam, "track_rig_layout") and hasattr(vxslam, "rig_camera")
    # vx_rig_camera: six 8-byte fields, no padding
    T = vxslam.RIG_CAMERA_DTYPE
    assert T.itemsize == 48 and T.names == ("last_kf_id", "last_kf", "last", "curr", "pose_last7", "intr4")
    # the new kernels are profiling stages with stable names
    L = vxslam.lib()
    L.vx_prof_name.restype = C.c_char_p
    names = [L.vx_prof_name(i).decode() for i in range(L.vx_prof_count())]
    for n in ("rig_pairs", "rig_pack", "rig_gate", "rig_epairs", "rig_epose", "rig_final", "frame_capture_batch"):
        assert names.count(n) == 1, n
    assert names.index("track_final") < names.index("rig_pairs")  # the existing stages keep their numbers


CAPS = [
    ([300], [320], [303]),
    ([300, 320, 303, 600], [320, 300, 600, 303], [303, 1, 323, 601]),
    ([0, 1, 0, 17, 0], [1, 0, 33, 0, 0], [0, 0, 5, 1, 0]),
    (list(range(1, 17)), list(range(16, 0, -1)), [1025] * 16),
]


@pytest.mark.parametrize("cp0, cp1, ckp", CAPS)
def test_layout_properties(cp0, cp1, ckp):
    off, total = vxslam.track_rig_layout(cp0, cp1, ckp)
    assert len(off) == len(cp0) and off[0] == 0
    end = 0
    for i in range(len(cp0)):
        assert off[i] % 16 == 0                       # every offset is 16-byte aligned
        assert off[i] >= end                          # blocks disjoint and ascending
        end = int(off[i]) + part(cp0[i], cp1[i], ckp[i])[-1]
    assert total == end                               # total_bytes is the end of the last block
    assert total % 16 == 0


def test_layout_of_one_camera_is_the_single_calls():
    for cp0, cp1, ckp in ((320, 320, 323), (0, 300, 300), (1, 1, 1), (1024, 1025, 2000)):
        off, total = vxslam.track_rig_layout([cp0], [cp1], [ckp])
        assert off[0] == 0 and total == part(cp0, cp1, ckp)[-1]
        # a second camera starts where the single call's block ends, so the offsets inside a block are its own
        off2, _ = vxslam.track_rig_layout([cp0, 7], [cp1, 9], [ckp, 11])
        assert off2[1] == total
    assert part(320, 320, 323)[:5] == (560, 560 + 1280, 560 + 1280 + 320, 560 + 1280 + 320 + 1280, 560 + 2 * (1280 + 320))


EDGE = (0, 1, 15, 16, 17)  # where a 16-byte rounding term can go wrong


def test_block_layout_against_the_second_statement():
    """the library's Python statement of a block (vxslam.track_frame_block), this file's (part) and the C
    one (vx_track_rig_layout: the end of a block is where a second camera's begins) agree"""
    cases = [(a, b, k) for cp0, cp1, ckp in CAPS for a, b, k in zip(cp0, cp1, ckp)]
    cases += [(a, b, k) for a in EDGE for b in EDGE for k in EDGE]
    for cp0, cp1, ckp in cases:
        want = part(cp0, cp1, ckp)
        assert vxslam.track_frame_block(cp0, cp1, ckp) == want, (cp0, cp1, ckp)
        off, total = vxslam.track_rig_layout([cp0, 3], [cp1, 5], [ckp, 7])
        assert off[1] == want[-1] and total == want[-1] + part(3, 5, 7)[-1], (cp0, cp1, ckp)
        # without the keypoint rows a block ends where they would begin
        assert vxslam.track_rig_layout([cp0], [cp1], [0])[1] == want[4], (cp0, cp1, ckp)


def test_layout_accepts_zero_capacities():
    off, total = vxslam.track_rig_layout([0, 0], [0, 0], [0, 0])
    head = a16(vxslam.TRACK_FRAME_RESULT_DTYPE.itemsize)
    assert list(off) == [0, head] and total == 2 * head


def test_layout_argument_checks():
    L = vxslam.lib()
    z = np.zeros(32, np.int32)
    off = np.zeros(32, np.int64)
    total = C.c_int64(-1)
    p = lambda a: C.c_void_p(a.ctypes.data)
    for n in (0, -1, 17, 1 << 20):
        assert L.vx_track_rig_layout(n, p(z), p(z), p(z), p(off), C.byref(total)) == vxslam.VX_ERR_INVALID, n
    for n in (1, 16):
        assert L.vx_track_rig_layout(n, p(z), p(z), p(z), p(off), C.byref(total)) == vxslam.VX_OK, n
    assert L.vx_track_rig_layout(2, None, p(z), p(z), p(off), C.byref(total)) == vxslam.VX_ERR_INVALID
    neg = z.copy()
    neg[1] = -1
    for args in ((neg, z, z), (z, neg, z), (z, z, neg)):
        assert L.vx_track_rig_layout(2, *(p(a) for a in args), p(off), C.byref(total)) == vxslam.VX_ERR_INVALID
    # the outputs are optional
    assert L.vx_track_rig_layout(2, p(z), p(z), p(z), None, None) == vxslam.VX_OK
    with pytest.raises(vxslam.VxError):
        vxslam.track_rig_layout([1] * 17, [1] * 17, [1] * 17)


def test_null_arguments_need_no_device():
    L = vxslam.lib()
    assert L.vx_track_rig_async(None, None, 1, None, 0.8, None, None) == vxslam.VX_ERR_INVALID
    assert L.vx_track_rig_fetch(None, 1, None, 0, None) == vxslam.VX_ERR_INVALID
    assert L.vx_track_rig_pairs(None, 0, 0, None, None, 0) == vxslam.VX_ERR_INVALID
    assert L.vx_track_rig_keypoints(None, 0, None, 0, None) == vxslam.VX_ERR_INVALID
    assert L.vx_track_rig_matches(None, 0, 0, None, None, None) == vxslam.VX_ERR_INVALID
    assert L.vx_track_rig_block(None, None, None, None, None, None, 0) == vxslam.VX_ERR_INVALID
    assert L.vx_frame_capture_batch_async(None, 0, 1, None) == vxslam.VX_ERR_INVALID


def test_the_rules_are_stated_once():
    """the single-camera kernels and the rig kernels run the same program text"""
    csrc = os.path.join(ROOT, "visionx-slam_amd", "csrc")
    rd = lambda f: open(os.path.join(csrc, f)).read()
    for f, inc in (("track.hip", "track_pairs_body.inc"), ("track_ess.hip", "track_epairs_body.inc")):
        assert '#include "%s"' % inc in rd(f) and '#include "%s"' % inc in rd("track_rig.hip"), inc
    for fn in ("trk::track_gate(", "trk::track_epose(", "trk::track_final<"):
        assert fn in rd("track_rig.hip") and sum(fn in rd(f) for f in ("track_frame.hip", "track_ess.hip")) == 1, fn
    for rule in ("a.offsets[1] = run ? n_pairs : 0", "a.offsets[1] = enough ? n_pairs : 0", "const bool open = !a.pnp"):
        hits = [f for f in os.listdir(csrc) if rule in rd(f)]
        assert len(hits) == 1, (rule, hits)
    # ... and the host side fills and checks their argument records by one statement each
    # (the map side of TrackArgs: other calls' records have an id table of their own, so among the tracking files)
    hits = [f for f in os.listdir(csrc) if f.startswith("track") and "a.ht_mask = " in rd(f)]
    assert hits == ["track_bodies.hpp"], hits
    for rule in ("return mask(1) + align16((size_t)cap1);",            # the frame block's chain (o_mask1's term)
                 "f.o_mask1 = ",                                       # FinalArgs' offsets
                 "o.max_iterations < 0 ? 100 : o.max_iterations",      # PnP's hypothesis bound
                 "a.opt_out = reinterpret_cast<OptOf<A>*>(prob + kProb1Opt);",  # the single problem record
                 "constexpr size_t kProbOffsets = 0, kProbCnt = 128",  # the batch problem record
                 "g.cap_last = ", "p.pose_last[i] = ", "a.mask = block + off_mask<R>(cap);",
                 "intr4[0] + intr4[1] != 0.0", "bad PnP options", "bad essential options",
                 "neither a last keyframe nor a last frame", "a last keyframe without a map / options",
                 "const int np = which ? r->ess.n_pairs : r->pnp.n_pairs;"):
        hits = [f for f in os.listdir(csrc) if rule in rd(f)]
        assert hits == ["track_bodies.hpp"], (rule, hits)
    # the staged upload (hipEventCreateWithFlags( of a plain hipEventDisableTiming event; vx_ctx.cpp's are the
    # cross-stream ordering events): the helper, and frame.hip's own (it copies into a block it does not own)
    ev = re.compile(r"hipEventCreateWithFlags\(&[^,]+, hipEventDisableTiming\)")
    hits = sorted(f for f in os.listdir(csrc) if ev.search(rd(f)))
    assert hits == ["frame.hip", "vx_internal.hpp"], hits
