"""synth.make_sequence (the frame sequence tests/test_gpu_frontend_adapter.py feeds visionx::Tracking) on
the CPU: what it promises the tracker's adapters — float positions in a permuted order, descriptors a few
bits from the point's base row, the depth pixel CreateLandmarksFromDepth reads, an image that passes the
quality gate, centres one unit apart — and its garbage / dark options."""
import numpy as np

from vxslam import synth

import init_ref as R

KW = dict(width=320, height=240, intr=(260.0, 260.0, 160.0, 120.0))


def test_sequence_shape_and_determinism():
    a = synth.make_sequence(5, 6, 350, **KW)
    b = synth.make_sequence(5, 6, 350, **KW)
    assert len(a["frames"]) == 6
    for fa, fb in zip(a["frames"], b["frames"]):
        for k in ("xy", "desc", "point", "depth", "img", "pose"):
            assert np.array_equal(fa[k], fb[k]), k
        n = len(fa["xy"])
        assert 300 <= n <= 400
        assert fa["xy"].dtype == np.float32 and fa["desc"].shape == (n, 32) and fa["depth"].shape == (240, 320)
        assert len(np.unique(fa["point"])) == n and not np.all(np.diff(fa["point"]) > 0)   # permuted
        assert R.init_gate_ref(fa["img"], fa["xy"])["status"] == R.INIT_OK
    # camera centres exactly one unit apart (the unit translation of InitWithSecondFrame)
    c = [-synth.quat_to_mat(f["pose"][:4]).T @ f["pose"][4:] for f in a["frames"]]
    assert np.allclose(np.linalg.norm(np.diff(c, axis=0), axis=1), 1.0, atol=1e-12)


def test_views_of_a_point_match_and_carry_its_depth():
    s = synth.make_sequence(7, 3, 350, **KW)
    f0, f1 = s["frames"][0], s["frames"][1]
    common, i0, i1 = np.intersect1d(f0["point"], f1["point"], return_indices=True)
    assert len(common) > 250
    dist = np.unpackbits(f0["desc"][i0] ^ f1["desc"][i1], axis=1).sum(1)
    assert dist.max() <= 20   # two views: at most 2 * max_flips apart (the filter of :299 keeps <= 30)
    other = np.unpackbits(f0["desc"][i0] ^ f1["desc"][np.roll(i1, 1)], axis=1).sum(1)
    assert other.min() > 60
    disp = np.linalg.norm(f0["xy"][i0] - f1["xy"][i1], axis=1)
    assert disp.mean() > 10.0   # NeedNewKeyFrame's parallax gate (tracking.h:28) is within reach
    # the depth pixel CreateLandmarksFromDepth reads holds round(z * 5000) for about half of the features
    fx, fy, cx, cy = s["intr"]
    px = (f1["xy"].astype(np.float64) + 0.5).astype(np.int64)
    d = f1["depth"][px[:, 1], px[:, 0]]
    assert 0.35 < np.count_nonzero(d) / len(d) < 0.65
    Rm, t = synth.quat_to_mat(f1["pose"][:4]), f1["pose"][4:]
    z = (s["points"][f1["point"]] @ Rm.T + t)[:, 2]
    has = d > 0
    assert np.array_equal(d[has], np.round(z[has] * 5000.0).astype(np.uint16))
    assert np.count_nonzero(f1["depth"]) == np.count_nonzero(has)


def test_garbage_and_dark_frames():
    s = synth.make_sequence(5, 4, 350, garbage=(2,), dark=(1,), **KW)
    clean = synth.make_sequence(5, 4, 350, **KW)
    g, c = s["frames"][2], clean["frames"][2]
    assert len(g["xy"]) == len(c["xy"]) and not np.array_equal(g["desc"], c["desc"])
    nearest = np.unpackbits(g["desc"][:50, None, :] ^ s["frames"][1]["desc"][None, :, :], axis=2).sum(2).min(1)
    assert nearest.min() > 60   # nothing matches
    assert not s["frames"][1]["img"].any() and np.array_equal(s["frames"][1]["xy"], clean["frames"][1]["xy"])
    assert R.init_gate_ref(s["frames"][1]["img"], s["frames"][1]["xy"])["status"] == R.INIT_POOR_IMAGE
    assert np.array_equal(s["frames"][3]["img"], clean["frames"][3]["img"])
