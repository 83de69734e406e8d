"""CPU pins of tests/init_ref.py: the numpy restatement of Tracking::InitWithFirstFrame's gates
(core/frontend/tracking.cpp:93-139, :177-204) that tests/test_gpu_init_gate.py holds csrc/init_gate.hip
to, and the Python restatement of the tracking state machine (:39-89, :459-499, :562-575) that
tests/test_gpu_frontend_adapter.py holds visionx::Tracking to."""
import numpy as np

from vxslam import synth

import init_ref as R
from init_ref import INIT, TRACKING_BAD, TRACKING_GOOD, StateMachine


def spread(n, w, h):
    """n float positions covering every cell of the 5 x 5 grid"""
    i = np.arange(n)
    return np.stack([(i % 25 % 5 + 0.5) * w / 5, (i % 25 // 5 + 0.5) * h / 5], -1).astype(np.float32)


# ---------------------------------------------------------------------------- gray
def test_gray_equals_the_pyramid_level0(oracle):
    f3 = synth.make_frames(3, 2, h=60, w=83)[0]
    rng = np.random.default_rng(5)
    f4 = rng.integers(0, 256, (31, 47, 4), dtype=np.uint8)
    for img in (f3, f4):
        assert np.array_equal(R.gray(img), oracle.pyramid(img)[0])
    g = rng.integers(0, 256, (9, 13), dtype=np.uint8)
    assert R.gray(g) is g


def test_texture_frame_passes_the_quality_gate():
    f = synth.make_frames(3, 2)[0]
    mean, std = R.mean_stddev(*R.sums(R.gray(f)))
    assert abs(mean - 111.7) < 0.05 and abs(std - 49.3) < 0.05
    assert R.init_gate_ref(f, spread(100, 640, 480))["status"] == R.INIT_OK


# ---------------------------------------------------------------------------- scale edge
def half_195_255(w, h):
    """half the pixels 195, half 255 (an odd count: the middle one 225, so the integer mean stays 225)"""
    g = np.full(w * h, 195, np.uint8)
    g[w * h // 2:] = 255
    if (w * h) % 2:
        g[w * h // 2] = 225
    return g.reshape(h, w)


def test_scale_edge_multiplies_by_the_reciprocal():
    g = half_195_255(640, 480)
    n, s, q = R.sums(g)
    assert s == 225 * n and q == (225 * 225 + 30 * 30) * n  # integer mean exactly 225, stddev 30
    mean, std = R.mean_stddev(n, s, q)
    assert mean == 225.00000000000003 and mean > 225.0  # 225 * N * (1 / N)
    assert np.float64(s) / np.float64(n) == 225.0        # a division would pass the gate
    assert abs(std - 30.0) < 1e-6
    assert R.init_gate_ref(g, spread(100, 640, 480))["status"] == R.INIT_POOR_IMAGE
    # the same pattern at 37 x 5 (185 pixels: the middle one 225) and at 37 x 6 (an even count, exact
    # halves) passes: there 225 * N * (1 / N) rounds to 225
    for w, h in ((37, 5), (37, 6)):
        g2 = half_195_255(w, h)
        n2, s2, q2 = R.sums(g2)
        assert s2 == 225 * n2
        assert R.mean_stddev(n2, s2, q2)[0] == 225.0
        assert R.init_gate_ref(g2, spread(100, w, h))["status"] == R.INIT_OK


# ---------------------------------------------------------------------------- grid edges
def edge_positions(w):
    return np.array([0, w / 5, 2 * w / 5, w - 1, w, -0.3], np.float32)


def test_grid_edges():
    for w, want in ((640, [0, 1, 2, 4, 4, 0]), (37, [0, 1, 2, 4, 4, 0]), (641, [0, 0, 1, 4, 4, 0])):
        x = edge_positions(w)
        col, _ = R.grid_cells(np.stack([x, np.zeros_like(x)], -1), w, 480)
        assert col.tolist() == want, (w, col)
        _, row = R.grid_cells(np.stack([np.zeros_like(x), x], -1), 640, w)
        assert row.tolist() == want, (w, row)


def test_occupancy_threshold():
    img = synth.make_frames(3, 1, h=48, w=64)[0]
    for cells, status in ((12, R.INIT_POOR_DISTRIBUTION), (13, R.INIT_OK)):
        xy = np.repeat(spread(25, 64, 48)[:cells], 5, axis=0)
        r = R.init_gate_ref(img, xy)
        assert r["n_features"] == 5 * cells and r["valid_grids"] == cells and r["status"] == status
        assert bin(int(r["grid_mask"])).count("1") == cells


def test_gate_order_and_fields():
    dark = np.zeros((48, 64, 3), np.uint8)
    r = R.init_gate_ref(dark, spread(10, 64, 48)[:1])  # fails all three
    assert r["status"] == R.INIT_FEW_FEATURES and r["valid_grids"] == 1 and r["mean"] == 0.0 and r["stddev"] == 0.0
    r = R.init_gate_ref(dark, np.repeat(spread(25, 64, 48)[:3], 20, axis=0))
    assert r["status"] == R.INIT_POOR_DISTRIBUTION
    r = R.init_gate_ref(dark, spread(60, 64, 48))
    assert r["status"] == R.INIT_POOR_IMAGE and r["n_pixels"] == 64 * 48
    # bit = col * rows + row
    r = R.init_gate_ref(dark, np.array([[63.0, 0.0]], np.float32))
    assert r["grid_mask"] == 1 << (4 * 5 + 0)


# ---------------------------------------------------------------------------- the state machine
GOOD = {"track": True, "inliers": 80, "parallax": 2.0}


def run(sm, outcomes, first_id=0):
    return [sm.step(first_id + i, o) for i, o in enumerate(outcomes)]


def test_state_machine_good_fail_bad_init():
    sm = StateMachine()
    got = run(sm, [{"gate": False}, {"gate": True}, {"init": False}, {"init": True, "inliers": 90, "parallax": 4.0},
                   GOOD, {"track": False}, {}, {"gate": True}, {"init": True, "inliers": 40, "parallax": 1.0}, GOOD])
    assert [s for s, _ in got] == [INIT, INIT, INIT, TRACKING_GOOD, TRACKING_GOOD, TRACKING_BAD, INIT, INIT,
                                   TRACKING_GOOD, TRACKING_GOOD]
    assert not any(k for _, k in got)
    assert sm.resets == 1 and sm.init_frame == 7 and sm.last_keyframe == 8 and sm.last_frame == 9


def test_state_machine_failed_track_keeps_last_frame():
    sm = StateMachine()
    run(sm, [{"gate": True}, {"init": True, "inliers": 90, "parallax": 4.0}, GOOD])
    assert sm.last_frame == 2
    assert sm.step(3, {"track": False}) == (TRACKING_BAD, False)
    assert sm.last_frame == 2 and sm.last_inliers == 80  # returned before :88
    assert sm.step(4, {}) == (INIT, False)
    assert (sm.init_frame, sm.last_frame, sm.last_keyframe, sm.last_inliers, sm.last_parallax) == (None, None, None, 0, 0.0)


def test_state_machine_keyframe_gap():
    sm = StateMachine(min_keyframe_gap=3)
    kf = {"track": True, "inliers": 80, "parallax": 12.0}
    got = run(sm, [{"gate": True}, {"init": True, "inliers": 90, "parallax": 20.0}, kf, kf, kf, kf, kf, kf, kf])
    # init at frame 1 is never a keyframe decision (just_initialized); then ids 4 and 7: gap 3 from 1 and 4
    assert [k for _, k in got] == [False, False, False, False, True, False, False, True, False]
    assert sm.last_keyframe == 7


def test_state_machine_inlier_and_parallax_gates():
    sm = StateMachine(min_keyframe_gap=1)
    init = [{"gate": True}, {"init": True, "inliers": 90, "parallax": 20.0}]
    got = run(sm, init + [{"track": True, "inliers": 49, "parallax": 50.0},    # < min_keyframe_inliers
                          {"track": True, "inliers": 50, "parallax": 9.999},   # < min_parallax
                          {"track": True, "inliers": 50, "parallax": 10.0},    # both at their bounds
                          {"track": True, "inliers": 29, "parallax": 50.0},    # < min_inliers: BAD, no keyframe
                          {}])
    assert got[2:] == [(TRACKING_GOOD, False), (TRACKING_GOOD, False), (TRACKING_GOOD, True), (TRACKING_BAD, False),
                       (INIT, False)]
    # a weak initialisation goes straight to TRACKING_BAD (UpdateTrackingState, :58)
    sm = StateMachine()
    assert run(sm, [{"gate": True}, {"init": True, "inliers": 29, "parallax": 20.0}])[-1] == (TRACKING_BAD, False)
