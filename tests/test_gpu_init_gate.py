"""GPU parity of InitWithFirstFrame's gates on the device (vx_init_gate_async / vx_init_gate_host_async /
vx_init_gate_fetch, csrc/init_gate.hip) against the numpy restatement tests/init_ref.py (pinned by
tests/test_init_gate_cpu.py).

Bar: the whole record byte for byte — status, n_features, valid_grids, grid_mask, n_pixels, sum, sum_sq
are integers, and mean / stddev are the same IEEE operations on both sides (the bar would be 1e-12
relative, as for the composed pose of tests/test_gpu_track_essential.py; equality is asserted and any
difference printed first).

Shapes: the smallest at which k_init_sums can go wrong — rows whose base is off a 16-byte boundary by
1 and 3 bytes, row padding, widths below one vector group (1), a single row, 4 channels at a width
that leaves a tail, more workgroups than one, and 1024 x 1024 of value 255, whose sum of squares
(6.8e10) exceeds 32 bits."""
import numpy as np
import pytest

import vxslam
from vxslam import synth

import init_ref as R

pytestmark = pytest.mark.gpu


def dev(a, offset=0):
    """numpy array -> device bytes `offset` bytes into a torch tensor (kept by the caller); padded, so
    the pointer is never NULL"""
    import torch

    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.from_numpy(np.concatenate([np.zeros(offset, np.uint8), b, np.zeros(16, np.uint8)])).cuda()
    torch.cuda.synchronize()
    return t


def make_image(seed, w, h, ch, pad, value=None):
    """(raw rows h x (w * ch + pad), the logical image as a strided view of them)"""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, (h, w * ch + pad), dtype=np.uint8)
    if value is not None:
        raw[:] = value
    img = raw[:, :w * ch].reshape(h, w) if ch == 1 else raw[:, :w * ch].reshape(h, w, ch)
    return raw, img


def spread(n, w, h, seed=0):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-1, w + 1, n), rng.uniform(-1, h + 1, n)], -1).astype(np.float32)


def gate_dev(ctx, raw, w, h, ch, offset, xy, *, n_dev=None, cap=None, xy_stride=8, opts=None):
    """the device-input call on explicit buffers"""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    rows = np.zeros((max(len(xy), 1), xy_stride // 4), np.float32)
    rows[:len(xy), :2] = xy
    keep = (dev(raw, offset), dev(rows), dev(np.array([len(xy) if n_dev is None else n_dev], np.int32)))
    ctx.init_gate_async(keep[0].data_ptr() + offset, w, h, ch, raw.shape[1], (keep[1].data_ptr(), xy_stride, keep[2].data_ptr()),
                        opts, cap_feat=len(xy) if cap is None else cap)
    out = ctx.init_gate_fetch()
    del keep
    return out


def assert_same(got, ref, what=""):
    for k in R.RESULT_DTYPE.names:
        if got[k] != ref[k]:
            print(what, k, got[k], ref[k], (float(got[k]) - float(ref[k])) / max(abs(float(ref[k])), 1e-300))
    assert got.tobytes() == ref.tobytes(), (what, got, ref)


def test_layout_and_defaults():
    assert vxslam.INIT_GATE_RESULT_DTYPE.itemsize == R.RESULT_DTYPE.itemsize == 56
    assert vxslam.INIT_GATE_RESULT_DTYPE.names == R.RESULT_DTYPE.names
    o = vxslam.init_gate_options()
    assert {k: o[k].item() for k in R.DEFAULTS} == R.DEFAULTS
    assert (vxslam.INIT_OK, vxslam.INIT_FEW_FEATURES, vxslam.INIT_POOR_DISTRIBUTION, vxslam.INIT_POOR_IMAGE) == (
        R.INIT_OK, R.INIT_FEW_FEATURES, R.INIT_POOR_DISTRIBUTION, R.INIT_POOR_IMAGE)


# ---------------------------------------------------------------------------- images
IMAGES = [(640, 480, 3, 0, 0), (37, 5, 3, 5, 1), (1, 1, 1, 0, 0), (64, 1, 3, 0, 0), (641, 3, 4, 0, 0),
          (130, 67, 1, 3, 3), (1024, 1024, 1, 0, 0)]


@pytest.mark.parametrize("w,h,ch,pad,offset", IMAGES)
def test_images(ctx, w, h, ch, pad, offset):
    if (w, h, ch) == (640, 480, 3):
        img = synth.make_frames(3, 1)[0]
        raw = img.reshape(h, w * ch)
    else:
        raw, img = make_image(w * 7 + h, w, h, ch, pad, value=255 if w == 1024 else None)
    xy = spread(200, w, h, seed=w)
    ref = R.init_gate_ref(img, xy)
    if w == 1024:
        assert ref["sum_sq"] == 1024 * 1024 * 255 * 255 > 2 ** 32 and ref["status"] == R.INIT_POOR_IMAGE
    assert_same(gate_dev(ctx, raw, w, h, ch, offset, xy), ref, "device")
    assert_same(ctx.init_gate_host(img, xy), ref, "host")


def test_four_channels_off_a_pixel_boundary(ctx):
    """a 4-channel row whose base is not a multiple of 4 never reaches a 16-byte pixel boundary: the
    byte path for the whole row, over more than one workgroup column"""
    raw, img = make_image(11, 700, 3, 4, 6)
    xy = spread(60, 700, 3)
    for offset in (1, 2, 4):
        assert_same(gate_dev(ctx, raw, 700, 3, 4, offset, xy), R.init_gate_ref(img, xy), offset)


def test_scale_edge(ctx):
    """half 195, half 255: the integer mean is exactly 225, and 225 * N * (1 / N) is above it at 640 x 480"""
    for w, h, status in ((640, 480, R.INIT_POOR_IMAGE), (37, 6, R.INIT_OK), (37, 5, R.INIT_OK)):
        g = np.full(w * h, 195, np.uint8)
        g[w * h // 2:] = 255
        if (w * h) % 2:
            g[w * h // 2] = 225
        g = g.reshape(h, w)
        xy = spread(300, w, h)
        ref = R.init_gate_ref(g, xy)
        assert ref["status"] == status and ref["sum"] == 225 * w * h
        assert_same(ctx.init_gate_host(g, xy), ref, (w, h))
        assert_same(gate_dev(ctx, g, w, h, 1, 0, xy), ref, (w, h))


# ---------------------------------------------------------------------------- keypoints
@pytest.fixture(scope="module")
def frame():
    return synth.make_frames(3, 1, h=48, w=64)[0]


@pytest.mark.parametrize("n", [0, 1, 49, 50, 2000])
def test_feature_counts(ctx, frame, n):
    xy = spread(n, 64, 48, seed=n)
    ref = R.init_gate_ref(frame, xy)
    assert ref["status"] == (R.INIT_FEW_FEATURES if n < 50 else R.INIT_OK)
    assert_same(gate_dev(ctx, frame.reshape(48, -1), 64, 48, 3, 0, xy), ref)
    assert_same(gate_dev(ctx, frame.reshape(48, -1), 64, 48, 3, 0, xy, xy_stride=20), ref)
    assert_same(ctx.init_gate_host(frame, xy), ref)


def test_grid_edges(ctx):
    for w, want in ((640, [0, 1, 2, 4, 4, 0]), (37, [0, 1, 2, 4, 4, 0]), (641, [0, 0, 1, 4, 4, 0])):
        x = np.array([0, w / 5, 2 * w / 5, w - 1, w, -0.3], np.float32)
        raw, img = make_image(w, w, 7, 1, 0)
        opts = vxslam.init_gate_options(min_features=1)
        for axis in (0, 1):  # the same list along x of a w-wide image and along y of a w-high one
            xy = np.zeros((6, 2), np.float32)
            xy[:, axis] = x
            im = img if axis == 0 else np.ascontiguousarray(img.T)
            ref = R.init_gate_ref(im, xy, min_features=1)
            cells = sorted(set(want))
            bits = [c * 5 for c in cells] if axis == 0 else cells
            assert int(ref["grid_mask"]) == sum(1 << b for b in bits)
            assert_same(ctx.init_gate_host(im, xy, opts), ref, (w, axis))


def test_occupancy_threshold_and_every_status(ctx, frame):
    cells = np.stack([(np.arange(25) % 5 + 0.5) * 64 / 5, (np.arange(25) // 5 + 0.5) * 48 / 5], -1).astype(np.float32)
    seen = set()
    for k, status in ((12, R.INIT_POOR_DISTRIBUTION), (13, R.INIT_OK)):
        xy = np.repeat(cells[:k], 5, axis=0)
        got = ctx.init_gate_host(frame, xy)
        assert got["status"] == status and got["valid_grids"] == k
        assert_same(got, R.init_gate_ref(frame, xy))
        seen.add(int(got["status"]))
    dark = np.zeros_like(frame)
    got = ctx.init_gate_host(dark, cells[:1])   # fails all three gates: the first in the reference's order
    assert got["status"] == R.INIT_FEW_FEATURES and got["valid_grids"] == 1 and got["mean"] == 0.0
    assert_same(got, R.init_gate_ref(dark, cells[:1]))
    seen.add(int(got["status"]))
    got = ctx.init_gate_host(dark, np.repeat(cells, 3, axis=0))
    assert_same(got, R.init_gate_ref(dark, np.repeat(cells, 3, axis=0)))
    seen.add(int(got["status"]))
    assert seen == {R.INIT_OK, R.INIT_FEW_FEATURES, R.INIT_POOR_DISTRIBUTION, R.INIT_POOR_IMAGE}
    # other grids and bounds
    xy = spread(80, 64, 48)
    for opt in (dict(grid_cols=8, grid_rows=4), dict(grid_cols=1, grid_rows=1), dict(min_grid_frac=0.9),
                dict(min_mean=120.0), dict(max_mean=100.0), dict(min_stddev=60.0), dict(min_features=81)):
        assert_same(ctx.init_gate_host(frame, xy, vxslam.init_gate_options(**opt)), R.init_gate_ref(frame, xy, **opt), opt)


def test_capacity_below_the_device_count(ctx, frame):
    xy = spread(120, 64, 48)
    raw = frame.reshape(48, -1)
    assert_same(gate_dev(ctx, raw, 64, 48, 3, 0, xy, cap=40), R.init_gate_ref(frame, xy[:40]))      # count 120, cap 40
    assert_same(gate_dev(ctx, raw, 64, 48, 3, 0, xy, n_dev=70), R.init_gate_ref(frame, xy[:70]))    # count 70, cap 120
    assert_same(gate_dev(ctx, raw, 64, 48, 3, 0, xy, n_dev=-5), R.init_gate_ref(frame, xy[:0]))     # a negative count
    assert_same(gate_dev(ctx, raw, 64, 48, 3, 0, xy, cap=0), R.init_gate_ref(frame, xy[:0]))


# ---------------------------------------------------------------------------- after an extraction
def test_slot_keypoints_equal_the_host_variant(ctx):
    import torch

    frames = synth.make_frames(41, 2, 240, 320)
    p = vxslam.default_orb_params(n_features=500)
    d = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    ctx.orb_extract_async(d[0].data_ptr(), 320, 240, 3, 320 * 3, 0, p)
    ctx.orb_extract_async(d[1].data_ptr(), 320, 240, 3, 320 * 3, 1, p)   # the scratch now holds frame 1's pyramid
    ctx.init_gate_async(d[0].data_ptr(), 320, 240, 3, 320 * 3, 0)         # slot 0: stride 20, the slot's count
    a = ctx.init_gate_fetch()
    k0, _ = ctx.orb_fetch(0)
    assert a["n_features"] == len(k0) >= 50
    xy = np.stack([k0["x"], k0["y"]], -1)
    b = ctx.init_gate_host(frames[0], xy)
    assert a.tobytes() == b.tobytes()
    assert_same(a, R.init_gate_ref(frames[0], xy))
    assert a["status"] == R.INIT_OK


# ---------------------------------------------------------------------------- state, arguments, profiling
def test_fetch_before_any_call_and_repeats(frame):
    c = vxslam.Context(0)
    try:
        with pytest.raises(vxslam.VxError) as e:
            c.init_gate_fetch()
        assert e.value.code == -5   # VX_ERR_STATE
        xy = spread(90, 64, 48)
        got = [c.init_gate_host(frame, xy).tobytes() for _ in range(3)]
        assert got[0] == got[1] == got[2] == R.init_gate_ref(frame, xy).tobytes()
        assert c.init_gate_fetch().tobytes() == got[0]   # the record stays fetchable
    finally:
        c.close()


def test_invalid_arguments(ctx, frame):
    L = vxslam.lib()
    import ctypes as C

    o = vxslam.init_gate_options()
    keep = (dev(frame), dev(np.zeros((4, 2), np.float32)), dev(np.array([4], np.int32)))
    img, xy, n = (C.c_void_p(k.data_ptr()) for k in keep)
    op = C.c_void_p(o.ctypes.data)

    def call(img=img, w=64, h=48, ch=3, stride=192, xy=xy, xs=8, n=n, cap=4, op=op):
        return L.vx_init_gate_async(ctx.handle, img, w, h, ch, stride, xy, xs, n, cap, op)

    assert call() == 0
    ctx.init_gate_fetch()
    for kw in (dict(img=None), dict(op=None), dict(n=None), dict(xy=None), dict(w=0), dict(h=-1), dict(ch=2), dict(ch=5),
               dict(stride=191), dict(xs=4), dict(xs=10), dict(cap=-1)):
        assert call(**kw) == -1, kw
    for cols, rows in ((0, 5), (5, 0), (6, 6), (33, 1), (-1, -1)):
        bad = vxslam.init_gate_options(grid_cols=cols, grid_rows=rows)
        assert call(op=C.c_void_p(bad.ctypes.data)) == -1, (cols, rows)
    ok = vxslam.init_gate_options(grid_cols=32, grid_rows=1)
    assert call(op=C.c_void_p(ok.ctypes.data)) == 0
    ctx.init_gate_fetch()
    # the host form: the same checks, and a count without positions
    hp = C.c_void_p(frame.ctypes.data)
    hxy = np.zeros((4, 2), np.float32)
    assert L.vx_init_gate_host_async(ctx.handle, hp, 64, 48, 3, 192, C.c_void_p(hxy.ctypes.data), 8, 4, op) == 0
    ctx.init_gate_fetch()
    assert L.vx_init_gate_host_async(ctx.handle, hp, 64, 48, 3, 192, None, 8, 4, op) == -1
    assert L.vx_init_gate_host_async(ctx.handle, hp, 64, 48, 3, 192, None, 8, 0, op) == 0
    ctx.init_gate_fetch()
    assert L.vx_init_gate_host_async(ctx.handle, None, 64, 48, 3, 192, None, 8, 0, op) == -1
    assert L.vx_init_gate_host_async(ctx.handle, hp, 64, 48, 2, 192, None, 8, 0, op) == -1
    assert L.vx_init_gate_fetch(ctx.handle, None) == -1
    del keep


def test_stages_are_profiled(ctx, frame):
    xy = spread(90, 64, 48)
    ctx.prof_enable(True, ["init_sums", "init_gate"])
    try:
        ctx.prof_read()
        ctx.init_gate_host(frame, xy)
        p = ctx.prof_read()
    finally:
        ctx.prof_enable(False)
    assert p["init_sums"][1] == 1 and p["init_sums"][0] > 0.0
    assert p["init_gate"][1] == 1 and p["init_gate"][0] > 0.0
