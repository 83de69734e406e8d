"""Device-resident frames (vx_frame_*, csrc/frame.hip) on the GPU: a captured frame outlives its slot and
equals the extraction's vx_orb_fetch byte for byte; k_frame_capture's byte-range copy at every head /
tail size (a block of n 20-byte rows has 20 n mod 16 != 0 for odd n) and at the capacities around the
count; the host-image and host-feature forms; the fetch's capacity rules.  Everything is a copy, so
every bar is equality."""
import ctypes as C

import numpy as np
import pytest

import vxslam
from vxslam import synth

pytestmark = pytest.mark.gpu

W, H = 320, 240


def dev(a):
    """numpy array -> device bytes (a torch tensor, kept by the caller)"""
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


@pytest.fixture(scope="module")
def images():
    return synth.make_frames(0x5EED0031, 2, H, W)


@pytest.fixture(scope="module")
def params():
    return vxslam.default_orb_params(n_features=400)


@pytest.fixture(scope="module")
def extracted(ctx, images, params):
    """vx_orb_extract of both images (the yardstick), computed once"""
    return [ctx.orb_extract(im, params) for im in images]


def extract_into_slot(ctx, d_img, params, slot):
    ctx.orb_extract_async(d_img.data_ptr(), W, H, 3, W * 3, slot, params)


def test_capture_outlives_the_slot(ctx, images, params, extracted):
    (k0, d0), (k1, d1) = extracted
    n = len(k0)
    assert 300 <= n and not np.array_equal(k0[:50], k1[:50])
    d = dev(images)
    f = vxslam.Frame(ctx, n + 1)
    extract_into_slot(ctx, d[0], params, 1)
    f.capture(ctx, 1)
    sk, sd = ctx.orb_fetch(1)
    extract_into_slot(ctx, d[1], params, 1)  # the slot now holds the other image
    k, de, ov = f.fetch(ctx, overflow=True)
    assert ov == 0 and len(k) == n
    assert k.tobytes() == sk.tobytes() == k0.tobytes() and de.tobytes() == sd.tobytes() == d0.tobytes()
    k2, d2 = ctx.orb_fetch(1)
    assert k2.tobytes() == k1.tobytes() and d2.tobytes() == d1.tobytes()
    f.close()


@pytest.mark.parametrize("delta", [1, 0, -1, None])
def test_capture_capacities(ctx, images, params, extracted, delta):
    """frame capacities n + 1, n, n - 1 and 1 around the extraction's count n"""
    k0, d0 = extracted[0]
    n = len(k0)
    cap = 1 if delta is None else n + delta
    d = dev(images[0])
    extract_into_slot(ctx, d, params, 2)
    f = vxslam.Frame(ctx, cap).capture(ctx, 2)
    k, de, ov = f.fetch(ctx, overflow=True)
    m = min(n, cap)
    assert len(k) == m and ov == int(n > cap)
    assert k.tobytes() == k0[:m].tobytes() and de.tobytes() == d0[:m].tobytes()
    # the device count is the kept count, never more than the rows behind it
    cnt = np.zeros(4, np.int32)
    ctx.synchronize()
    assert vxslam.lib().hipMemcpy(C.c_void_p(cnt.ctypes.data), C.c_void_p(f.device()["count"]), C.c_size_t(16), C.c_int(2)) == 0
    assert list(cnt) == [m, int(n > cap), 0, 0]
    f.close()


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 64, 65])
def test_row_blocks_head_and_tail(ctx, n):
    """uploaded rows fetched back: 20 n bytes of keypoints end (n mod 4) * 4 bytes past a 16-byte boundary"""
    rng = np.random.default_rng(100 + n)
    xy = rng.uniform(0, 300, (n, 2)).astype(np.float32)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    f = vxslam.Frame(ctx, 65).upload(ctx, xy, desc)
    k, de, ov = f.fetch(ctx, overflow=True)
    assert len(k) == n and ov == 0
    assert np.array_equal(np.stack([k["x"], k["y"]], -1).reshape(-1, 2), xy) and np.array_equal(de, desc)
    assert not k["response"].any() and not k["angle"].any() and not k["octave"].any()
    # the same rows as a frame of exactly n rows (n >= 1): the block ends where the rows end
    if n:
        g = vxslam.Frame(ctx, n).upload(ctx, xy, desc)
        k2, d2 = g.fetch(ctx)
        assert k2.tobytes() == k.tobytes() and d2.tobytes() == de.tobytes()
        g.close()
    f.close()


@pytest.mark.parametrize("rows", [1, 3, 4, 5, 64, 65])
def test_capture_row_blocks(ctx, images, params, extracted, rows):
    """k_frame_capture itself at exactly `rows` rows (a frame of that capacity keeps the slot's first
    rows): 20 * rows bytes of keypoints end 4, 12, 0, 4, 0, 4 bytes past a 16-byte boundary"""
    k0, d0 = extracted[0]
    d = dev(images[0])
    extract_into_slot(ctx, d, params, 0)
    f = vxslam.Frame(ctx, rows).capture(ctx, 0)
    k, de, ov = f.fetch(ctx, overflow=True)
    assert len(k) == rows and ov == 1
    assert k.tobytes() == k0[:rows].tobytes() and de.tobytes() == d0[:rows].tobytes()
    f.close()


def test_extract_host_equals_orb_extract(ctx, images, params, extracted):
    f = vxslam.Frame(ctx, 1024)
    for im, (k0, d0) in zip(images, extracted):
        f.extract_host(ctx, im, params)
        k, de = f.fetch(ctx)
        assert k.tobytes() == k0.tobytes() and de.tobytes() == d0.tobytes()
    # a strided (non-contiguous rows) image gives the same
    wide = np.zeros((H, W + 7, 3), np.uint8)
    wide[:, :W] = images[0]
    view = wide[:, :W]
    params_ = params
    rc = vxslam.lib().vx_frame_extract_host_async(ctx.handle, f.handle, C.byref(params_), C.c_void_p(view.ctypes.data), W, H, 3,
                                                  C.c_int64(view.strides[0]))
    assert rc == vxslam.VX_OK
    k, de = f.fetch(ctx)
    assert k.tobytes() == extracted[0][0].tobytes() and de.tobytes() == extracted[0][1].tobytes()
    f.close()


def test_fetch_without_descriptors_and_capacity(ctx, images, params, extracted):
    k0, d0 = extracted[0]
    f = vxslam.Frame(ctx, 1024).extract_host(ctx, images[0], params)
    k, de = f.fetch(ctx, descriptors=False)
    assert de is None and k.tobytes() == k0.tobytes()
    with pytest.raises(vxslam.VxError) as e:
        f.fetch(ctx, cap=len(k0) - 1)
    assert e.value.code == vxslam.VX_ERR_CAPACITY
    n = C.c_int(0)
    kp = np.zeros(4, vxslam.KEYPOINT_DTYPE)
    rc = vxslam.lib().vx_frame_fetch(ctx.handle, f.handle, C.c_void_p(kp.ctypes.data), None, 4, C.byref(n))
    assert rc == vxslam.VX_ERR_CAPACITY and n.value == len(k0)
    # count only
    rc = vxslam.lib().vx_frame_fetch(ctx.handle, f.handle, None, None, 0, C.byref(n))
    assert rc == vxslam.VX_OK and n.value == len(k0)
    f.close()


def test_upload_round_trip_and_capacity(ctx):
    rng = np.random.default_rng(7)
    cap = 37
    f = vxslam.Frame(ctx, cap)
    k, de = f.fetch(ctx)
    assert len(k) == 0 and len(de) == 0  # a new frame is empty
    for n in (cap, 0, 12):
        xy = rng.uniform(0, 300, (n, 2)).astype(np.float32)
        desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        k, de = f.upload(ctx, xy, desc).fetch(ctx)
        assert len(k) == n and np.array_equal(de, desc)
        assert np.array_equal(np.stack([k["x"], k["y"]], -1).reshape(-1, 2), xy)
    xy = np.zeros((cap + 1, 2), np.float32)
    with pytest.raises(vxslam.VxError):
        f.upload(ctx, xy, np.zeros((cap + 1, 32), np.uint8))
    rc = vxslam.lib().vx_frame_upload_async(ctx.handle, f.handle, C.c_void_p(xy.ctypes.data), C.c_void_p(xy.ctypes.data), cap + 1)
    assert rc == vxslam.VX_ERR_CAPACITY
    k, de = f.fetch(ctx)
    assert len(k) == 12  # the refused upload changed nothing
    f.close()


def test_argument_checks(ctx):
    L = vxslam.lib()
    h = C.c_void_p()
    assert L.vx_frame_create(ctx.handle, 0, C.byref(h)) == vxslam.VX_ERR_INVALID and not h
    f = vxslam.Frame(ctx, 8)
    assert L.vx_frame_capture_async(ctx.handle, 9, f.handle) == vxslam.VX_ERR_STATE
    assert L.vx_frame_capture_async(ctx.handle, 0, None) == vxslam.VX_ERR_INVALID
    assert L.vx_frame_upload_async(ctx.handle, f.handle, None, None, 3) == vxslam.VX_ERR_INVALID
    assert L.vx_frame_upload_async(ctx.handle, f.handle, None, None, 0) == vxslam.VX_OK
    p = vxslam.default_orb_params()
    img = np.zeros((H, W), np.uint8)
    assert L.vx_frame_extract_host_async(ctx.handle, f.handle, C.byref(p), C.c_void_p(img.ctypes.data), W, H, 2, C.c_int64(W)) == vxslam.VX_ERR_INVALID
    assert L.vx_frame_extract_host_async(ctx.handle, f.handle, C.byref(p), C.c_void_p(img.ctypes.data), W, H, 1, C.c_int64(W - 1)) == vxslam.VX_ERR_INVALID
    d = f.device()
    assert d["stride"] == 20 and d["cap"] == 8 and d["xy"] == d["count"] + 16 and d["desc"] == d["xy"] + 160
    ctx.synchronize()
    f.close()


def test_profile_shows_the_capture(ctx, images, params):
    d = dev(images[0])
    extract_into_slot(ctx, d, params, 0)
    ctx.synchronize()
    f = vxslam.Frame(ctx, 512)
    ctx.prof_enable(True)
    f.capture(ctx, 0)
    f.fetch(ctx)
    prof = ctx.prof_read()
    ctx.prof_enable(False)
    assert prof["frame_capture"][1] == 1 and prof["frame_capture"][0] > 0.0
    f.close()
