"""vx_frame_capture_batch_async (csrc/frame.hip) on the GPU: the frames of a batch bank
(vx_orb_extract_batch) into one device-resident frame each in ONE launch.  Everything is a copy, so every
bar is equality with vx_orb_batch_fetch of the same frame, under k_frame_capture's clamping rules."""
import ctypes as C

import numpy as np
import pytest

import vxslam
from vxslam import synth

pytestmark = pytest.mark.gpu

W, H = 320, 240
BANK = 1


@pytest.fixture(scope="module")
def images():
    return synth.make_frames(0x5EED0071, 3, H, W)


@pytest.fixture(scope="module")
def params():
    return vxslam.default_orb_params(n_features=500)


def device_count(ctx, f):
    cnt = np.zeros(4, np.int32)
    ctx.synchronize()
    assert vxslam.lib().hipMemcpy(C.c_void_p(cnt.ctypes.data), C.c_void_p(f.device()["count"]), C.c_size_t(16), C.c_int(2)) == 0
    return list(cnt)


def test_three_frames_in_one_launch(ctx, images, params):
    ctx.orb_extract_batch(np.stack(images), params, bank=BANK)
    want = [ctx.orb_batch_fetch(BANK, i) for i in range(3)]
    assert all(len(k) >= 300 for k, _ in want) and not np.array_equal(want[0][0][:50], want[1][0][:50])
    frames = [vxslam.Frame(ctx, 1024) for _ in range(3)]
    ctx.prof_enable(True)
    ctx.frame_capture_batch(BANK, frames)
    ctx.synchronize()
    prof = ctx.prof_read()
    ctx.prof_enable(False)
    assert prof["frame_capture_batch"][1] == 1 and prof["frame_capture"][1] == 0
    for f, (k0, d0) in zip(frames, want):
        k, d, ov = f.fetch(ctx, overflow=True)
        assert ov == 0 and k.tobytes() == k0.tobytes() and d.tobytes() == d0.tobytes()
    # the first two frames of the bank only: the third handle keeps what it holds
    again = [vxslam.Frame(ctx, 1024) for _ in range(2)]
    ctx.frame_capture_batch(BANK, again)
    for f, (k0, d0) in zip(again, want):
        k, d = f.fetch(ctx)
        assert k.tobytes() == k0.tobytes() and d.tobytes() == d0.tobytes()
    for f in frames + again:
        f.close()


def test_capacities_and_a_blank_frame_in_one_call(ctx, images, params):
    """handle capacities n + 1, n, n - 1 (overflow set, first n - 1 rows) and 1 around the count n, and a blank
    frame (0 rows) in the middle of the batch"""
    blank = np.zeros_like(images[0])
    batch = np.stack([images[0], images[0], blank, images[0], images[0]])
    ctx.orb_extract_batch(batch, params, bank=BANK)
    k0, d0 = ctx.orb_batch_fetch(BANK, 0)
    n = len(k0)
    assert n >= 300 and len(ctx.orb_batch_fetch(BANK, 2)[0]) == 0
    caps = [n + 1, n, 8, n - 1, 1]
    frames = [vxslam.Frame(ctx, c) for c in caps]
    # the blank frame's handle holds rows from before: the capture must leave it empty
    frames[2].upload(ctx, np.ones((5, 2), np.float32), np.full((5, 32), 7, np.uint8))
    ctx.frame_capture_batch(BANK, frames)
    for i, (f, cap) in enumerate(zip(frames, caps)):
        src_n = 0 if i == 2 else n
        m = min(src_n, cap)
        k, d, ov = f.fetch(ctx, overflow=True)
        assert len(k) == m and ov == int(src_n > cap), i
        assert k.tobytes() == k0[:m].tobytes() and d.tobytes() == d0[:m].tobytes(), i
        assert device_count(ctx, f) == [m, int(src_n > cap), 0, 0], i
    for f in frames:
        f.close()


def test_handles_outlive_the_bank(ctx, images, params):
    ctx.orb_extract_batch(np.stack(images[:2]), params, bank=BANK)
    want = [ctx.orb_batch_fetch(BANK, i) for i in range(2)]
    frames = [vxslam.Frame(ctx, len(k) + 3) for k, _ in want]
    ctx.frame_capture_batch(BANK, frames)
    ctx.orb_extract_batch(np.stack(images[::-1]), params, bank=BANK)  # the bank now holds another batch
    assert ctx.orb_batch_fetch(BANK, 0)[0].tobytes() != want[0][0].tobytes()
    for f, (k0, d0) in zip(frames, want):
        k, d = f.fetch(ctx)
        assert k.tobytes() == k0.tobytes() and d.tobytes() == d0.tobytes()
    for f in frames:
        f.close()


def test_argument_and_state_checks(ctx, images, params):
    L = vxslam.lib()
    ctx.orb_extract_batch(np.stack(images[:2]), params, bank=BANK)
    fr = [vxslam.Frame(ctx, 64) for _ in range(3)]
    hs = lambda fs: (C.c_void_p * len(fs))(*[f.handle for f in fs])
    assert L.vx_frame_capture_batch_async(ctx.handle, BANK, 3, hs(fr)) == vxslam.VX_ERR_STATE       # the bank holds 2
    assert L.vx_frame_capture_batch_async(ctx.handle, BANK, 0, hs(fr)) == vxslam.VX_ERR_STATE
    assert L.vx_frame_capture_batch_async(ctx.handle, 7, 1, hs(fr)) == vxslam.VX_ERR_INVALID
    assert L.vx_frame_capture_batch_async(ctx.handle, BANK, 2, None) == vxslam.VX_ERR_INVALID
    assert L.vx_frame_capture_batch_async(ctx.handle, BANK, 2, hs([fr[0], fr[0]])) == vxslam.VX_ERR_INVALID  # one handle twice
    assert L.vx_frame_capture_batch_async(ctx.handle, BANK, 2, (C.c_void_p * 2)(fr[0].handle, None)) == vxslam.VX_ERR_INVALID
    fresh = vxslam.Context(0)
    assert L.vx_frame_capture_batch_async(fresh.handle, 0, 1, hs(fr)) == vxslam.VX_ERR_STATE        # nothing extracted
    fresh.close()
    assert L.vx_frame_capture_batch_async(ctx.handle, BANK, 2, hs(fr)) == vxslam.VX_OK
    assert fr[0].fetch(ctx, overflow=True)[2] == 1 and len(fr[0].fetch(ctx)[0]) == 64
    for f in fr:
        f.close()
