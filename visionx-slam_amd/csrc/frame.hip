// frame.hip — a frame's features on the device for as long as the frame lives (vx_frame_*).
//
// The reference's Frame owns the keypoints and descriptors ORBExtractor::Extract copied out of
// detectAndCompute (orb_extractor.cpp:13-24, frame.h:16-40) and hands them to every later step of
// Tracking: Match, TrackWithPnP, TrackLastFrame, CreateKeyFrame.  Here an extraction slot belongs to
// its context and is overwritten by the next extraction into it, so a vx_frame is a block of its own,
//
//   int32 count[4] {n, overflow, 0, 0} | vx_keypoint rows[cap] | descriptor rows[cap] (32 B each)
//
// (both row arrays on 16-byte boundaries), whose pointers are what vx_match_device_async,
// vx_track_pnp_async, vx_track_essential_async and vx_dmap_create_keyframe already take.
//
// k_frame_capture copies a slot's rows into the block.  The count is known on the device only, so the
// grid is sized by min(slot cap, frame cap) and every thread stops at the count.  Keypoint rows are
// 20 bytes, so a row is not a vector: the n rows are copied as ONE byte range of 20 n bytes — a dword
// head up to the first 16-byte boundary (both sides share it: hipMalloc'd bases, offset 16), uint4
// loads and stores over the body, a dword tail of 20 n mod 16 bytes — as k_init_sums treats an image
// row (init_gate.hip; grid_copy_range, vx_rows.hpp).  The descriptor rows are 2 uint4 each.  One item
// (a uint4, or a dword of the head / tail) per thread, grid-stride; no atomics, no LDS; the count is
// written by one lane.
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950): 16 VGPRs, 42 SGPRs, 0 B LDS, 0 B scratch.
//
// The kernel moves 52 n bytes (104 KB at 2000 features): a few hundred nanoseconds of traffic behind
// a launch, so it is bound by launch latency, not bandwidth; the grid (one 256-thread workgroup per
// 256 items) only has to keep that traffic from serialising on one CU.
#include <algorithm>
#include <cstddef>
#include <cstring>

#include "vx_internal.hpp"
#include "vx_rows.hpp"

namespace vx {
namespace {

constexpr int kBlock = 256;
constexpr int kMaxWg = 512;

struct CaptureArgs {
    const uint8_t* src_kp;    // the slot's vx_keypoint rows
    const uint8_t* src_desc;  // its descriptor rows
    const int* src_count;     // {n, overflow}
    int src_cap;
    uint8_t* dst_kp;
    uint8_t* dst_desc;
    int* dst_count;
    int dst_cap;
};

__global__ void __launch_bounds__(kBlock) k_frame_capture(CaptureArgs a) {
    const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x, nt = (size_t)gridDim.x * kBlock;
    const int n_src = min(max(a.src_count[0], 0), a.src_cap);
    const int n = min(n_src, a.dst_cap);
    grid_copy_range(a.dst_kp, a.src_kp, (size_t)n * sizeof(vx_keypoint), t, nt);
    grid_copy_range(a.dst_desc, a.src_desc, (size_t)n * 32, t, nt);
    if (t == 0) {
        a.dst_count[0] = n;
        a.dst_count[1] = (a.src_count[0] > a.dst_cap || a.src_count[1] != 0) ? 1 : 0;
        a.dst_count[2] = 0;
        a.dst_count[3] = 0;
    }
}

// The frames of a batch bank (vx_orb_extract_batch_async: frame-major rows, count of frame f at
// src_count + 4 f) into one handle each in ONE launch: frame = blockIdx.y, and per frame exactly
// k_frame_capture's copy, clamping and flags.  The handles' pointers travel as kernel arguments
// (28 B a frame, 1.8 KB at VX_MAX_BATCH); a frame's row arrays start frame * src_cap rows into the bank,
// so its keypoint range need not share the handle's 16-byte phase (grid_copy_range then moves dwords).
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950): 16 VGPRs, 44 SGPRs, 0 B LDS, 0 B scratch.
struct CaptureBatchArgs {
    const uint8_t* src_kp;
    const uint8_t* src_desc;
    const int* src_count;
    int src_cap;
    uint8_t* dst_kp[VX_MAX_BATCH];
    uint8_t* dst_desc[VX_MAX_BATCH];
    int* dst_count[VX_MAX_BATCH];
    int dst_cap[VX_MAX_BATCH];
};

__global__ void __launch_bounds__(kBlock) k_frame_capture_batch(CaptureBatchArgs a) {
    const int f = blockIdx.y;
    const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x, nt = (size_t)gridDim.x * kBlock;
    const int* src_count = a.src_count + 4 * (size_t)f;
    const int dst_cap = a.dst_cap[f];
    const int n_src = min(max(src_count[0], 0), a.src_cap);
    const int n = min(n_src, dst_cap);
    grid_copy_range(a.dst_kp[f], a.src_kp + (size_t)f * a.src_cap * sizeof(vx_keypoint), (size_t)n * sizeof(vx_keypoint), t, nt);
    grid_copy_range(a.dst_desc[f], a.src_desc + (size_t)f * a.src_cap * 32, (size_t)n * 32, t, nt);
    if (t == 0) {
        int* dst_count = a.dst_count[f];
        dst_count[0] = n;
        dst_count[1] = (src_count[0] > dst_cap || src_count[1] != 0) ? 1 : 0;
        dst_count[2] = 0;
        dst_count[3] = 0;
    }
}

int check_frame(vx_ctx* c, const vx_frame* f, const char* what) {
    if (!f || !f->block.p) return set_error(c, VX_ERR_INVALID, "%s: null frame", what);
    if (f->device != c->device) return set_error(c, VX_ERR_INVALID, "%s: frame and context on different devices", what);
    return VX_OK;
}

// the pinned staging of the two host-input forms: reused once the previous upload has left it
int staging(vx_ctx* c, size_t bytes) {
    if (c->fr_in_event) VX_HIP(c, hipEventSynchronize(c->fr_in_event));
    else VX_HIP(c, hipEventCreateWithFlags(&c->fr_in_event, hipEventDisableTiming));
    VX_HIP(c, c->fr_in_host.ensure(bytes));
    return VX_OK;
}

}  // namespace
}  // namespace vx

using namespace vx;

extern "C" {

int vx_frame_create(vx_ctx* c, int cap, vx_frame** out) {
    if (!c || !out) return c ? set_error(c, VX_ERR_INVALID, "vx_frame_create: null output") : VX_ERR_INVALID;
    *out = nullptr;
    if (cap < 1 || cap > (1 << 22)) return set_error(c, VX_ERR_INVALID, "vx_frame_create: capacity %d outside [1, 2^22]", cap);
    VX_HIP(c, hipSetDevice(c->device));
    vx_frame* f = new vx_frame;
    f->device = c->device;
    f->cap = cap;
    f->off_kp = 16;
    f->off_desc = f->off_kp + align16((size_t)cap * sizeof(vx_keypoint));
    f->bytes = f->off_desc + (size_t)cap * 32;
    hipError_t e = f->block.ensure(f->bytes);
    // an empty frame until something is captured or uploaded
    if (e == hipSuccess) e = hipMemsetAsync(f->block.p, 0, 16, c->stream);
    if (e != hipSuccess) {
        delete f;
        return hip_fail(c, e, "vx_frame_create");
    }
    *out = f;
    return VX_OK;
}

void vx_frame_destroy(vx_frame* f) { delete f; }

int vx_frame_capture_async(vx_ctx* c, int slot, vx_frame* f) {
    if (!c) return VX_ERR_INVALID;
    int rc;
    if ((rc = check_frame(c, f, "vx_frame_capture_async"))) return rc;
    if (slot < 0 || slot >= VX_MAX_SLOTS || !c->slots[slot].valid)
        return set_error(c, VX_ERR_STATE, "slot %d holds no extraction", slot);
    VX_HIP(c, hipSetDevice(c->device));
    const Slot& s = c->slots[slot];
    CaptureArgs a{};
    a.src_kp = s.kp.as<uint8_t>();
    a.src_desc = s.desc.as<uint8_t>();
    a.src_count = s.count.as<int>();
    a.src_cap = s.cap;
    a.dst_kp = reinterpret_cast<uint8_t*>(f->kp());
    a.dst_desc = f->desc();
    a.dst_count = f->count();
    a.dst_cap = f->cap;
    const size_t rows = (size_t)std::min(s.cap, f->cap);
    const size_t items = (rows * sizeof(vx_keypoint) + 15) / 16 + 2 + rows * 2;  // uint4 items of the larger range + head / tail
    const int grid = (int)std::min<size_t>(kMaxWg, std::max<size_t>(1, (items + kBlock - 1) / kBlock));
    VX_HIP(c, launch(c, kStFrameCapture, k_frame_capture, dim3(grid), dim3(kBlock), 0, c->stream, a));
    return VX_OK;
}

int vx_frame_capture_batch_async(vx_ctx* c, int bank, int n_frames, vx_frame* const* frames) {
    if (!c) return VX_ERR_INVALID;
    if (!frames) return set_error(c, VX_ERR_INVALID, "vx_frame_capture_batch_async: null frame list");
    if (bank < 0 || bank >= VX_BATCH_BANKS) return set_error(c, VX_ERR_INVALID, "bad batch bank %d", bank);
    if (n_frames < 1 || n_frames > c->batch_n[bank])
        return set_error(c, VX_ERR_STATE, "batch bank %d holds %d frames, %d asked for", bank, c->batch_n[bank], n_frames);
    const Slot& s = c->batch[bank];
    CaptureBatchArgs a{};
    a.src_kp = s.kp.as<uint8_t>();
    a.src_desc = s.desc.as<uint8_t>();
    a.src_count = s.count.as<int>();
    a.src_cap = s.cap;
    int max_cap = 1;
    for (int i = 0; i < n_frames; ++i) {
        int rc;
        if ((rc = check_frame(c, frames[i], "vx_frame_capture_batch_async"))) return rc;
        for (int j = 0; j < i; ++j)
            if (frames[j] == frames[i]) return set_error(c, VX_ERR_INVALID, "vx_frame_capture_batch_async: frame %d given twice", i);
        a.dst_kp[i] = reinterpret_cast<uint8_t*>(frames[i]->kp());
        a.dst_desc[i] = frames[i]->desc();
        a.dst_count[i] = frames[i]->count();
        a.dst_cap[i] = frames[i]->cap;
        max_cap = std::max(max_cap, frames[i]->cap);
    }
    VX_HIP(c, hipSetDevice(c->device));
    const size_t rows = (size_t)std::min(s.cap, max_cap);
    const size_t items = (rows * sizeof(vx_keypoint) + 15) / 16 + 2 + rows * 2;  // as vx_frame_capture_async, per frame
    const int grid = (int)std::min<size_t>(kMaxWg, std::max<size_t>(1, (items + kBlock - 1) / kBlock));
    VX_HIP(c, launch(c, kStFrameCaptureBatch, k_frame_capture_batch, dim3(grid, n_frames), dim3(kBlock), 0, c->stream, a));
    return VX_OK;
}

int vx_frame_extract_host_async(vx_ctx* c, vx_frame* f, const vx_orb_params* p, const uint8_t* img, int w, int h,
                                int channels, int64_t stride) {
    if (!c) return VX_ERR_INVALID;
    int rc;
    if ((rc = check_frame(c, f, "vx_frame_extract_host_async"))) return rc;
    if (!p || !img) return set_error(c, VX_ERR_INVALID, "vx_frame_extract_host_async: null params / image");
    if (w <= 0 || h <= 0) return set_error(c, VX_ERR_INVALID, "vx_frame_extract_host_async: image %d x %d", w, h);
    if (channels != 1 && channels != 3 && channels != 4) return set_error(c, VX_ERR_INVALID, "channels must be 1, 3 or 4");
    if (stride < (int64_t)w * channels) return set_error(c, VX_ERR_INVALID, "row stride too small");
    VX_HIP(c, hipSetDevice(c->device));
    const size_t packed = (size_t)w * channels, bytes = packed * h;
    if ((rc = staging(c, bytes))) return rc;
    VX_HIP(c, c->img_in.ensure(bytes));
    uint8_t* hs = static_cast<uint8_t*>(c->fr_in_host.p);
    if (stride == (int64_t)packed) std::memcpy(hs, img, bytes);
    else
        for (int y = 0; y < h; ++y) std::memcpy(hs + packed * y, img + (int64_t)y * stride, packed);
    VX_HIP(c, hipMemcpyAsync(c->img_in.p, hs, bytes, hipMemcpyHostToDevice, c->stream));
    VX_HIP(c, hipEventRecord(c->fr_in_event, c->stream));
    const int slot = VX_MAX_SLOTS - 1;
    if ((rc = vx_orb_extract_async(c, p, c->img_in.as<uint8_t>(), w, h, channels, (int64_t)packed, slot))) return rc;
    return vx_frame_capture_async(c, slot, f);
}

int vx_frame_upload_async(vx_ctx* c, vx_frame* f, const float* xy, const uint8_t* desc, int n) {
    if (!c) return VX_ERR_INVALID;
    int rc;
    if ((rc = check_frame(c, f, "vx_frame_upload_async"))) return rc;
    if (n < 0 || (n > 0 && (!xy || !desc))) return set_error(c, VX_ERR_INVALID, "vx_frame_upload_async: %d rows without arrays", n);
    if (n > f->cap) return set_error(c, VX_ERR_CAPACITY, "need %d rows, frame capacity %d", n, f->cap);
    VX_HIP(c, hipSetDevice(c->device));
    // the block's own layout up to the last descriptor row, so one copy fills it (the keypoint rows
    // between n and cap travel along: at most 20 B a row, never read)
    const size_t bytes = n ? f->off_desc + (size_t)n * 32 : 16;
    if ((rc = staging(c, bytes))) return rc;
    uint8_t* hs = static_cast<uint8_t*>(c->fr_in_host.p);
    const int32_t counts[4] = {n, 0, 0, 0};
    std::memcpy(hs, counts, sizeof counts);
    if (n) {
        std::memset(hs + f->off_kp, 0, f->off_desc - f->off_kp);
        for (int i = 0; i < n; ++i) std::memcpy(hs + f->off_kp + (size_t)i * sizeof(vx_keypoint), xy + 2 * (size_t)i, 8);
        std::memcpy(hs + f->off_desc, desc, (size_t)n * 32);
    }
    VX_HIP(c, hipMemcpyAsync(f->block.p, hs, bytes, hipMemcpyHostToDevice, c->stream));
    VX_HIP(c, hipEventRecord(c->fr_in_event, c->stream));
    return VX_OK;
}

int vx_frame_device(const vx_frame* f, const float** d_xy, int64_t* stride_bytes, const uint8_t** d_desc,
                    const int32_t** d_count, int32_t* cap) {
    if (!f || !f->block.p) return VX_ERR_INVALID;
    if (d_xy) *d_xy = &f->kp()->x;
    if (stride_bytes) *stride_bytes = (int64_t)sizeof(vx_keypoint);
    if (d_desc) *d_desc = f->desc();
    if (d_count) *d_count = f->count();
    if (cap) *cap = f->cap;
    return VX_OK;
}

int vx_frame_fetch_ex(vx_ctx* c, const vx_frame* f, vx_keypoint* kp, uint8_t* desc, int cap, int* n_out, int* overflow) {
    if (!c || !n_out) return c ? set_error(c, VX_ERR_INVALID, "vx_frame_fetch: null count") : VX_ERR_INVALID;
    *n_out = 0;
    int rc;
    if ((rc = check_frame(c, f, "vx_frame_fetch"))) return rc;
    if (cap < 0) return set_error(c, VX_ERR_INVALID, "vx_frame_fetch: negative capacity");
    VX_HIP(c, hipSetDevice(c->device));
    // the count is on the device, so the copy is sized by the frame's capacity: count | keypoint rows
    // (| descriptor rows), one copy into pinned memory
    const size_t bytes = desc ? f->bytes : (kp ? f->off_desc : 16);
    VX_HIP(c, c->fr_host.ensure(bytes));
    VX_HIP(c, hipMemcpyAsync(c->fr_host.p, f->block.p, bytes, hipMemcpyDeviceToHost, c->stream));
    VX_HIP(c, hipStreamSynchronize(c->stream));
    if (c->prof) prof_collect(c);
    const uint8_t* hs = static_cast<const uint8_t*>(c->fr_host.p);
    int32_t cnt[4];
    std::memcpy(cnt, hs, sizeof cnt);
    const int n = std::min(std::max(cnt[0], 0), f->cap);
    *n_out = n;
    if (overflow) *overflow = cnt[1];
    if ((kp || desc) && n > cap) return set_error(c, VX_ERR_CAPACITY, "need %d keypoints, cap %d", n, cap);
    if (kp && n) std::memcpy(kp, hs + f->off_kp, (size_t)n * sizeof(vx_keypoint));
    if (desc && n) std::memcpy(desc, hs + f->off_desc, (size_t)n * 32);
    return VX_OK;
}

int vx_frame_fetch(vx_ctx* c, const vx_frame* f, vx_keypoint* kp, uint8_t* desc, int cap, int* n_out) {
    return vx_frame_fetch_ex(c, f, kp, desc, cap, n_out, nullptr);
}

}  // extern "C"

static_assert(sizeof(vx_keypoint) == 20, "vx_keypoint rows: 20 bytes, a multiple of 4 (k_frame_capture's dword head / tail)");
