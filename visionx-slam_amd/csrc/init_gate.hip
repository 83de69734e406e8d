// init_gate.hip — the three gates of Tracking::InitWithFirstFrame (core/frontend/tracking.cpp:177-204)
// on an image and keypoints that are already on the device (vx_init_gate_async / vx_init_gate_fetch).
//
// The reference checks the feature count (:179), CheckFeatureDistribution's 5 x 5 occupancy grid over
// the keypoints (:93-118) and CheckImageQuality's cvtColor(BGR2GRAY) + meanStdDev bounds (:120-139) on
// every frame while the tracker waits for a usable first frame.  Here that is
//
//   k_init_sums (many workgroups) -> k_init_gate (1 workgroup)
//
// on the context's stream with one synchronisation, in the fetch.
//
// k_init_sums reads the INPUT image (not the extraction's pyramid: the call does not depend on what
// was last extracted on the context) and accumulates the integer sum and sum of squares of the gray
// level-0 pixel, gray_px of vx_gray.hpp.  A row is cut into a byte head up to the first 16-byte
// boundary that is also a pixel boundary, groups of 16 pixels read as 1 / 3 / 4 uint4 (1 / 3 / 4
// channels) and a byte tail, so any base alignment, stride and width takes the vector path for all but
// at most 30 pixels of a row (a 4-channel row whose base is not a multiple of 4 has no such boundary
// and goes by bytes).  An image without row padding is one row of width * height pixels.  Lanes keep
// 32-bit partials for as many pixels as provably fit and widen them to 64 bits; everything that
// crosses lanes is 64-bit: wave butterfly, one LDS slot per wave, one {sum, sum_sq} slot per
// workgroup.  No atomics and no zeroing launch: k_init_gate adds the slots in slot order (integer
// sums are order-free, so the record is bitwise repeatable either way).
//
// k_init_gate: finishes the sums; walks the keypoints (col = (int)((x / width) * cols) in double,
// truncation toward zero, clamp: :101-104) and OR-reduces the occupancy mask; one lane then restates
// meanStdDev's arithmetic — scale = 1.0 / N, mean = sum * scale, sqrt(max(sum_sq * scale - mean *
// mean, 0)), every operation rounded on its own — and the gates, and writes the record.
#include <algorithm>
#include <cstddef>
#include <cstring>

#include "vx_gray.hpp"
#include "vx_internal.hpp"

namespace vx {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxWg = 1024;  // slots k_init_gate adds (4 workgroups per compute unit of a 256-CU device)
constexpr int kGroup = 16;    // pixels per vector group
// A lane's 32-bit sum of squares holds at most 66 051 pixels of value 255 (66 051 * 255 * 255 =
// 4 294 966 275 <= 2^32 - 1 < 66 052 * 255 * 255); its 32-bit sum holds more.
constexpr uint32_t kLaneMax = 66051;

struct SumArgs {
    const uint8_t* img;
    int64_t rows, px;   // rows of px pixels each (1 x width * height when the image has no row padding)
    int64_t stride;     // bytes between rows
    unsigned long long* part;  // 2 per workgroup: sum, sum_sq
};

struct LaneAcc {
    uint32_t s = 0, q = 0, n = 0;       // 32-bit partials over n pixels since the last widening
    unsigned long long S = 0, Q = 0;
    __device__ __forceinline__ void widen() {
        S += s;
        Q += q;
        s = q = n = 0;
    }
    __device__ __forceinline__ void add(uint32_t v) {
        s += v;
        q += v * v;
    }
    // after at most kGroup pixels were added: widen while another kGroup still provably fits
    __device__ __forceinline__ void added(uint32_t k) {
        n += k;
        if (n > kLaneMax - kGroup) widen();
    }
};

// the 16 gray pixels of one group from its CH uint4
template <int CH>
__device__ __forceinline__ void add_group(LaneAcc& acc, const uint4* p) {
    uint32_t w[4 * CH];
#pragma unroll
    for (int k = 0; k < CH; ++k) {
        const uint4 v = p[k];
        w[4 * k] = v.x;
        w[4 * k + 1] = v.y;
        w[4 * k + 2] = v.z;
        w[4 * k + 3] = v.w;
    }
    auto byte_at = [&](int i) -> int { return (int)((w[i >> 2] >> ((i & 3) * 8)) & 255u); };
#pragma unroll
    for (int j = 0; j < kGroup; ++j) {
        uint32_t g;
        if (CH == 1) g = (uint32_t)byte_at(j);
        else g = gray_bgr(byte_at(CH * j), byte_at(CH * j + 1), byte_at(CH * j + 2));
        acc.add(g);
    }
    acc.added(kGroup);
}

template <int CH>
__global__ void __launch_bounds__(kBlock) k_init_sums(SumArgs a) {
    __shared__ unsigned long long s_red[kWaves][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t col0 = (int64_t)blockIdx.x * kBlock + tid, col_step = (int64_t)gridDim.x * kBlock;
    LaneAcc acc;
    for (int64_t r = blockIdx.y; r < a.rows; r += gridDim.y) {
        const uint8_t* row = a.img + r * a.stride;
        // head: pixels before the first address that is a multiple of 16 and a pixel boundary
        const int64_t m = (int64_t)((16 - (reinterpret_cast<uintptr_t>(row) & 15)) & 15);  // bytes to it
        int64_t head;
        if (CH == 1) head = m;
        else if (CH == 3) head = (m * 11) & 15;  // 3 * head = m (mod 16): 3 * 11 = 33 = 1 (mod 16)
        else head = (m & 3) ? a.px : (m >> 2);   // 4 channels: a base off a multiple of 4 never gets there
        if (head > a.px) head = a.px;
        const int64_t groups = (a.px - head) / kGroup, tail = head + groups * kGroup;
        for (int64_t i = col0; i < head; i += col_step) {
            acc.add(gray_px(row + i * CH, CH));
            acc.added(1);
        }
        const uint4* vrow = reinterpret_cast<const uint4*>(row + head * CH);
        for (int64_t g = col0; g < groups; g += col_step) add_group<CH>(acc, vrow + g * CH);
        for (int64_t i = tail + col0; i < a.px; i += col_step) {
            acc.add(gray_px(row + i * CH, CH));
            acc.added(1);
        }
    }
    acc.widen();
    unsigned long long S = acc.S, Q = acc.Q;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        S += __shfl_xor(S, off);
        Q += __shfl_xor(Q, off);
    }
    if (lane == 0) {
        s_red[wave][0] = S;
        s_red[wave][1] = Q;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < kWaves; ++w) {
            S += s_red[w][0];
            Q += s_red[w][1];
        }
        const int64_t wg = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        a.part[2 * wg] = S;
        a.part[2 * wg + 1] = Q;
    }
}

struct GateArgs {
    const unsigned long long* part;
    int n_part;
    const uint8_t* xy;  // two floats at xy + i * xy_stride
    int64_t xy_stride;
    const int* n_feat;
    int cap_feat;
    int width, height;
    vx_init_gate_options opt;
    vx_init_gate_result* res;
};

__global__ void __launch_bounds__(kBlock) k_init_gate(GateArgs a) {
    __shared__ unsigned long long s_red[kWaves][2];
    __shared__ uint32_t s_mask[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long S = 0, Q = 0;
    for (int i = tid; i < a.n_part; i += kBlock) {
        S += a.part[2 * i];
        Q += a.part[2 * i + 1];
    }
    // CheckFeatureDistribution (:100-106)
    const int n = min(max(*a.n_feat, 0), a.cap_feat);
    const int cols = a.opt.grid_cols, rows = a.opt.grid_rows;
    uint32_t mask = 0;
    for (int i = tid; i < n; i += kBlock) {
        const float* p = reinterpret_cast<const float*>(a.xy + (int64_t)i * a.xy_stride);
        int col = (int)(((double)p[0] / a.width) * cols);
        int row = (int)(((double)p[1] / a.height) * rows);
        col = min(max(col, 0), cols - 1);
        row = min(max(row, 0), rows - 1);
        mask |= 1u << (col * rows + row);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        S += __shfl_xor(S, off);
        Q += __shfl_xor(Q, off);
        mask |= __shfl_xor(mask, off);
    }
    if (lane == 0) {
        s_red[wave][0] = S;
        s_red[wave][1] = Q;
        s_mask[wave] = mask;
    }
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
        S += s_red[w][0];
        Q += s_red[w][1];
        mask |= s_mask[w];
    }
    const int valid = __popc(mask);
    const int64_t n_pixels = (int64_t)a.width * a.height;
    // meanStdDev (:126): the reciprocal, and no fused multiply-add in the variance
    const double scale = __ddiv_rn(1.0, (double)n_pixels);
    const double mean = __dmul_rn((double)S, scale);
    const double var = __dsub_rn(__dmul_rn((double)Q, scale), __dmul_rn(mean, mean));
    const double stddev = __dsqrt_rn(var > 0.0 ? var : 0.0);
    int status = VX_INIT_OK;
    if (n < a.opt.min_features) status = VX_INIT_FEW_FEATURES;                                          // (:179)
    else if ((double)valid < __dmul_rn((double)(cols * rows), a.opt.min_grid_frac)) status = VX_INIT_POOR_DISTRIBUTION;  // (:117)
    else if (mean < a.opt.min_mean || mean > a.opt.max_mean || stddev < a.opt.min_stddev) status = VX_INIT_POOR_IMAGE;  // (:129-135)
    vx_init_gate_result* r = a.res;
    r->status = status;
    r->n_features = n;
    r->valid_grids = valid;
    r->grid_mask = mask;
    r->n_pixels = n_pixels;
    r->sum = S;
    r->sum_sq = Q;
    r->mean = mean;
    r->stddev = stddev;
}

int check_args(vx_ctx* c, const void* img, int w, int h, int ch, int64_t stride, int64_t xy_stride,
               const vx_init_gate_options* opt) {
    if (!img || !opt) return set_error(c, VX_ERR_INVALID, "vx_init_gate: null image / options");
    if (w <= 0 || h <= 0) return set_error(c, VX_ERR_INVALID, "vx_init_gate: image %d x %d", w, h);
    if (ch != 1 && ch != 3 && ch != 4) return set_error(c, VX_ERR_INVALID, "vx_init_gate: %d channels (1, 3 or 4)", ch);
    if (stride < (int64_t)w * ch)
        return set_error(c, VX_ERR_INVALID, "vx_init_gate: row stride %lld < %d * %d", (long long)stride, w, ch);
    if (xy_stride < 8 || (xy_stride & 3))
        return set_error(c, VX_ERR_INVALID, "position stride %lld: a multiple of 4, at least 8", (long long)xy_stride);
    if (opt->grid_cols < 1 || opt->grid_rows < 1 || (int64_t)opt->grid_cols * opt->grid_rows > 32)
        return set_error(c, VX_ERR_INVALID, "vx_init_gate: grid %d x %d (1..32 cells)", opt->grid_cols, opt->grid_rows);
    return VX_OK;
}

}  // namespace
}  // namespace vx

using namespace vx;

extern "C" {

void vx_init_gate_default_options(vx_init_gate_options* o) {
    if (!o) return;
    std::memset(o, 0, sizeof *o);
    o->min_features = 50;  // Tracking::Options::min_matches (tracking.h:27)
    o->grid_cols = 5;      // (tracking.cpp:96-97)
    o->grid_rows = 5;
    o->min_grid_frac = 0.5;  // (:117)
    o->min_mean = 30.0;      // (:129)
    o->max_mean = 225.0;
    o->min_stddev = 20.0;    // (:134)
}

int vx_init_gate_async(vx_ctx* c, const uint8_t* d_img, int width, int height, int channels, int64_t row_stride,
                       const float* d_xy, int64_t xy_stride_bytes, const int32_t* d_n_feat, int cap_feat,
                       const vx_init_gate_options* opt) {
    if (!c) return VX_ERR_INVALID;
    int rc;
    if ((rc = check_args(c, d_img, width, height, channels, row_stride, xy_stride_bytes, opt))) return rc;
    if (!d_n_feat || cap_feat < 0 || (cap_feat > 0 && !d_xy))
        return set_error(c, VX_ERR_INVALID, "vx_init_gate_async: positions without a count / capacity");
    VX_HIP(c, hipSetDevice(c->device));

    SumArgs s{};
    s.img = d_img;
    s.stride = row_stride;
    if (row_stride == (int64_t)width * channels) {  // no row padding: one row
        s.rows = 1;
        s.px = (int64_t)width * height;
    } else {
        s.rows = height;
        s.px = width;
    }
    const int64_t per_row = ((s.px + kGroup - 1) / kGroup + kBlock - 1) / kBlock;  // workgroups a row can feed
    const int gx = (int)std::min<int64_t>(std::max<int64_t>(per_row, 1), kMaxWg);
    const int gy = (int)std::min<int64_t>(s.rows, std::max(kMaxWg / gx, 1));
    const int n_part = gx * gy;
    VX_HIP(c, c->ig_part.ensure((size_t)kMaxWg * 2 * sizeof(unsigned long long)));
    VX_HIP(c, c->ig_out.ensure(sizeof(vx_init_gate_result)));
    s.part = c->ig_part.as<unsigned long long>();
    c->ig_valid = false;
    const dim3 grid(gx, gy), block(kBlock);
    if (channels == 1) VX_HIP(c, launch(c, kStInitSums, k_init_sums<1>, grid, block, 0, c->stream, s));
    else if (channels == 3) VX_HIP(c, launch(c, kStInitSums, k_init_sums<3>, grid, block, 0, c->stream, s));
    else VX_HIP(c, launch(c, kStInitSums, k_init_sums<4>, grid, block, 0, c->stream, s));

    GateArgs g{};
    g.part = s.part;
    g.n_part = n_part;
    g.xy = reinterpret_cast<const uint8_t*>(d_xy);
    g.xy_stride = xy_stride_bytes;
    g.n_feat = d_n_feat;
    g.cap_feat = cap_feat;
    g.width = width;
    g.height = height;
    g.opt = *opt;
    g.res = c->ig_out.as<vx_init_gate_result>();
    VX_HIP(c, launch(c, kStInitGate, k_init_gate, dim3(1), block, 0, c->stream, g));
    c->ig_valid = true;
    return VX_OK;
}

int vx_init_gate_host_async(vx_ctx* c, const uint8_t* img, int width, int height, int channels, int64_t row_stride,
                            const float* xy, int64_t xy_stride_bytes, int n_feat, const vx_init_gate_options* opt) {
    if (!c) return VX_ERR_INVALID;
    int rc;
    if ((rc = check_args(c, img, width, height, channels, row_stride, xy_stride_bytes, opt))) return rc;
    if (n_feat < 0 || (n_feat > 0 && !xy))
        return set_error(c, VX_ERR_INVALID, "vx_init_gate_host_async: %d positions without an array", n_feat);
    VX_HIP(c, hipSetDevice(c->device));
    // one staged block: {n_feat} | float2 positions | image rows without their padding
    const size_t row_bytes = (size_t)width * channels;
    const size_t o_xy = 16, o_img = o_xy + align16((size_t)n_feat * 8), bytes = o_img + row_bytes * height;
    // (the one place this entry can block: until the previous call's upload has left the staging)
    VX_HIP(c, c->ig_in.begin(bytes));
    uint8_t* h = static_cast<uint8_t*>(c->ig_in.host.p);
    const int32_t counts[4] = {n_feat, 0, 0, 0};
    std::memcpy(h, counts, sizeof counts);
    if (xy_stride_bytes == 8) {
        if (n_feat) std::memcpy(h + o_xy, xy, (size_t)n_feat * 8);
    } else {
        const uint8_t* src = reinterpret_cast<const uint8_t*>(xy);
        for (int i = 0; i < n_feat; ++i) std::memcpy(h + o_xy + (size_t)i * 8, src + (int64_t)i * xy_stride_bytes, 8);
    }
    if (row_stride == (int64_t)row_bytes) {
        std::memcpy(h + o_img, img, row_bytes * height);
    } else {
        for (int y = 0; y < height; ++y) std::memcpy(h + o_img + row_bytes * y, img + (int64_t)y * row_stride, row_bytes);
    }
    VX_HIP(c, c->ig_in.upload(bytes, c->stream));
    const uint8_t* d = c->ig_in.dev.as<uint8_t>();
    return vx_init_gate_async(c, d + o_img, width, height, channels, (int64_t)row_bytes,
                              reinterpret_cast<const float*>(d + o_xy), 8, c->ig_in.dev.as<int32_t>(), n_feat, opt);
}

int vx_init_gate_fetch(vx_ctx* c, vx_init_gate_result* out) {
    if (!c || !out) return c ? set_error(c, VX_ERR_INVALID, "vx_init_gate_fetch: null result") : VX_ERR_INVALID;
    if (!c->ig_valid) return set_error(c, VX_ERR_STATE, "no vx_init_gate_async enqueued");
    VX_HIP(c, hipSetDevice(c->device));
    VX_HIP(c, c->ig_host.ensure(sizeof *out));
    VX_HIP(c, hipMemcpyAsync(c->ig_host.p, c->ig_out.p, sizeof *out, hipMemcpyDeviceToHost, c->stream));
    VX_HIP(c, hipStreamSynchronize(c->stream));
    if (c->prof) prof_collect(c);
    std::memcpy(out, c->ig_host.p, sizeof *out);
    return VX_OK;
}

}  // extern "C"

static_assert(sizeof(vx_init_gate_options) == 48 && offsetof(vx_init_gate_options, min_grid_frac) == 16,
              "vx_init_gate_options layout (python INIT_GATE_OPTIONS_DTYPE)");
static_assert(sizeof(vx_init_gate_result) == 56 && offsetof(vx_init_gate_result, n_pixels) == 16 &&
                  offsetof(vx_init_gate_result, mean) == 40,
              "vx_init_gate_result layout (python INIT_GATE_RESULT_DTYPE)");
