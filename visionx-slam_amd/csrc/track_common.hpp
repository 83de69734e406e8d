// track_common.hpp — the stages k_track_pairs (track.hip) and k_track_epairs (track_ess.hip) share:
// the distance filter every Tracking::Track* path opens with (core/frontend/tracking.cpp:342-355,
// :291-304, :211-222) as ONE workgroup of kBlock threads — block minimum, threshold, the kept
// matches written in match order — and the ordered rank both kernels compact with.
#pragma once

#include "vx_internal.hpp"

namespace vx {
namespace trk {

constexpr int kBlock = 1024;
constexpr int kWaves = kBlock / 64;

// The packed result block of vx_track_pnp_async / vx_track_essential_async (R = its record):
// R | pair_match[cap] | mask[cap], each part on a 16-byte boundary.
template <class R>
__host__ __device__ inline size_t off_pair_match() { return align16(sizeof(R)); }
template <class R>
__host__ __device__ inline size_t off_mask(int cap) { return off_pair_match<R>() + align16((size_t)cap * sizeof(int32_t)); }
template <class R>
__host__ __device__ inline size_t packed_bytes(int cap) { return off_mask<R>(cap) + align16((size_t)cap); }

// The status rules the fetches apply on the host and k_track_gate / k_track_final (track_frame.hip)
// on the device: ONE statement of each, in the order of the reference's return statements.
// x - x is 0 exactly when x is finite (inf - inf and NaN - NaN are NaN), on either side.  That holds under
// IEEE arithmetic only: the library is built without -ffast-math / -ffinite-math-only (Makefile), which
// would let the compiler fold the test to true here as it would fold std::isfinite.
__host__ __device__ inline bool pose_finite(const double* pose7) {
    bool finite = true;  // R = Rodrigues(rvec) is finite exactly when the pose is (tracking.cpp:441)
    for (int k = 0; k < 7; ++k) finite &= (pose7[k] - pose7[k]) == 0.0;
    return finite;
}
// TrackWithPnP (tracking.cpp:357, :402, :425, :441)
__host__ __device__ inline int pnp_status(const vx_track_result& r, int min_matches, int min_inliers) {
    if (r.n_good_matches < min_matches) return VX_TRACK_FEW_MATCHES;
    if (r.n_pairs < min_inliers) return VX_TRACK_FEW_PAIRS;
    if (!r.pnp.ok || r.pnp.n_inliers < min_inliers) return VX_TRACK_PNP_FAILED;
    if (!pose_finite(r.pnp.pose)) return VX_TRACK_BAD_ROTATION;
    return VX_TRACK_OK;
}
// TrackLastFrame (tracking.cpp:306, :317)
__host__ __device__ inline int ess_status(const vx_track_essential_result& r, int min_matches, int min_inliers) {
    if (r.n_good_matches < min_matches) return VX_TRACK_FEW_MATCHES;
    if (!r.ess.ok || r.ess.n_inliers < min_inliers) return VX_TRACK_ESSENTIAL_FAILED;
    return VX_TRACK_OK;
}

// Exclusive rank of this thread's flag among the block's flags (thread order) and their total.
// Two barriers: the wave counts are read by everyone before the next call rewrites them.
__device__ __forceinline__ int block_rank(bool flag, int* s_cnt, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t b = __ballot(flag);
    const int in_wave = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
    if (lane == 0) s_cnt[wave] = __popcll(b);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const int v = s_cnt[w];
        before += w < wave ? v : 0;
        all += v;
    }
    __syncthreads();
    *total = all;
    return before + in_wave;
}

// Stages 1-3 of both kernels over matches[0, n): min distance started at 100.0f, thr = max(2 min, 30),
// the indices of the matches with distance <= thr into good[] in match order.  Returns their count
// (the same in every thread) and the minimum in *min_out; ends on a barrier, so good[] may be read
// by any thread of the workgroup afterwards (one workgroup: one CU, one L1).
// s_cnt / s_min: kWaves entries of LDS each.
__device__ __forceinline__ int filter_matches(const vx_match* matches, int n, int* good, int* s_cnt, float* s_min,
                                              float* min_out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // 1: min distance (tracking.cpp:345-348)
    float mn = 100.0f;
    for (int i = tid; i < n; i += kBlock) {
        const float d = matches[i].distance;
        if (d < mn) mn = d;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float o = __shfl_xor(mn, off);
        if (o < mn) mn = o;
    }
    if (lane == 0) s_min[wave] = mn;
    __syncthreads();
    mn = s_min[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w)
        if (s_min[w] < mn) mn = s_min[w];
    // 2: std::max(2 * min_dist, 30.0f) (:350)
    const float thr = fmaxf(2 * mn, 30.0f);

    // 3: the kept matches, in match order
    int n_good = 0;
    for (int base = 0; base < n; base += kBlock) {
        const int i = base + tid;
        const bool keep = i < n && matches[i].distance <= thr;
        int total;
        const int r = block_rank(keep, s_cnt, &total);
        if (keep) good[n_good + r] = i;
        n_good += total;
    }
    __syncthreads();
    *min_out = mn;
    return n_good;
}

}  // namespace trk
}  // namespace vx
