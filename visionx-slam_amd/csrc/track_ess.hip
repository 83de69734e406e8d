// track_ess.hip — Tracking::TrackLastFrame (core/frontend/tracking.cpp:281-330) and the head of
// Tracking::InitWithSecondFrame (:207-245) from the match list to the composed pose without leaving
// the device (vx_track_essential_async / vx_track_essential_fetch).
//
// The reference filters the matches by distance (:291-304), builds the cv::Point2f pairs (:509-514),
// calls findEssentialMat + recoverPose on them (:521-528), composes T_cl * T_lw (:539-541) and
// averages the pixel displacement of the kept matches (ComputeParallax, :325, :548-560).  Everything
// those steps read is already resident: the match list (match.hip) and both frames' keypoints
// (extraction slots, or any float2 rows).  The sequence is
//
//   k_track_epairs (1 workgroup) -> k_em_hyp .. k_em_final [ess_enqueue] -> k_track_epose (1 lane)
//
// with no host step between and one synchronisation, in the fetch.
//
// k_track_epairs is ONE workgroup for the reason k_track_pairs is (track.hip): the pairs keep the
// match order, which fixes RANSAC's sample stream, so the compaction is one block-wide ordered scan.
// Its stages 1-3 (min distance, threshold, kept list) ARE k_track_pairs' (track_common.hpp); then
//   4  pair gather   kept match j (in order): index bounds against the device counts (a match out of
//                    range is counted and never dereferenced); survivors compacted by ballot + mbcnt,
//                    16 wave totals in LDS and a running base into pts_last / pts_curr (the floats
//                    as they are) and pair_match
//   5  parallax      sqrt(dx * dx + dy * dy) on the widened doubles; per-thread partial, wave
//                    butterfly, wave partials summed in wave order: a fixed order
//   6  record        offsets {0, n_pairs} (or {0, 0} when the min_matches gate of :306 fails: the
//                    essential kernels then return ok = 0 without a hypothesis), intrinsics, options
// No atomics decide a position; no scratch.
//
// k_track_epose: one lane restates Sophus::SE3d(R, t) * T_lw after k_em_final — Shepperd's branches
// as PoseFromRt (host/src/geometry.cpp), the Hamilton product, the first-order renormalisation,
// t = R(q_cl) t_lw + t_cl in SE3d::operator*(Vec3d)'s operation order (host/include/visionx/types.h)
// — so the host adapters, tests/track_ess_ref.py and this kernel run the same IEEE sequence.
//
// Host side: EPairArgs / EPoseArgs are filled and the host values checked (trk::check_ess_host_args) by
// track_bodies.hpp's host section; the host-input form stages its upload in c->te_in (vx::StagedUpload).
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "vx_internal.hpp"
#include "track_bodies.hpp"

namespace vx {
namespace {

using trk::kBlock;
using trk::kWaves;

using trk::EPairArgs;
using trk::EPoseArgs;

// the stages above, stated in track_epairs_body.inc (shared with k_rig_epairs, track_rig.hip)
__global__ void __launch_bounds__(kBlock) k_track_epairs(EPairArgs a) {
#include "track_epairs_body.inc"
}

// Sophus::SE3d(R, t) * T_lw by one lane (tracking.cpp:539-541); zero when recoverPose gave nothing
__global__ void __launch_bounds__(64) k_track_epose(EPoseArgs a) {
    if (threadIdx.x != 0) return;
    trk::track_epose(a);
}

// packed result block: vx_track_essential_result | pair_match[cap] | mask[cap] (track_common.hpp)
size_t off_pair_match() { return trk::off_pair_match<vx_track_essential_result>(); }
size_t off_mask(int cap) { return trk::off_mask<vx_track_essential_result>(cap); }
size_t packed_bytes(int cap) { return trk::packed_bytes<vx_track_essential_result>(cap); }

bool stride_ok(int64_t s) { return s >= 8 && !(s & 3); }

}  // namespace
}  // namespace vx

using namespace vx;

extern "C" {

void vx_track_essential_default_options(vx_track_essential_options* o) {
    if (!o) return;
    o->min_matches = 50;  // Tracking::Options (tracking.h:27-28)
    o->min_inliers = 30;
    vx_essential_default_options(&o->ess);
}

int vx_track_essential_async(vx_ctx* c, const float* d_last_xy, int64_t last_stride_bytes, const int32_t* d_n_last,
                             const float* d_curr_xy, int64_t curr_stride_bytes, const int32_t* d_n_curr,
                             const vx_match* d_matches, const int32_t* d_n_matches, int cap_matches,
                             const double* pose_last7, const double* intr4, const vx_track_essential_options* opt) {
    if (!c) return VX_ERR_INVALID;
    if (!d_last_xy || !d_n_last || !d_curr_xy || !d_n_curr)
        return set_error(c, VX_ERR_INVALID, "vx_track_essential_async: null argument");
    int rc;
    if ((rc = trk::check_ess_host_args(c, "vx_track_essential_async", intr4, opt))) return rc;
    if (!stride_ok(last_stride_bytes) || !stride_ok(curr_stride_bytes))
        return set_error(c, VX_ERR_INVALID, "position strides %lld / %lld: multiples of 4, at least 8",
                         (long long)last_stride_bytes, (long long)curr_stride_bytes);
    if (d_matches) {
        if (!d_n_matches || cap_matches < 0) return set_error(c, VX_ERR_INVALID, "match list without a count / capacity");
    } else {
        if (!c->match_valid) return set_error(c, VX_ERR_STATE, "no match enqueued on this context");
        d_matches = c->matches.as<vx_match>();
        d_n_matches = c->match_count.as<int32_t>();
        cap_matches = c->match_cap;
    }
    VX_HIP(c, hipSetDevice(c->device));

    const int cap = std::max(cap_matches, 1);
    VX_HIP(c, c->te_good.ensure((size_t)cap * sizeof(int)));
    VX_HIP(c, c->te_p1.ensure((size_t)cap * 2 * sizeof(float)));
    VX_HIP(c, c->te_p2.ensure((size_t)cap * 2 * sizeof(float)));
    VX_HIP(c, c->te_prob.ensure(trk::prob1_bytes<EPairArgs>()));
    VX_HIP(c, c->te_out.ensure(packed_bytes(cap)));
    EPairArgs a{};
    a.matches = d_matches;
    a.n_matches = d_n_matches;
    a.cap_matches = cap_matches;
    a.last_xy = reinterpret_cast<const uint8_t*>(d_last_xy);
    a.last_stride = last_stride_bytes;
    a.n_last = d_n_last;
    a.curr_xy = reinterpret_cast<const uint8_t*>(d_curr_xy);
    a.curr_stride = curr_stride_bytes;
    a.n_curr = d_n_curr;
    trk::set_options(a, *opt, intr4);
    a.good = c->te_good.as<int>();
    a.p1 = c->te_p1.as<float>();
    a.p2 = c->te_p2.as<float>();
    trk::packed_outputs(a, c->te_out.as<uint8_t>(), cap);
    trk::prob1_pointers(a, c->te_prob.as<uint8_t>());
    c->te_valid = false;
    VX_HIP(c, launch(c, kStTrackEPairs, k_track_epairs, dim3(1), dim3(kBlock), 0, c->stream, a));
    EmDeviceArgs d{};
    d.offsets = a.offsets;
    d.intr = a.intr_out;
    d.opt = a.opt_out;
    d.p1 = a.p1;
    d.p2 = a.p2;
    d.out = &a.res->ess;
    d.mask = a.mask;
    // the per-match grids are sized by the capacity: the pair count is known on the device only
    if ((rc = ess_enqueue(c, 1, std::max(1, opt->ess.max_iterations), cap, d, c->te_hyp))) return rc;
    EPoseArgs p{};
    trk::epose_args(p, a.res, pose_last7);
    VX_HIP(c, launch(c, kStTrackEPose, k_track_epose, dim3(1), dim3(64), 0, c->stream, p));
    c->te_cap = cap;
    c->te_min_matches = opt->min_matches;
    c->te_min_inliers = opt->min_inliers;
    c->te_valid = true;
    return VX_OK;
}

int vx_track_essential_host_async(vx_ctx* c, const uint8_t* last_desc, int n_last, const float* last_xy,
                                  const uint8_t* curr_desc, int n_curr, const float* curr_xy, float ratio,
                                  const double* pose_last7, const double* intr4,
                                  const vx_track_essential_options* opt) {
    if (!c) return VX_ERR_INVALID;
    if (n_last < 0 || n_curr < 0 || (n_last && (!last_desc || !last_xy)) || (n_curr && (!curr_desc || !curr_xy)))
        return set_error(c, VX_ERR_INVALID, "vx_track_essential_host_async: bad descriptor / position arguments");
    int rc;
    if ((rc = trk::check_ess_host_args(c, "vx_track_essential_host_async", intr4, opt))) return rc;
    VX_HIP(c, hipSetDevice(c->device));
    // one staged block: {n_last, n_curr} | last rows | current rows | last positions | current positions.
    // The row capacities are rounded up to 256 as in vx_track_pnp_host_async (one launch configuration,
    // and one captured match graph, for frames with about as many features).
    const int cap_q = (std::max(n_last, 1) + 255) & ~255, cap_t = (std::max(n_curr, 1) + 255) & ~255;
    const size_t o_q = 16, o_t = o_q + (size_t)cap_q * 32, o_qxy = o_t + (size_t)cap_t * 32,
                 o_txy = o_qxy + (size_t)cap_q * 8, bytes = o_txy + (size_t)cap_t * 8;
    // (the one place this entry can block: until the previous call's upload has left the staging)
    VX_HIP(c, c->te_in.begin(bytes));
    uint8_t* h = static_cast<uint8_t*>(c->te_in.host.p);
    const int32_t counts[4] = {n_last, n_curr, 0, 0};
    std::memcpy(h, counts, sizeof counts);
    // rows between the counts and the rounded capacities are not filled: every kernel stops at the
    // device-side counts, so what the upload carries there is never read
    if (n_last) {
        std::memcpy(h + o_q, last_desc, (size_t)n_last * 32);
        std::memcpy(h + o_qxy, last_xy, (size_t)n_last * 8);
    }
    if (n_curr) {
        std::memcpy(h + o_t, curr_desc, (size_t)n_curr * 32);
        std::memcpy(h + o_txy, curr_xy, (size_t)n_curr * 8);
    }
    VX_HIP(c, c->te_in.upload(bytes, c->stream));
    const uint8_t* d = c->te_in.dev.as<uint8_t>();
    const int32_t* dn = c->te_in.dev.as<int32_t>();
    if ((rc = vx_match_device_async(c, d + o_q, dn, cap_q, d + o_t, dn + 1, cap_t, ratio))) return rc;
    // the list just enqueued, named explicitly with the capacity it was enqueued with
    return vx_track_essential_async(c, reinterpret_cast<const float*>(d + o_qxy), 8, dn,
                                    reinterpret_cast<const float*>(d + o_txy), 8, dn + 1, c->matches.as<vx_match>(),
                                    c->match_count.as<int32_t>(), cap_q, pose_last7, intr4, opt);
}

int vx_track_essential_fetch(vx_ctx* c, vx_track_essential_result* out, int32_t* pair_match, uint8_t* mask,
                             int cap_pairs) {
    if (!c || !out) return c ? set_error(c, VX_ERR_INVALID, "vx_track_essential_fetch: null result") : VX_ERR_INVALID;
    if (!c->te_valid) return set_error(c, VX_ERR_STATE, "no vx_track_essential_async enqueued");
    VX_HIP(c, hipSetDevice(c->device));
    const size_t bytes = packed_bytes(c->te_cap);
    VX_HIP(c, c->te_host.ensure(bytes));
    VX_HIP(c, hipMemcpyAsync(c->te_host.p, c->te_out.p, bytes, hipMemcpyDeviceToHost, c->stream));
    VX_HIP(c, hipStreamSynchronize(c->stream));
    if (c->prof) prof_collect(c);
    const uint8_t* h = static_cast<const uint8_t*>(c->te_host.p);
    std::memcpy(out, h, sizeof *out);
    out->status = trk::ess_status(*out, c->te_min_matches, c->te_min_inliers);  // (:306, :317; track_common.hpp)
    const int np = out->n_pairs;
    if ((pair_match || mask) && np > cap_pairs)
        return set_error(c, VX_ERR_CAPACITY, "need %d pairs, cap %d", np, cap_pairs);
    if (pair_match && np) std::memcpy(pair_match, h + off_pair_match(), (size_t)np * sizeof(int32_t));
    if (mask && np) std::memcpy(mask, h + off_mask(c->te_cap), (size_t)np);
    return VX_OK;
}

}  // extern "C"

static_assert(sizeof(vx_track_essential_options) == 48, "vx_track_essential_options layout (python TRACK_ESS_OPTIONS_DTYPE)");
static_assert(sizeof(vx_track_essential_result) == 288, "vx_track_essential_result layout (python TRACK_ESS_RESULT_DTYPE)");
static_assert(offsetof(vx_track_essential_result, parallax) == 24 && offsetof(vx_track_essential_result, pose) == 32 &&
                  offsetof(vx_track_essential_result, ess) == 88,
              "vx_track_essential_result has no implicit padding");
