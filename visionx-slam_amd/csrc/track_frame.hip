// track_frame.hip — Tracking::Track (core/frontend/tracking.cpp:267-279) over device-resident frames as
// one stream-ordered sequence (vx_track_frame_async / vx_track_frame_fetch).
//
// The reference tries TrackWithPnP against the last keyframe (:269-273) and, when that returns false,
// TrackLastFrame against the last frame (:278).  Decided on the host, a fallback frame is two matches,
// two uploads and two synchronisations.  Here the decision is taken on the device:
//
//   Match(last_kf, curr)  -> k_track_pairs -> k_pnp_hyp -> k_pnp_refine      [vx_track_pnp_async]
//   k_track_gate (1 workgroup)
//   Match(last, curr)     -> k_track_epairs -> k_em_* -> k_track_epose       [vx_track_essential_async]
//   k_track_final
//
// k_track_gate applies trk::pnp_status (track_common.hpp: the rule vx_track_pnp_fetch applies on the
// host, tracking.cpp:357, :402, :425, :441) to the PnP record and writes the GATED query count: the last
// frame's count when PnP failed or there is no last keyframe, 0 when it succeeded.  The fallback's
// match reads it as its query count and k_track_epairs as the last frame's row count; every kernel
// behind them is driven by device-side counts already, so with the gate closed they run as empty
// launches (no kernel changes for this): the match list is empty, the essential problem record says
// {0, 0}, k_em_hyp runs no hypothesis, and the record is what vx_track_essential_async leaves on an
// empty match list.  When the last keyframe IS the last frame (the frame after a keyframe) the second
// match is not enqueued: list 1 is list 0's rows under a gated count the gate writes.
//
// k_track_final packs what the fetch brings down in one copy:
//   vx_track_frame_result | pair_match0 | mask0 | pair_match1 | mask1 | the current frame's keypoint rows
// One lane writes the head (path, status, inliers, parallax, pose: COPIED from the path that set the
// pose, never recomputed) and the two status fields; the grid copies the two records, the pair arrays
// up to their device-side counts and the keypoint rows (grid_copy_range: 16-byte vectors).
//
// Both kernels are bound by launch latency, not bandwidth: the gate reads one record and writes 16
// bytes; the final kernel moves 464 B of records, 5 B a pair and 20 B a keypoint (about 50 KB at 2000
// features).  Resources (-Rpass-analysis=kernel-resource-usage, gfx950): k_track_gate 10 VGPRs / 34 SGPRs,
// k_track_final 28 VGPRs / 56 SGPRs; no LDS, no scratch.
//
// Host side: the block's layout is trk::FrameBlock (c->tf_blk), GateArgs / FinalArgs are filled and the frames
// checked (trk::check_frames) by track_bodies.hpp's host section.
#include <algorithm>
#include <cstddef>
#include <cstring>

#include "vx_internal.hpp"
#include "dmap.hpp"
#include "track_bodies.hpp"

namespace vx {
namespace {

constexpr int kGateBlock = 64;
constexpr int kFinalBlock = 256;
constexpr int kFinalMaxWg = 64;

using trk::FinalArgs;
using trk::GateArgs;

// One workgroup; one lane has all the work (a record read, a rule, four stores: track_bodies.hpp)
__global__ void __launch_bounds__(kGateBlock) k_track_gate(GateArgs a) {
    if (threadIdx.x != 0) return;
    trk::track_gate(a);
}

// (the body: track_bodies.hpp, shared with k_rig_final; the masks are the two packed blocks' own)
__global__ void __launch_bounds__(kFinalBlock) k_track_final(FinalArgs a) {
    const size_t t = (size_t)blockIdx.x * kFinalBlock + threadIdx.x, nt = (size_t)gridDim.x * kFinalBlock;
    trk::track_final<false>(a, a.tk + trk::off_mask<vx_track_result>(a.tk_cap),
                            a.te + trk::off_mask<vx_track_essential_result>(a.te_cap), t, nt);
}

}  // namespace
}  // namespace vx

using namespace vx;

extern "C" {

int vx_track_frame_async(vx_ctx* c, vx_dmap* m, uint64_t last_kf_id, const vx_frame* last_kf, const vx_frame* last,
                         const vx_frame* curr, float ratio, const double* pose_last7, const double* intr4,
                         const vx_track_options* pnp_opt, const vx_track_essential_options* ess_opt) {
    if (!c) return VX_ERR_INVALID;
    const char* who = "vx_track_frame_async";
    if (!ess_opt) return set_error(c, VX_ERR_INVALID, "%s: null argument", who);
    int rc;
    if ((rc = trk::check_frames(c, who, m, m && pnp_opt, last_kf_id, last_kf, last, curr, intr4))) return rc;
    VX_HIP(c, hipSetDevice(c->device));
    c->tf_valid = c->tf_fetched = false;
    c->tf_cap[0] = c->tf_cap[1] = 0;

    // The fallback's query side when there is no last frame: the current frame's rows under a gated
    // count of 0 (never read), so the essential record is the empty one in every case.
    const vx_frame* q1 = last ? last : curr;
    const bool shared = last_kf && last_kf == last;  // list 1 = list 0's rows under a gated count
    const int cap0 = last_kf ? last_kf->cap : 0, cap1 = q1->cap;
    VX_HIP(c, c->tf_count.ensure(32));
    VX_HIP(c, c->tf_gate.ensure(16));
    if (last_kf) VX_HIP(c, c->tf_matches[0].ensure((size_t)cap0 * sizeof(vx_match)));
    if (!shared) VX_HIP(c, c->tf_matches[1].ensure((size_t)cap1 * sizeof(vx_match)));
    int32_t* n0 = c->tf_count.as<int32_t>();
    int32_t* n1 = n0 + 4;
    int32_t* gate = c->tf_gate.as<int32_t>();
    vx_match* list0 = c->tf_matches[0].as<vx_match>();
    vx_match* list1 = shared ? list0 : c->tf_matches[1].as<vx_match>();
    const float* curr_xy = &curr->kp()->x;
    const int64_t stride = (int64_t)sizeof(vx_keypoint);

    // 1 + 2: Match(last_kf, curr) and TrackWithPnP's chain on it (:340-455)
    if (last_kf) {
        if ((rc = match_enqueue_to(c, last_kf->desc(), last_kf->count(), cap0, curr->desc(), curr->count(), curr->cap, cap0,
                                   curr->cap, ratio, list0, n0)))
            return rc;
        if ((rc = vx_track_pnp_async(c, m, last_kf_id, curr_xy, stride, curr->count(), list0, n0, cap0, intr4, pnp_opt)))
            return rc;
    }
    // 3: the decision of :269-273
    GateArgs g{};
    trk::gate_args(g, last_kf ? c->tk_out.as<vx_track_result>() : nullptr, pnp_opt, last, gate);
    g.n_matches0 = shared ? n0 : nullptr;
    g.n_matches1 = n1;
    VX_HIP(c, launch(c, kStTrackGate, k_track_gate, dim3(1), dim3(kGateBlock), 0, c->stream, g));
    // 4 + 5: Match(last, curr) under the gated count and TrackLastFrame's chain on it (:287-325)
    if (!shared &&
        (rc = match_enqueue_to(c, q1->desc(), gate, cap1, curr->desc(), curr->count(), curr->cap, cap1, curr->cap, ratio,
                               list1, n1)))
        return rc;
    if ((rc = vx_track_essential_async(c, &q1->kp()->x, stride, gate, curr_xy, stride, curr->count(), list1, n1, cap1,
                                       pose_last7, intr4, ess_opt)))
        return rc;
    // 6: the head and the packed block
    const trk::FrameBlock blk{last_kf ? c->tk_cap : 0, c->te_cap, curr->cap};
    VX_HIP(c, c->tf_out.ensure(blk.bytes(true)));
    FinalArgs f{};
    trk::final_args(f, last_kf ? c->tk_out.as<uint8_t>() : nullptr, c->te_out.as<uint8_t>(), blk, gate, last != nullptr, *ess_opt,
                    curr, c->tf_out.as<uint8_t>());
    const size_t items = ((size_t)curr->cap * sizeof(vx_keypoint)) / 16 + 1;
    const int grid = (int)std::min<size_t>(kFinalMaxWg, (items + kFinalBlock - 1) / kFinalBlock);
    VX_HIP(c, launch(c, kStTrackFinal, k_track_final, dim3(std::max(grid, 1)), dim3(kFinalBlock), 0, c->stream, f));
    c->tf_cap[0] = cap0;
    c->tf_cap[1] = cap1;
    c->tf_blk = blk;
    c->tf_list1_own = !shared;
    c->tf_valid = true;
    return VX_OK;
}

int vx_track_frame_fetch(vx_ctx* c, vx_track_frame_result* out, vx_keypoint* curr_kp, int cap_kp, int* n_kp) {
    if (!c || !out) return c ? set_error(c, VX_ERR_INVALID, "vx_track_frame_fetch: null result") : VX_ERR_INVALID;
    if (curr_kp && (!n_kp || cap_kp < 0)) return set_error(c, VX_ERR_INVALID, "vx_track_frame_fetch: keypoints without a count / capacity");
    if (!c->tf_valid) return set_error(c, VX_ERR_STATE, "no vx_track_frame_async enqueued");
    VX_HIP(c, hipSetDevice(c->device));
    // the keypoint rows are the block's tail: copied only when asked for
    const size_t o_kp = c->tf_blk.kp(), bytes = c->tf_blk.bytes(curr_kp != nullptr);
    VX_HIP(c, c->tf_host.ensure(bytes));
    VX_HIP(c, hipMemcpyAsync(c->tf_host.p, c->tf_out.p, bytes, hipMemcpyDeviceToHost, c->stream));
    VX_HIP(c, hipStreamSynchronize(c->stream));
    if (c->prof) prof_collect(c);
    const uint8_t* h = static_cast<const uint8_t*>(c->tf_host.p);
    std::memcpy(out, h, sizeof *out);
    c->tf_fetched = true;
    if (n_kp) *n_kp = out->n_keypoints;
    if (curr_kp) {
        if (out->n_keypoints > cap_kp) return set_error(c, VX_ERR_CAPACITY, "need %d keypoints, cap %d", out->n_keypoints, cap_kp);
        if (out->n_keypoints) std::memcpy(curr_kp, h + o_kp, (size_t)out->n_keypoints * sizeof(vx_keypoint));
    }
    return VX_OK;
}

int vx_track_frame_pairs(vx_ctx* c, int which, int32_t* pair_match, uint8_t* mask, int cap_pairs) {
    if (!c) return VX_ERR_INVALID;
    if (which != 0 && which != 1) return set_error(c, VX_ERR_INVALID, "vx_track_frame_pairs: path %d (0 or 1)", which);
    if (!c->tf_valid || !c->tf_fetched) return set_error(c, VX_ERR_STATE, "no vx_track_frame_fetch before vx_track_frame_pairs");
    return trk::copy_pairs(c, static_cast<const uint8_t*>(c->tf_host.p), c->tf_blk, which, pair_match, mask, cap_pairs);
}

int vx_track_frame_matches(vx_ctx* c, int which, const vx_match** d_matches, const int32_t** d_n, int32_t* cap) {
    if (!c) return VX_ERR_INVALID;
    if (which != 0 && which != 1) return set_error(c, VX_ERR_INVALID, "vx_track_frame_matches: list %d (0 or 1)", which);
    if (!c->tf_valid || c->tf_cap[which] <= 0) return set_error(c, VX_ERR_STATE, "vx_track_frame_async enqueued no match %d", which);
    // list 1 may be list 0's rows under its own (gated) count
    const bool shared = which == 1 && !c->tf_list1_own;
    if (d_matches) *d_matches = c->tf_matches[shared ? 0 : which].as<vx_match>();
    if (d_n) *d_n = c->tf_count.as<int32_t>() + 4 * which;
    if (cap) *cap = c->tf_cap[which];
    return VX_OK;
}

}  // extern "C"

static_assert(sizeof(vx_track_frame_result) == 552 && offsetof(vx_track_frame_result, parallax) == 16 &&
                  offsetof(vx_track_frame_result, pose) == 24 && offsetof(vx_track_frame_result, pnp_ran) == 80 &&
                  offsetof(vx_track_frame_result, pnp) == 88 && offsetof(vx_track_frame_result, ess) == 264,
              "vx_track_frame_result layout (python TRACK_FRAME_RESULT_DTYPE)");
