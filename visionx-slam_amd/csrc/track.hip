// track.hip — Tracking::TrackWithPnP (core/frontend/tracking.cpp:332-455) from the match list to the
// pose without leaving the device (vx_track_pnp_async / vx_track_pnp_fetch).
//
// The reference filters the matches by distance (:342-355), builds the 3D-2D pairs with one
// Map::GetLandmark per match (:364-400), calls cv::solvePnPRansac on them (:414-423) and averages
// the pixel displacement of the kept matches (ComputeParallax, :449, :548-560).  Everything those
// steps read is already resident: the match list (match.hip), the current frame's keypoints (an
// extraction slot), the last keyframe's features and the landmarks (vx_dmap), the landmark id ->
// row table (lm_hash.hpp).  One kernel turns them into the device-side problem record the RANSAC
// kernels of ransac.hip read (their correspondence count included), so the sequence is
//
//   k_track_pairs (1 workgroup)  ->  k_pnp_hyp (H, 1)  ->  k_pnp_refine (1)     [pnp_enqueue]
//
// with no host step between and one synchronisation, in the fetch.
//
// k_track_pairs is ONE workgroup: the problem is the match list of one frame pair (at most a few
// thousand entries) and both compactions are ordered (the pairs keep the match order, which is
// what fixes RANSAC's sample stream), so each needs a block-wide exclusive scan; a second
// workgroup would need a second launch or a grid barrier to see the first one's totals.  Its stages:
//   1  min distance       strided loads, wave butterfly + LDS, started at 100.0f (:345-348)
//   2  thr = max(2 min, 30)
//   3  distance filter    match i kept when distance <= thr; kept indices written in match order:
//                         per chunk of kBlock matches a wave64 ballot + mbcnt gives the rank inside
//                         the wave, the wave totals are scanned in LDS, a running base carries over
//   4  pair gather        kept match j (in order): index bounds, feature flags, hash probe, lm_bad,
//                         position checks (:373-394); survivors compacted the same way into
//                         obj (float3), img (float2), pair_match
//   5  parallax           per-thread partial over its kept matches (j = t, t + kBlock, ...), wave
//                         butterfly, wave partials summed in wave order: a fixed order, so the
//                         double result repeats bit for bit
//   6  problem record     offsets {0, n_pairs} (or {0, 0} when a gate of :357 / :402 fails: the RANSAC
//                         kernels then return ok = 0 without a hypothesis), intrinsics, options with
//                         max_iterations resolved (:421)
// No atomics anywhere: every output position comes from a scan.
//
// Block size 1024 (16 waves, 4 per SIMD): the kernel is a chain of dependent global loads per
// match (match -> feature -> hash slot -> lm_bad / lm_pos) on a single CU, so what bounds it is
// how many of those chains are in flight; 1024 threads put a typical 1000-2000 match list through
// each stage in one or two chunks (two __syncthreads per chunk).  Registers are no constraint
// (58 VGPRs, no scratch); LDS: 16 wave counts + 16 wave minima + 16 wave doubles = 256 B.
// The hash probe and the lm_bad / lm_pos reads behind it are the only loads whose address depends
// on another load of the same stage beyond the match record itself.
//
// Host side: TrackArgs is filled and the options checked by track_bodies.hpp's host section; the host-input form
// stages its upload in c->tk_in (vx::StagedUpload, vx_internal.hpp).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "vx_internal.hpp"
#include "dmap.hpp"
#include "track_bodies.hpp"

namespace vx {
namespace {

using trk::kBlock;
using trk::kWaves;

using trk::TrackArgs;

// the stages above, stated in track_pairs_body.inc (shared with k_rig_pairs, track_rig.hip)
__global__ void __launch_bounds__(kBlock) k_track_pairs(TrackArgs a) {
#include "track_pairs_body.inc"
}

// packed result block: vx_track_result | pair_match[cap] | mask[cap] (track_common.hpp)
size_t off_pair_match() { return trk::off_pair_match<vx_track_result>(); }
size_t off_mask(int cap) { return trk::off_mask<vx_track_result>(cap); }
size_t packed_bytes(int cap) { return trk::packed_bytes<vx_track_result>(cap); }

}  // namespace
}  // namespace vx

using namespace vx;

extern "C" {

void vx_track_default_options(vx_track_options* o) {
    if (!o) return;
    o->min_matches = 50;  // Tracking::Options (tracking.h:27-28)
    o->min_inliers = 30;
    vx_pnp_default_options(0, &o->pnp);
    o->pnp.max_iterations = -1;  // min(100, 2 * n_pairs) once n_pairs is known (tracking.cpp:421)
}

int vx_track_block(void) { return kBlock; }

int vx_orb_slot_keypoints(vx_ctx* c, int slot, const vx_keypoint** d_kp) {
    if (!c || !d_kp) return VX_ERR_INVALID;
    if (slot < 0 || slot >= VX_MAX_SLOTS || !c->slots[slot].valid)
        return set_error(c, VX_ERR_STATE, "slot %d holds no extraction", slot);
    *d_kp = c->slots[slot].kp.as<vx_keypoint>();
    return VX_OK;
}

int vx_track_pnp_async(vx_ctx* c, vx_dmap* m, uint64_t last_kf_id, const float* d_curr_xy, int64_t curr_stride_bytes,
                       const int32_t* d_n_curr, const vx_match* d_matches, const int32_t* d_n_matches, int cap_matches,
                       const double* intr4, const vx_track_options* opt) {
    if (!c) return VX_ERR_INVALID;
    if (!m || !m->c || !d_curr_xy || !d_n_curr || !intr4 || !opt)
        return set_error(c, VX_ERR_INVALID, "vx_track_pnp_async: null argument");
    if (curr_stride_bytes < 8 || (curr_stride_bytes & 3))
        return set_error(c, VX_ERR_INVALID, "position stride %lld: a multiple of 4, at least 8", (long long)curr_stride_bytes);
    if (m->c->device != c->device) return set_error(c, VX_ERR_INVALID, "map and context on different devices");
    if (d_matches) {
        if (!d_n_matches || cap_matches < 0) return set_error(c, VX_ERR_INVALID, "match list without a count / capacity");
    } else {
        if (!c->match_valid) return set_error(c, VX_ERR_STATE, "no match enqueued on this context");
        d_matches = c->matches.as<vx_match>();
        d_n_matches = c->match_count.as<int32_t>();
        cap_matches = c->match_cap;
    }
    const auto kf = m->kf_index.find(last_kf_id);
    if (kf == m->kf_index.end())
        return set_error(c, VX_ERR_INVALID, "keyframe %llu is not in the map", (unsigned long long)last_kf_id);
    // (fx + fy != 0 is NOT tested here, unlike trk::check_focal: track_bodies.hpp)
    if (!(intr4[0] != 0.0 && intr4[1] != 0.0)) return set_error(c, VX_ERR_INVALID, "vx_track_pnp_async: zero focal length");
    int rc;
    if ((rc = trk::check_pnp_options(c, "vx_track_pnp_async", opt->pnp))) return rc;
    VX_HIP(c, hipSetDevice(c->device));
    // the id table must hold the landmarks added since the last LocalBA; it belongs to the map, so it
    // is brought up to date on the map context's stream, which this context's stream then follows
    if ((rc = ht_sync(m->c, m))) return set_error(c, rc, "landmark id table: %s", vx_last_error(m->c));
    if ((rc = vx_stream_wait_ctx(c, m->c))) return rc;

    const int cap = std::max(cap_matches, 1);
    VX_HIP(c, c->tk_good.ensure((size_t)cap * sizeof(int)));
    VX_HIP(c, c->tk_obj.ensure((size_t)cap * 3 * sizeof(float)));
    VX_HIP(c, c->tk_img.ensure((size_t)cap * 2 * sizeof(float)));
    VX_HIP(c, c->tk_prob.ensure(trk::prob1_bytes<TrackArgs>()));
    VX_HIP(c, c->tk_out.ensure(packed_bytes(cap)));
    TrackArgs a{};
    a.matches = d_matches;
    a.n_matches = d_n_matches;
    a.cap_matches = cap_matches;
    a.curr_xy = reinterpret_cast<const uint8_t*>(d_curr_xy);
    a.stride = curr_stride_bytes;
    a.n_curr = d_n_curr;
    trk::map_side(a, m, kf->second);
    trk::set_options(a, *opt, intr4);
    a.good = c->tk_good.as<int>();
    a.obj = c->tk_obj.as<float>();
    a.img = c->tk_img.as<float>();
    trk::packed_outputs(a, c->tk_out.as<uint8_t>(), cap);
    trk::prob1_pointers(a, c->tk_prob.as<uint8_t>());
    c->tk_valid = false;
    VX_HIP(c, launch(c, kStTrackPairs, k_track_pairs, dim3(1), dim3(kBlock), 0, c->stream, a));
    PnpDeviceArgs d{};
    d.offsets = a.offsets;
    d.intr = a.intr_out;
    d.opt = a.opt_out;
    d.obj = a.obj;
    d.img = a.img;
    d.out = &a.res->pnp;
    d.mask = a.mask;
    if ((rc = pnp_enqueue(c, 1, trk::pnp_hyp_bound(opt->pnp), d, c->tk_hyp))) return rc;
    c->tk_cap = cap;
    c->tk_min_matches = opt->min_matches;
    c->tk_min_inliers = opt->min_inliers;
    c->tk_valid = true;
    return VX_OK;
}

int vx_track_pnp_host_async(vx_ctx* c, vx_dmap* m, uint64_t last_kf_id, const uint8_t* query_desc, int n_query,
                            const uint8_t* train_desc, int n_train, const float* curr_xy, float ratio,
                            const double* intr4, const vx_track_options* opt) {
    if (!c) return VX_ERR_INVALID;
    if (n_query < 0 || n_train < 0 || (n_query && !query_desc) || (n_train && (!train_desc || !curr_xy)))
        return set_error(c, VX_ERR_INVALID, "vx_track_pnp_host_async: bad descriptor / position arguments");
    VX_HIP(c, hipSetDevice(c->device));
    // one staged block: {n_query, n_train} | query rows | train rows | positions.  The row capacities
    // (what the match is enqueued with; the counts are read on the device) are rounded up to 256 so
    // frames with about as many features share one launch configuration (its captured graph).
    const int cap_q = (std::max(n_query, 1) + 255) & ~255, cap_t = (std::max(n_train, 1) + 255) & ~255;
    const size_t o_q = 16, o_t = o_q + (size_t)cap_q * 32, o_xy = o_t + (size_t)cap_t * 32,
                 bytes = o_xy + (size_t)cap_t * 8;
    // (the one place this entry can block: until the previous call's upload has left the staging)
    VX_HIP(c, c->tk_in.begin(bytes));
    uint8_t* h = static_cast<uint8_t*>(c->tk_in.host.p);
    const int32_t counts[4] = {n_query, n_train, 0, 0};
    std::memcpy(h, counts, sizeof counts);
    // rows between the counts and the rounded capacities are not filled: the match kernels stop at
    // the device-side counts, so what the upload carries there is never read
    if (n_query) std::memcpy(h + o_q, query_desc, (size_t)n_query * 32);
    if (n_train) {
        std::memcpy(h + o_t, train_desc, (size_t)n_train * 32);
        std::memcpy(h + o_xy, curr_xy, (size_t)n_train * 8);
    }
    VX_HIP(c, c->tk_in.upload(bytes, c->stream));
    const uint8_t* d = c->tk_in.dev.as<uint8_t>();
    const int32_t* dn = c->tk_in.dev.as<int32_t>();
    int rc;
    if ((rc = vx_match_device_async(c, d + o_q, dn, cap_q, d + o_t, dn + 1, cap_t, ratio))) return rc;
    // the list just enqueued, named explicitly with the capacity it was enqueued with
    return vx_track_pnp_async(c, m, last_kf_id, reinterpret_cast<const float*>(d + o_xy), 8, dn + 1,
                              c->matches.as<vx_match>(), c->match_count.as<int32_t>(), cap_q, intr4, opt);
}

int vx_track_pnp_fetch(vx_ctx* c, vx_track_result* out, int32_t* pair_match, uint8_t* inlier_mask, int cap_pairs) {
    if (!c || !out) return c ? set_error(c, VX_ERR_INVALID, "vx_track_pnp_fetch: null result") : VX_ERR_INVALID;
    if (!c->tk_valid) return set_error(c, VX_ERR_STATE, "no vx_track_pnp_async enqueued");
    VX_HIP(c, hipSetDevice(c->device));
    const size_t bytes = packed_bytes(c->tk_cap);
    VX_HIP(c, c->tk_host.ensure(bytes));
    VX_HIP(c, hipMemcpyAsync(c->tk_host.p, c->tk_out.p, bytes, hipMemcpyDeviceToHost, c->stream));
    VX_HIP(c, hipStreamSynchronize(c->stream));
    if (c->prof) prof_collect(c);
    const uint8_t* h = static_cast<const uint8_t*>(c->tk_host.p);
    std::memcpy(out, h, sizeof *out);
    out->status = trk::pnp_status(*out, c->tk_min_matches, c->tk_min_inliers);  // (track_common.hpp)
    const int np = out->n_pairs;
    if ((pair_match || inlier_mask) && np > cap_pairs)
        return set_error(c, VX_ERR_CAPACITY, "need %d pairs, cap %d", np, cap_pairs);
    if (pair_match && np) std::memcpy(pair_match, h + off_pair_match(), (size_t)np * sizeof(int32_t));
    if (inlier_mask && np) std::memcpy(inlier_mask, h + off_mask(c->tk_cap), (size_t)np);
    return VX_OK;
}

}  // extern "C"

static_assert(sizeof(vx_track_options) == 40, "vx_track_options layout (python TRACK_OPTIONS_DTYPE)");
static_assert(sizeof(vx_track_result) == 176, "vx_track_result layout (python TRACK_RESULT_DTYPE)");
static_assert(sizeof(vx_keypoint) == 20, "vx_keypoint rows as a position array of stride 20");
