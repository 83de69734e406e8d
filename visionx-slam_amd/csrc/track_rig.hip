// track_rig.hip — Tracking::Track (core/frontend/tracking.cpp:267-279) for every camera of a rig time
// step over one shared map as ONE stream-ordered sequence and ONE synchronisation
// (vx_track_rig_async / vx_track_rig_fetch).
//
// vx_track_frame_async (track_frame.hip) tracks one camera in 15 launches that are bound by launch
// latency, not work; a rig of B cameras pays them B times, with B synchronisations, and cannot overlap
// two cameras on one context (the call owns tk_* / te_* / tf_*).  Here camera = workgroup or grid row
// of every kernel, so the number of launches (17, or 19 when ess_enqueue splits k_em_hyp by grid size) does not depend on B:
//
//   Match(last_kf_i, curr_i) for all i      k_knn_rows_batch + k_knn_compact_batch (match_batch_enqueue_to)
//   k_rig_pairs     grid = cameras           camera i = workgroup i: k_track_pairs' stages 1-6 on table entry i
//   k_rig_pack      grid (chunks, cameras)   exclusive prefix of the per-camera problem sizes -> offsets[P + 1];
//                                            the obj / img segments moved to their contiguous places
//   pnp_enqueue(P = cameras)                 unchanged kernels (ransac.hip)
//   k_rig_gate      one workgroup            lane i: camera i's PnP record completed, trk::track_gate on it
//   Match(last_i, curr_i) under the gated counts
//   k_rig_epairs    grid = cameras           k_track_epairs' stages per camera
//   k_rig_pack      (essential form: p1 / p2)
//   ess_enqueue(P = cameras)                 unchanged kernels (essential.hip)
//   k_rig_epose     one workgroup            lane i: camera i's essential record completed, trk::track_epose
//   k_rig_final     grid (chunks, cameras)   trk::track_final per camera, the masks read from the camera's slice
//                                            of the contiguous RANSAC masks
//
// Why a pack step: the RANSAC kernels read problem p as [offsets[p], offsets[p + 1]) of ONE contiguous
// correspondence array, and the per-camera pair counts exist on the device only.  So the pair kernels
// write capacity-strided segments (camera i's first slot = the sum of the capacities before it, known
// on the host) and k_rig_pack, which reads all the counts, places them; the other choice — a pair
// kernel that learns its base from the cameras before it — needs a second launch or a grid barrier.
// The RANSAC kernels stay untouched; their masks come back indexed by packed position and k_rig_final
// reads camera i's at offsets[i].
//
// Equal bytes are expected: RANSAC's sample stream depends on the seed and the hypothesis index only,
// the batched match and both batched RANSACs are bit-exact per problem, both compactions of a camera
// stay ONE ordered 1024-thread workgroup, and the rules are the single call's own program text
// (track_bodies.hpp, track_*pairs_body.inc).  No atomics anywhere: every position comes from a scan or
// from a prefix over at most 16 counts that each workgroup recomputes for itself.
//
// The per-camera arguments (RigCam: five argument records, about 1 KB) do not fit kernel arguments 16
// times over: one table is staged in pinned memory and uploaded in one copy per call, the staging
// guarded by an event as in the *_host_async forms (c->tr_tab, vx::StagedUpload).  The kernels read their entry
// through uniform addresses (scalar loads).  An entry is filled by the single call's fillers (track_bodies.hpp's host
// section), which also state the checks, the block layout (trk::FrameBlock, tr_cam[i].blk) and the problem records.
//
// Every kernel is bound by launch latency at rig sizes (a camera's work is the single call's).
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950; VGPRs / SGPRs / LDS / scratch):
//   k_rig_pairs 61 / 88 / 256 B / 0      k_rig_epairs 63 / 74 / 256 B / 0    k_rig_pack 10 / 36 / 0 / 0
//   k_rig_gate  44 / 22 / 0 / 0          k_rig_epose  67 / 16 / 0 / 0        k_rig_final 28 / 62 / 0 / 0
#include <algorithm>
#include <cstddef>
#include <cstring>

#include "vx_internal.hpp"
#include "dmap.hpp"
#include "track_bodies.hpp"

namespace vx {
namespace {

using trk::kBlock;
using trk::kProbCnt;
using trk::kProbIntr;
using trk::kProbOffsets;
using trk::kProbOpt;

constexpr int kPackBlock = 256;
constexpr int kPackMaxWg = 16;
constexpr int kFinalBlock = 256;
constexpr int kFinalMaxWg = 64;
constexpr int kP = VX_MAX_RIG_CAMERAS;

// one camera's arguments: the single call's five argument records
struct RigCam {
    trk::TrackArgs tk;   // tk.matches == NULL: no last keyframe (an empty PnP problem)
    trk::EPairArgs te;
    trk::GateArgs g;
    trk::EPoseArgs ep;
    trk::FinalArgs f;
};

// camera = workgroup: k_track_pairs' stages on the camera's own table entry
__global__ void __launch_bounds__(kBlock) k_rig_pairs(const RigCam* __restrict__ tab) {
    const trk::TrackArgs& a = tab[blockIdx.x].tk;
    if (!a.matches) {  // (block-uniform) no last keyframe: the empty problem {0, 0}; no record (k_rig_final zeroes it)
        if (threadIdx.x == 0) {
            a.offsets[0] = 0;
            a.offsets[1] = 0;
            for (int k = 0; k < 4; ++k) a.intr_out[k] = a.intr[k];
            vx_pnp_options o = a.pnp;
            if (o.max_iterations < 0) o.max_iterations = 0;
            *a.opt_out = o;
        }
        return;
    }
#include "track_pairs_body.inc"
}

__global__ void __launch_bounds__(kBlock) k_rig_epairs(const RigCam* __restrict__ tab) {
    const trk::EPairArgs& a = tab[blockIdx.x].te;
#include "track_epairs_body.inc"
}

// The cameras' capacity-strided pair segments into the contiguous arrays the RANSAC kernels read.
// Camera c = blockIdx.y owns n_c = cnt[2 c + 1] pairs (the {0, n} record its pair kernel wrote) at
// slots [seg[c], seg[c] + n_c) of src_a (wa floats a pair) and src_b (wb floats a pair); they go to
// [off_c, off_c + n_c) with off_c = n_0 + ... + n_(c-1), recomputed by every workgroup from the <= 16
// counts.  The packed mask is zeroed over the same positions; offsets[0 .. n_cams] by workgroup (0, 0).
// n_c <= the camera's capacity (the pair kernels compact at most cap_matches matches), so every read
// stays inside the camera's segment and every write below the sum of the capacities.
struct PackArgs {
    const int* cnt;
    int n_cams;
    int64_t seg[kP];
    const float* src_a;
    float* dst_a;
    int wa;
    const float* src_b;
    float* dst_b;
    int wb;
    uint8_t* mask;
    int* offsets;
};

__global__ void __launch_bounds__(kPackBlock) k_rig_pack(PackArgs a) {
    const int cam = blockIdx.y;
    int64_t off = 0;
    for (int j = 0; j < cam; ++j) off += max(a.cnt[2 * j + 1], 0);
    const int64_t n = max(a.cnt[2 * cam + 1], 0), seg = a.seg[cam];
    const int64_t t = (int64_t)blockIdx.x * kPackBlock + threadIdx.x, nt = (int64_t)gridDim.x * kPackBlock;
    for (int64_t k = t; k < n * a.wa; k += nt) a.dst_a[off * a.wa + k] = a.src_a[seg * a.wa + k];
    for (int64_t k = t; k < n * a.wb; k += nt) a.dst_b[off * a.wb + k] = a.src_b[seg * a.wb + k];
    for (int64_t k = t; k < n; k += nt) a.mask[off + k] = 0;
    if (blockIdx.x == 0 && cam == 0 && (int)threadIdx.x <= a.n_cams) {
        int o = 0;
        for (int j = 0; j < (int)threadIdx.x; ++j) o += max(a.cnt[2 * j + 1], 0);
        a.offsets[threadIdx.x] = o;
    }
}

// lane i = camera i: the PnP record k_pnp_refine wrote into the batch's result array goes into the
// camera's vx_track_result, then the single call's rule on it
__global__ void __launch_bounds__(64) k_rig_gate(const RigCam* __restrict__ tab, int n_cams,
                                                 const vx_pnp_result* __restrict__ pnp_out) {
    const int i = threadIdx.x;
    if (i >= n_cams) return;
    const RigCam& r = tab[i];
    if (r.tk.matches) r.tk.res->pnp = pnp_out[i];
    trk::track_gate(r.g);
}

// lane i = camera i: the essential record of the batch's result array into the camera's record, then T_cl * T_lw
__global__ void __launch_bounds__(64) k_rig_epose(const RigCam* __restrict__ tab, int n_cams,
                                                  const vx_essential_result* __restrict__ ess_out) {
    const int i = threadIdx.x;
    if (i >= n_cams) return;
    const RigCam& r = tab[i];
    r.ep.res->ess = ess_out[i];
    trk::track_epose(r.ep);
}

// camera = blockIdx.y: the single call's final block.  A path's mask is the camera's slice of the
// contiguous RANSAC mask when its problem ran (offsets[c + 1] > offsets[c]); otherwise the camera's
// own zeroed mask (the pair kernel's), as the single call's RANSAC leaves it on the empty problem.
__global__ void __launch_bounds__(kFinalBlock) k_rig_final(const RigCam* __restrict__ tab, const int* __restrict__ off0,
                                                           const uint8_t* __restrict__ mask0,
                                                           const int* __restrict__ off1,
                                                           const uint8_t* __restrict__ mask1) {
    const int cam = blockIdx.y;
    const trk::FinalArgs& a = tab[cam].f;
    const size_t t = (size_t)blockIdx.x * kFinalBlock + threadIdx.x, nt = (size_t)gridDim.x * kFinalBlock;
    const uint8_t* m0 = off0[cam + 1] > off0[cam] ? mask0 + off0[cam] : a.tk + trk::off_mask<vx_track_result>(a.tk_cap);
    const uint8_t* m1 =
        off1[cam + 1] > off1[cam] ? mask1 + off1[cam] : a.te + trk::off_mask<vx_track_essential_result>(a.te_cap);
    trk::track_final<true>(a, m0, m1, t, nt);
}

// a running 256-byte aligned sub-allocation of one device buffer
struct Carve {
    size_t at = 0;
    size_t take(size_t bytes) {
        const size_t o = at;
        at += (bytes + 255) & ~(size_t)255;
        return o;
    }
};

int check_cam(vx_ctx* c, int cam, const char* what) {
    if (cam < 0 || cam >= c->tr_n) return set_error(c, VX_ERR_INVALID, "%s: camera %d outside [0, %d)", what, cam, c->tr_n);
    return VX_OK;
}

}  // namespace
}  // namespace vx

using namespace vx;

extern "C" {

int vx_track_rig_layout(int n_cams, const int32_t* cap_pairs0, const int32_t* cap_pairs1, const int32_t* cap_kp,
                        int64_t* cam_offset, int64_t* total_bytes) {
    if (n_cams < 1 || n_cams > VX_MAX_RIG_CAMERAS || !cap_pairs0 || !cap_pairs1 || !cap_kp) return VX_ERR_INVALID;
    size_t at = 0;
    for (int i = 0; i < n_cams; ++i) {
        if (cap_pairs0[i] < 0 || cap_pairs1[i] < 0 || cap_kp[i] < 0) return VX_ERR_INVALID;
        if (cam_offset) cam_offset[i] = (int64_t)at;
        at += trk::FrameBlock{cap_pairs0[i], cap_pairs1[i], cap_kp[i]}.bytes(true);  // (a sum of multiples of 16)
    }
    if (total_bytes) *total_bytes = (int64_t)at;
    return VX_OK;
}

int vx_track_rig_async(vx_ctx* c, vx_dmap* m, int n_cams, const vx_rig_camera* cams, float ratio,
                       const vx_track_options* pnp_opt, const vx_track_essential_options* ess_opt) {
    if (!c) return VX_ERR_INVALID;
    if (n_cams < 1 || n_cams > VX_MAX_RIG_CAMERAS)
        return set_error(c, VX_ERR_INVALID, "vx_track_rig_async: %d cameras outside [1, %d]", n_cams, VX_MAX_RIG_CAMERAS);
    if (!cams || !ess_opt) return set_error(c, VX_ERR_INVALID, "vx_track_rig_async: null argument");
    // ---- vx_track_frame_async's checks (and those of the two calls it runs), camera by camera
    const char* call = "vx_track_rig_async";
    int rc;
    bool any_kf = false;
    for (int i = 0; i < n_cams; ++i) {
        const vx_rig_camera& k = cams[i];
        char who[48];
        std::snprintf(who, sizeof who, "%s: camera %d", call, i);
        if ((rc = trk::check_frames(c, who, m, m && m->c && pnp_opt, k.last_kf_id, k.last_kf, k.last, k.curr, k.intr4))) return rc;
        if ((rc = trk::check_focal(c, who, k.intr4))) return rc;
        any_kf |= k.last_kf != nullptr;
    }
    if (any_kf) {
        if (m->c->device != c->device) return set_error(c, VX_ERR_INVALID, "%s: map and context on different devices", call);
        if ((rc = trk::check_pnp_options(c, call, pnp_opt->pnp))) return rc;
    }
    if ((rc = trk::check_ess_options(c, call, ess_opt->ess))) return rc;
    VX_HIP(c, hipSetDevice(c->device));
    // (as vx_track_frame_async: a call refused for its arguments leaves the previous call's result in place)
    c->tr_valid = c->tr_fetched = c->tr_fetched_kp = false;
    c->tr_n = 0;
    if (any_kf) {  // as vx_track_pnp_async: the id table up to date on the map's stream, which this stream then follows
        if ((rc = ht_sync(m->c, m))) return set_error(c, rc, "landmark id table: %s", vx_last_error(m->c));
        if ((rc = vx_stream_wait_ctx(c, m->c))) return rc;
    }
    vx_track_options po;
    if (pnp_opt) po = *pnp_opt;
    else vx_track_default_options(&po);  // (only empty problems read it)

    // ---- capacities
    int cap0[kP], cap1[kP], pc0[kP], pc1[kP], ckp[kP];
    int64_t seg0[kP + 1], seg1[kP + 1];
    int q_cap0 = 1, q_cap1 = 1, t_cap = 1;
    seg0[0] = seg1[0] = 0;
    for (int i = 0; i < n_cams; ++i) {
        const vx_rig_camera& k = cams[i];
        const vx_frame* q1 = k.last ? k.last : k.curr;
        cap0[i] = k.last_kf ? k.last_kf->cap : 0;
        cap1[i] = q1->cap;
        pc0[i] = k.last_kf ? std::max(cap0[i], 1) : 0;
        pc1[i] = std::max(cap1[i], 1);
        ckp[i] = k.curr->cap;
        seg0[i + 1] = seg0[i] + pc0[i];
        seg1[i + 1] = seg1[i] + pc1[i];
        q_cap0 = std::max(q_cap0, cap0[i]);
        q_cap1 = std::max(q_cap1, cap1[i]);
        t_cap = std::max(t_cap, k.curr->cap);
    }
    const int64_t slots = std::max<int64_t>(std::max(seg0[n_cams], seg1[n_cams]), 1);
    int64_t cam_off[kP], total = 0;
    if (vx_track_rig_layout(n_cams, pc0, pc1, ckp, cam_off, &total) != VX_OK) return set_error(c, VX_ERR_INVALID, "vx_track_rig_async: layout");

    // ---- buffers
    Carve cm;  // tr_match
    const size_t o_best = cm.take((size_t)n_cams * std::max(q_cap0, q_cap1) * sizeof(unsigned));
    const size_t o_list0 = cm.take((size_t)n_cams * q_cap0 * sizeof(vx_match));
    const size_t o_list1 = cm.take((size_t)n_cams * q_cap1 * sizeof(vx_match));
    const size_t o_count = cm.take(2 * kP * 16);  // list w of camera i: int32[4] at (w * kP + i) * 16
    const size_t o_gate = cm.take(kP * 16);       // camera i: {gated query count, PnP status, gate open, 0}
    Carve cw;  // tr_work
    const size_t o_good = cw.take((size_t)slots * sizeof(int));
    const size_t o_sega = cw.take((size_t)slots * 3 * sizeof(float));
    const size_t o_segb = cw.take((size_t)slots * 2 * sizeof(float));
    const size_t o_pka = cw.take((size_t)slots * 3 * sizeof(float));
    const size_t o_pkb = cw.take((size_t)slots * 2 * sizeof(float));
    const size_t o_mask0 = cw.take((size_t)slots);
    const size_t o_mask1 = cw.take((size_t)slots);
    const size_t o_prob0 = cw.take(trk::prob_bytes<trk::TrackArgs>());
    const size_t o_prob1 = cw.take(trk::prob_bytes<trk::EPairArgs>());
    const size_t o_res0 = cw.take(kP * sizeof(vx_pnp_result));
    const size_t o_res1 = cw.take(kP * sizeof(vx_essential_result));
    size_t o_tk[kP], o_te[kP];
    for (int i = 0; i < n_cams; ++i) {
        o_tk[i] = cw.take(trk::packed_bytes<vx_track_result>(std::max(pc0[i], 1)));
        o_te[i] = cw.take(trk::packed_bytes<vx_track_essential_result>(pc1[i]));
    }
    // A query count of 0 (list 0 of a camera without a last keyframe) in a buffer of its own: its place never
    // depends on a call's sizes, it is zeroed when it is allocated, and no kernel is ever given it to write.
    if (!c->tr_zero.p) {
        VX_HIP(c, c->tr_zero.ensure(16));
        VX_HIP(c, hipMemsetAsync(c->tr_zero.p, 0, 16, c->stream));
    }
    VX_HIP(c, c->tr_match.ensure(cm.at));
    VX_HIP(c, c->tr_work.ensure(cw.at));
    VX_HIP(c, c->tr_out.ensure((size_t)total));
    uint8_t* dm = c->tr_match.as<uint8_t>();
    uint8_t* dw = c->tr_work.as<uint8_t>();
    uint8_t* dout = c->tr_out.as<uint8_t>();
    unsigned* best = reinterpret_cast<unsigned*>(dm + o_best);
    vx_match* list0 = reinterpret_cast<vx_match*>(dm + o_list0);
    vx_match* list1 = reinterpret_cast<vx_match*>(dm + o_list1);
    int32_t* count0 = reinterpret_cast<int32_t*>(dm + o_count);
    int32_t* count1 = count0 + 4 * kP;
    int32_t* gate = reinterpret_cast<int32_t*>(dm + o_gate);
    const int32_t* zero = c->tr_zero.as<int32_t>();
    int* good = reinterpret_cast<int*>(dw + o_good);
    float* sega = reinterpret_cast<float*>(dw + o_sega);
    float* segb = reinterpret_cast<float*>(dw + o_segb);
    float* pka = reinterpret_cast<float*>(dw + o_pka);
    float* pkb = reinterpret_cast<float*>(dw + o_pkb);
    uint8_t* prob0 = dw + o_prob0;
    uint8_t* prob1 = dw + o_prob1;
    vx_pnp_result* res0 = reinterpret_cast<vx_pnp_result*>(dw + o_res0);
    vx_essential_result* res1 = reinterpret_cast<vx_essential_result*>(dw + o_res1);

    // ---- the argument table, staged and uploaded in one copy
    VX_HIP(c, c->tr_tab.begin(kP * sizeof(RigCam)));
    RigCam* tab = static_cast<RigCam*>(c->tr_tab.host.p);
    std::memset(tab, 0, (size_t)n_cams * sizeof(RigCam));
    const int64_t stride = (int64_t)sizeof(vx_keypoint);
    const uint8_t *mq0[kP], *mq1[kP], *mt[kP];
    const int *mnq0[kP], *mnq1[kP], *mnt[kP];
    for (int i = 0; i < n_cams; ++i) {
        const vx_rig_camera& k = cams[i];
        const vx_frame* q1 = k.last ? k.last : k.curr;  // (no last frame: the current rows under a gated count of 0)
        RigCam& r = tab[i];
        uint8_t* tkb = dw + o_tk[i];
        uint8_t* teb = dw + o_te[i];
        const uint8_t* curr_xy = reinterpret_cast<const uint8_t*>(&k.curr->kp()->x);
        // the matches' pairs
        mq0[i] = k.last_kf ? k.last_kf->desc() : k.curr->desc();
        mnq0[i] = k.last_kf ? k.last_kf->count() : zero;
        mq1[i] = q1->desc();
        mnq1[i] = gate + 4 * i;
        mt[i] = k.curr->desc();
        mnt[i] = k.curr->count();
        // what the fetches read of this camera (the call is not valid before its last launch is enqueued)
        vx_ctx::RigCam& h = c->tr_cam[i];
        h.cap[0] = cap0[i];
        h.cap[1] = cap1[i];
        h.blk = {pc0[i], pc1[i], ckp[i]};
        h.list[0] = list0 + (size_t)i * q_cap0;
        h.list[1] = list1 + (size_t)i * q_cap1;
        h.count[0] = count0 + 4 * i;
        h.count[1] = count1 + 4 * i;
        h.offset = cam_off[i];
        // TrackWithPnP's pairs
        trk::TrackArgs& a = r.tk;
        if (k.last_kf) {
            a.matches = list0 + (size_t)i * q_cap0;
            a.n_matches = count0 + 4 * i;
            a.cap_matches = cap0[i];
            a.curr_xy = curr_xy;
            a.stride = stride;
            a.n_curr = k.curr->count();
            trk::map_side(a, m, m->kf_index.find(k.last_kf_id)->second);
            a.good = good + seg0[i];
            a.obj = sega + 3 * seg0[i];
            a.img = segb + 2 * seg0[i];
            trk::packed_outputs(a, tkb, pc0[i]);
        }
        trk::set_options(a, po, k.intr4);
        trk::prob_pointers(a, prob0, i);
        // the decision (n_matches0 / n_matches1 stay NULL: with last_kf == last the fallback match runs again under the gate)
        trk::gate_args(r.g, k.last_kf ? reinterpret_cast<const vx_track_result*>(tkb) : nullptr, &po, k.last, gate + 4 * i);
        // TrackLastFrame's pairs
        trk::EPairArgs& e = r.te;
        e.matches = list1 + (size_t)i * q_cap1;
        e.n_matches = count1 + 4 * i;
        e.cap_matches = cap1[i];
        e.last_xy = reinterpret_cast<const uint8_t*>(&q1->kp()->x);
        e.last_stride = stride;
        e.n_last = gate + 4 * i;
        e.curr_xy = curr_xy;
        e.curr_stride = stride;
        e.n_curr = k.curr->count();
        trk::set_options(e, *ess_opt, k.intr4);
        e.good = good + seg1[i];
        e.p1 = sega + 2 * seg1[i];
        e.p2 = segb + 2 * seg1[i];
        trk::packed_outputs(e, teb, pc1[i]);
        trk::prob_pointers(e, prob1, i);
        // T_cl * T_lw; the head and the packed block
        trk::epose_args(r.ep, e.res, k.pose_last7);
        trk::final_args(r.f, k.last_kf ? tkb : nullptr, teb, h.blk, gate + 4 * i, k.last != nullptr, *ess_opt, k.curr, dout + cam_off[i]);
    }
    VX_HIP(c, c->tr_tab.upload((size_t)n_cams * sizeof(RigCam), c->stream));
    const RigCam* dtab = c->tr_tab.dev.as<RigCam>();

    // ---- 1 + 2: Match(last_kf_i, curr_i) and TrackWithPnP's chain on all of them (:340-455)
    if ((rc = match_batch_enqueue_to(c, n_cams, mq0, mnq0, mt, mnt, q_cap0, t_cap, ratio, best, list0, count0))) return rc;
    VX_HIP(c, launch(c, kStRigPairs, k_rig_pairs, dim3(n_cams), dim3(kBlock), 0, c->stream, dtab));
    PackArgs pk{};
    pk.n_cams = n_cams;
    pk.cnt = reinterpret_cast<const int*>(prob0 + kProbCnt);
    for (int i = 0; i < n_cams; ++i) pk.seg[i] = seg0[i];
    pk.src_a = sega;
    pk.dst_a = pka;
    pk.wa = 3;
    pk.src_b = segb;
    pk.dst_b = pkb;
    pk.wb = 2;
    pk.mask = dw + o_mask0;
    pk.offsets = reinterpret_cast<int*>(prob0 + kProbOffsets);
    const int pack_wg0 = std::max(1, std::min(kPackMaxWg, (3 * q_cap0 + kPackBlock - 1) / kPackBlock));
    VX_HIP(c, launch(c, kStRigPack, k_rig_pack, dim3(pack_wg0, n_cams), dim3(kPackBlock), 0, c->stream, pk));
    PnpDeviceArgs pd{};
    pd.offsets = pk.offsets;
    pd.intr = reinterpret_cast<const double*>(prob0 + kProbIntr);
    pd.opt = reinterpret_cast<const vx_pnp_options*>(prob0 + kProbOpt);
    pd.obj = pka;
    pd.img = pkb;
    pd.out = res0;
    pd.mask = dw + o_mask0;
    if ((rc = pnp_enqueue(c, n_cams, trk::pnp_hyp_bound(po.pnp), pd, c->tr_hyp[0]))) return rc;
    // ---- 3: the decision of :269-273, per camera
    VX_HIP(c, launch(c, kStRigGate, k_rig_gate, dim3(1), dim3(64), 0, c->stream, dtab, n_cams, (const vx_pnp_result*)res0));
    // ---- 4 + 5: Match(last_i, curr_i) under the gated counts and TrackLastFrame's chain (:287-325)
    if ((rc = match_batch_enqueue_to(c, n_cams, mq1, mnq1, mt, mnt, q_cap1, t_cap, ratio, best, list1, count1))) return rc;
    VX_HIP(c, launch(c, kStRigEPairs, k_rig_epairs, dim3(n_cams), dim3(kBlock), 0, c->stream, dtab));
    pk.cnt = reinterpret_cast<const int*>(prob1 + kProbCnt);
    for (int i = 0; i < n_cams; ++i) pk.seg[i] = seg1[i];
    pk.wa = 2;
    pk.mask = dw + o_mask1;
    pk.offsets = reinterpret_cast<int*>(prob1 + kProbOffsets);
    const int pack_wg1 = std::max(1, std::min(kPackMaxWg, (2 * q_cap1 + kPackBlock - 1) / kPackBlock));
    VX_HIP(c, launch(c, kStRigPack, k_rig_pack, dim3(pack_wg1, n_cams), dim3(kPackBlock), 0, c->stream, pk));
    EmDeviceArgs ed{};
    ed.offsets = pk.offsets;
    ed.intr = reinterpret_cast<const double*>(prob1 + kProbIntr);
    ed.opt = reinterpret_cast<const vx_essential_options*>(prob1 + kProbOpt);
    ed.p1 = pka;
    ed.p2 = pkb;
    ed.out = res1;
    ed.mask = dw + o_mask1;
    // (the per-match grids are sized by the largest camera's capacity: the pair counts are on the device)
    if ((rc = ess_enqueue(c, n_cams, std::max(1, ess_opt->ess.max_iterations), q_cap1, ed, c->tr_hyp[1]))) return rc;
    VX_HIP(c, launch(c, kStRigEPose, k_rig_epose, dim3(1), dim3(64), 0, c->stream, dtab, n_cams, (const vx_essential_result*)res1));
    // ---- 6: the heads and the packed blocks
    const size_t items = ((size_t)t_cap * sizeof(vx_keypoint)) / 16 + 1;
    const int fgrid = (int)std::min<size_t>(kFinalMaxWg, (items + kFinalBlock - 1) / kFinalBlock);
    VX_HIP(c, launch(c, kStRigFinal, k_rig_final, dim3(std::max(fgrid, 1), n_cams), dim3(kFinalBlock), 0, c->stream, dtab,
                     (const int*)(prob0 + kProbOffsets), (const uint8_t*)(dw + o_mask0), (const int*)(prob1 + kProbOffsets),
                     (const uint8_t*)(dw + o_mask1)));
    c->tr_n = n_cams;
    c->tr_bytes = total;
    c->tr_valid = true;
    return VX_OK;
}

int vx_track_rig_fetch(vx_ctx* c, int with_keypoints, vx_track_frame_result* out, int cap_cams, int* n_cams) {
    if (!c) return VX_ERR_INVALID;
    if (cap_cams < 0 || (cap_cams > 0 && !out)) return set_error(c, VX_ERR_INVALID, "vx_track_rig_fetch: records without an array");
    if (!c->tr_valid) return set_error(c, VX_ERR_STATE, "no vx_track_rig_async enqueued");
    VX_HIP(c, hipSetDevice(c->device));
    // the keypoint rows are each part's tail: without them the copy ends before the last part's
    const vx_ctx::RigCam& lastc = c->tr_cam[c->tr_n - 1];
    const size_t bytes = with_keypoints ? (size_t)c->tr_bytes : (size_t)lastc.offset + lastc.blk.bytes(false);
    VX_HIP(c, c->tr_host.ensure((size_t)c->tr_bytes));
    VX_HIP(c, hipMemcpyAsync(c->tr_host.p, c->tr_out.p, bytes, hipMemcpyDeviceToHost, c->stream));
    VX_HIP(c, hipStreamSynchronize(c->stream));
    if (c->prof) prof_collect(c);
    c->tr_fetched = true;
    c->tr_fetched_kp = with_keypoints != 0;
    if (n_cams) *n_cams = c->tr_n;
    if (cap_cams > 0 && cap_cams < c->tr_n) return set_error(c, VX_ERR_CAPACITY, "need %d records, cap %d", c->tr_n, cap_cams);
    const uint8_t* h = static_cast<const uint8_t*>(c->tr_host.p);
    if (cap_cams > 0)
        for (int i = 0; i < c->tr_n; ++i) std::memcpy(out + i, h + c->tr_cam[i].offset, sizeof *out);
    return VX_OK;
}

int vx_track_rig_pairs(vx_ctx* c, int cam, int which, int32_t* pair_match, uint8_t* mask, int cap_pairs) {
    if (!c) return VX_ERR_INVALID;
    if (which != 0 && which != 1) return set_error(c, VX_ERR_INVALID, "vx_track_rig_pairs: path %d (0 or 1)", which);
    if (!c->tr_valid || !c->tr_fetched) return set_error(c, VX_ERR_STATE, "no vx_track_rig_fetch before vx_track_rig_pairs");
    int rc;
    if ((rc = check_cam(c, cam, "vx_track_rig_pairs"))) return rc;
    const vx_ctx::RigCam& k = c->tr_cam[cam];
    return trk::copy_pairs(c, static_cast<const uint8_t*>(c->tr_host.p) + k.offset, k.blk, which, pair_match, mask, cap_pairs);
}

int vx_track_rig_keypoints(vx_ctx* c, int cam, vx_keypoint* kp, int cap, int* n) {
    if (!c) return VX_ERR_INVALID;
    if (!n || cap < 0) return set_error(c, VX_ERR_INVALID, "vx_track_rig_keypoints: null count / negative capacity");
    if (!c->tr_valid || !c->tr_fetched || !c->tr_fetched_kp)
        return set_error(c, VX_ERR_STATE, "no vx_track_rig_fetch with keypoints before vx_track_rig_keypoints");
    int rc;
    if ((rc = check_cam(c, cam, "vx_track_rig_keypoints"))) return rc;
    const vx_ctx::RigCam& k = c->tr_cam[cam];
    const uint8_t* h = static_cast<const uint8_t*>(c->tr_host.p) + k.offset;
    const int nk = std::min(std::max(reinterpret_cast<const vx_track_frame_result*>(h)->n_keypoints, 0), k.blk.cap_kp);
    *n = nk;
    if (kp && nk > cap) return set_error(c, VX_ERR_CAPACITY, "need %d keypoints, cap %d", nk, cap);
    if (kp && nk) std::memcpy(kp, h + k.blk.kp(), (size_t)nk * sizeof(vx_keypoint));
    return VX_OK;
}

int vx_track_rig_matches(vx_ctx* c, int cam, int which, const vx_match** d_matches, const int32_t** d_n, int32_t* cap) {
    if (!c) return VX_ERR_INVALID;
    if (which != 0 && which != 1) return set_error(c, VX_ERR_INVALID, "vx_track_rig_matches: list %d (0 or 1)", which);
    if (!c->tr_valid) return set_error(c, VX_ERR_STATE, "no vx_track_rig_async enqueued");
    int rc;
    if ((rc = check_cam(c, cam, "vx_track_rig_matches"))) return rc;
    const vx_ctx::RigCam& k = c->tr_cam[cam];
    if (k.cap[which] <= 0) return set_error(c, VX_ERR_STATE, "vx_track_rig_async enqueued no match %d for camera %d", which, cam);
    if (d_matches) *d_matches = k.list[which];
    if (d_n) *d_n = k.count[which];
    if (cap) *cap = k.cap[which];
    return VX_OK;
}

int vx_track_rig_block(vx_ctx* c, const uint8_t** block, int64_t* bytes, int32_t* cap_pairs0, int32_t* cap_pairs1,
                       int32_t* cap_kp, int cap_cams) {
    if (!c) return VX_ERR_INVALID;
    if (!c->tr_valid || !c->tr_fetched) return set_error(c, VX_ERR_STATE, "no vx_track_rig_fetch before vx_track_rig_block");
    if ((cap_pairs0 || cap_pairs1 || cap_kp) && cap_cams < c->tr_n)
        return set_error(c, VX_ERR_CAPACITY, "need %d capacities, cap %d", c->tr_n, cap_cams);
    if (block) *block = static_cast<const uint8_t*>(c->tr_host.p);
    if (bytes) *bytes = c->tr_bytes;
    for (int i = 0; i < c->tr_n; ++i) {
        if (cap_pairs0) cap_pairs0[i] = c->tr_cam[i].blk.cap0;
        if (cap_pairs1) cap_pairs1[i] = c->tr_cam[i].blk.cap1;
        if (cap_kp) cap_kp[i] = c->tr_cam[i].blk.cap_kp;
    }
    return VX_OK;
}

}  // extern "C"
