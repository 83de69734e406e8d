// keyframe_rig.hip — Tracking::CreateKeyFrame (core/frontend/tracking.cpp:577-584) for every camera
// of a rig time step that inserts a keyframe, over one shared map, as ONE stream-ordered sequence and
// ONE synchronisation (vx_dmap_create_keyframes_rig).
//
// vx_dmap_create_keyframe_frame (keyframe.hip) costs a memset, three launches, a depth upload, a
// synchronisation and a host-mirror pass per camera, all bound by launch and synchronisation latency.
// Here camera = grid row or workgroup of every kernel, so the sequence is one upload, one memset and
// four launches whatever the number of cameras:
//
//   k_rig_kf_feat    grid (chunks, cameras)   feat_body on the camera's table entry
//   k_rig_kf_match   grid (chunks, cameras)   match_body, with the camera's winner / qseen / err slices
//   k_rig_kf_count   grid = cameras           the commit's two ordered compactions' totals -> cnt[2 c]
//   k_rig_kf_commit  grid = cameras           every camera's error word, the exclusive prefix of cnt,
//                                             then commit_body
//
// The call gives what N vx_dmap_create_keyframe_frame calls in camera order give.  The only thing a
// camera needs from the ones before it is where its rows begin:
//
//   keyframe row     k + i                                          (host)
//   feature rows     f0 + sum_{j<i} n_feat_j                        (device counts, clamped)
//   landmark rows    n_lm + sum_{j<i} (n_depth_j + n_tri_j)         (k_rig_kf_count's table)
//   landmark ids     first_landmark_id + the same sum
//   observations     n_obs / n_ids + sum_{j<i} (n_depth_j + 2 n_tri_j)
//
// Every workgroup recomputes its camera's sums from at most 16 counts (k_rig_pack's idiom, track_rig.hip):
// no workgroup waits on another, no atomic decides a position, ranks come from block_rank.  The count
// is a launch of its own because the commit of camera i needs the totals of cameras j < i, which
// exist only once their compactions have run: inside one launch that would be a wait between workgroups.
//
// Apart from the bases the cameras are independent — the depth pass touches the new keyframe only,
// the triangulation pass reads and links the camera's own last keyframe only — as long as no two
// cameras name one last keyframe (both would link its features: the second call of a sequence would
// see the first one's links), no keyframe id is named twice, and every last keyframe is live BEFORE
// the call (a camera whose last keyframe is another camera's new one would read rows this call
// writes).  The call refuses all three (VX_KF_ERR_RIG_REPEAT, VX_KF_ERR_NO_LAST).
//
// All or nothing: k_rig_kf_commit reads every camera's error word first and, when any is set, every
// camera writes its header (with its own error bits) and nothing else; everything written before
// lies beyond the map's used counts, so a rejected call leaves the map as it was.
//
// The per-camera argument records (KfArgs, keyframe_bodies.hpp) and the cameras' HOST depth images are
// staged in one pinned block (the single call's staging, m->create.in, guarded by its event) and uploaded in one copy;
// the kernels read their entry through uniform addresses.  The kernels run the single call's program
// text and their records are filled by its filler, kf::fill_args (keyframe_bodies.hpp).  Resources (-Rpass-analysis=kernel-resource-usage, gfx950): DESIGN §34.
#include "keyframe_bodies.hpp"

namespace vx {
namespace {

using namespace vx::kf;

constexpr int kP = VX_MAX_RIG_CAMERAS;

// camera cam's feature rows begin after the clamped counts of the cameras before it
__device__ __forceinline__ int64_t feat_before(const KfArgs* __restrict__ tab, int cam) {
    int64_t s = 0;
    for (int j = 0; j < cam; ++j) s += clampi(*tab[j].n_feat, tab[j].cap_feat);
    return s;
}

__global__ __launch_bounds__(kThreads) void k_rig_kf_feat(const KfArgs* __restrict__ tab) {
    const int cam = blockIdx.y;
    const KfArgs& a = tab[cam];
    RigBase b = rig_base_of(a);
    b.f0_ += feat_before(tab, cam);
    feat_body(a, b, blockIdx.x * kThreads + threadIdx.x);
}

__global__ __launch_bounds__(kThreads) void k_rig_kf_match(const KfArgs* __restrict__ tab) {
    const int cam = blockIdx.y;
    const KfArgs& a = tab[cam];
    if (!a.has_last) return;  // (block-uniform) the single call does not launch k_kf_match
    RigBase b = rig_base_of(a);
    b.f0_ += feat_before(tab, cam);
    match_body(a, b, blockIdx.x * kThreads + threadIdx.x);
}

// cnt[2 cam] = n_depth, cnt[2 cam + 1] = n_triangulated of camera cam
__global__ void __launch_bounds__(kBlock) k_rig_kf_count(const KfArgs* __restrict__ tab, int* __restrict__ cnt) {
    __shared__ int s_cnt[kWaves];
    const int cam = blockIdx.x;
    int nd, nt;
    count_body(tab[cam], s_cnt, &nd, &nt);
    if (threadIdx.x == 0) {
        cnt[2 * cam] = nd;
        cnt[2 * cam + 1] = nt;
    }
}

__global__ void __launch_bounds__(kBlock) k_rig_kf_commit(const KfArgs* __restrict__ tab, int n_cams,
                                                          const int* __restrict__ cnt) {
    __shared__ int s_cnt[kWaves];
    const int cam = blockIdx.x;
    const KfArgs& a = tab[cam];
    int any = 0;
    for (int j = 0; j < n_cams; ++j) any |= *tab[j].err;
    RigBase b = rig_base_of(a);
    if (!any) {
        int64_t lm = 0, obs = 0;
        for (int j = 0; j < cam; ++j) {
            const int nd = cnt[2 * j], nt = cnt[2 * j + 1];
            lm += nd + nt;
            obs += (int64_t)nd + 2 * (int64_t)nt;
        }
        b.f0_ += feat_before(tab, cam);
        b.n_lm0_ += lm;
        b.first_id_ += (uint64_t)lm;
        b.rec_ += lm;
        b.n_obs0_ += obs;
        b.n_ids0_ += obs;
    }
#define KF_REJECTED(err) (any != 0)
#include "keyframe_commit_body.inc"
#undef KF_REJECTED
}

constexpr size_t kRigRecOff = 1024;  // pinned block: vx_keyframe_result[kP] | records
static_assert(kP * sizeof(vx_keyframe_result) <= kRigRecOff, "header block");

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace
}  // namespace vx

using namespace vx;

extern "C" {

int vx_dmap_create_keyframes_rig(vx_ctx* c, vx_dmap* m, int n_cams, const vx_rig_keyframe* cams,
                                 uint64_t first_landmark_id, const vx_keyframe_options* opt,
                                 vx_keyframe_result* results) {
    const char* who = "vx_dmap_create_keyframes_rig";
    if (!c) return VX_ERR_INVALID;
    if (n_cams < 1 || n_cams > kP) return set_error(c, VX_ERR_INVALID, "%s: %d cameras outside [1, %d]", who, n_cams, kP);
    if (!cams || !results) return set_error(c, VX_ERR_INVALID, "%s: null argument", who);
    int rc;
    if ((rc = kf::check_common(c, m, opt, who))) return rc;
    auto& K = m->create;
    K.rec.clear();
    for (int i = 0; i < n_cams; ++i) {
        std::memset(results + i, 0, sizeof *results);
        results[i].first_landmark_id = results[i].next_landmark_id = first_landmark_id;
    }
    // ---- argument errors, camera by camera (vx_dmap_create_keyframe_frame's)
    bool has_depth[kP];
    size_t d_bytes[kP];
    int64_t sum_feat = 0, sum_m = 0;
    for (int i = 0; i < n_cams; ++i) {
        const vx_rig_keyframe& k = cams[i];
        if (!k.pose7) return set_error(c, VX_ERR_INVALID, "%s: camera %d: null pose", who, i);
        if (!k.curr || !k.curr->block.p || k.curr->device != c->device)
            return set_error(c, VX_ERR_INVALID, "%s: camera %d: no frame, or a frame of another device", who, i);
        if (k.has_last && (!k.d_matches || !k.d_n_matches || k.cap_matches < 0))
            return set_error(c, VX_ERR_INVALID, "%s: camera %d: a last keyframe without a match list / count / capacity", who, i);
        has_depth[i] = k.depth && k.rows > 0 && k.cols > 0;
        d_bytes[i] = 0;
        if (has_depth[i]) {
            if ((rc = check_depth(c, k.depth_type, k.cols, k.row_stride))) return rc;
            d_bytes[i] = depth_bytes(k.depth_type, k.rows, k.cols, k.row_stride);
        }
        sum_feat += k.curr->cap;
        sum_m += k.has_last ? k.cap_matches : 0;
    }
    // ---- what the edit calls refuse, and what would break the cameras' independence: per-camera bits
    int k_last[kP] = {0};
    bool any_bits = false;
    bool id_hit = false;
    for (int64_t i = 0; i < sum_feat && !id_hit; ++i) id_hit = m->lm_index.count(first_landmark_id + (uint64_t)i) != 0;
    for (int i = 0; i < n_cams; ++i) {
        const vx_rig_keyframe& k = cams[i];
        int bits = id_hit ? VX_KF_ERR_ID_RANGE : 0;  // (the range is the call's: every camera carries it)
        if (m->kf_index.count(k.kf_id)) bits |= VX_KF_ERR_KF_LIVE;
        if (!k.intr4) bits |= VX_KF_ERR_NO_CAMERA;
        if (k.has_last) {
            const auto it = m->kf_index.find(k.last_kf_id);
            if (it == m->kf_index.end()) bits |= VX_KF_ERR_NO_LAST;  // (another camera's new keyframe included)
            else if (!m->kf_has_cam[k_last[i] = it->second]) bits |= VX_KF_ERR_NO_CAMERA;
        }
        for (int j = 0; j < n_cams; ++j) {
            if (j == i) continue;
            if (cams[j].kf_id == k.kf_id) bits |= VX_KF_ERR_RIG_REPEAT;
            if (k.has_last && cams[j].has_last && cams[j].last_kf_id == k.last_kf_id) bits |= VX_KF_ERR_RIG_REPEAT;
        }
        results[i].error_bits = bits;
        any_bits |= bits != 0;
    }
    if (any_bits) return set_error(c, VX_ERR_INVALID, "%s: refused before the launches (see each camera's error_bits)", who);

    VX_HIP(c, hipSetDevice(c->device));
    const int64_t k0 = (int64_t)m->kf_id.size(), f0 = m->kf_feat_ptr.back();
    if (m->n_lm + sum_feat > (int64_t)INT_MAX || f0 + sum_feat > (int64_t)INT_MAX || sum_m > (int64_t)INT_MAX)
        return set_error(c, VX_ERR_CAPACITY, "the map's rows would pass 2^31");
    // ---- capacity-strided slices, known on the host
    int64_t o_feat[kP + 1], o_match[kP + 1], o_last[kP + 1];
    int nf_last[kP];
    o_feat[0] = o_match[0] = o_last[0] = 0;
    int max_feat = 0, max_m = 0;
    for (int i = 0; i < n_cams; ++i) {
        const vx_rig_keyframe& k = cams[i];
        const int cm = k.has_last ? k.cap_matches : 0;
        nf_last[i] = k.has_last ? (int)(m->kf_feat_ptr[k_last[i] + 1] - m->kf_feat_ptr[k_last[i]]) : 0;
        o_feat[i + 1] = o_feat[i] + k.curr->cap;
        o_match[i + 1] = o_match[i] + cm;
        o_last[i + 1] = o_last[i] + nf_last[i];
        max_feat = std::max(max_feat, k.curr->cap);
        max_m = std::max(max_m, cm);
    }
    const size_t cf = (size_t)sum_feat, cmm = (size_t)sum_m, cl = (size_t)o_last[n_cams];
    // arrays grown once, for the sum of the capacities
    if ((rc = grow_map(c, m, n_cams, cf))) return rc;
    VX_HIP(c, K.dvalid.ensure(std::max<size_t>(cf, 1) * sizeof(int)));
    VX_HIP(c, K.dpw.ensure(std::max<size_t>(cf, 1) * 3 * sizeof(double)));
    VX_HIP(c, K.tvalid.ensure(std::max<size_t>(cmm, 1) * sizeof(int)));
    VX_HIP(c, K.tpw.ensure(std::max<size_t>(cmm, 1) * 3 * sizeof(double)));
    // aux: winner per feature | qseen per last-keyframe feature | error word per camera | count table
    VX_HIP(c, K.aux.ensure((cf + cl + 3 * (size_t)kP) * sizeof(int)));
    VX_HIP(c, K.host.ensure(kRigRecOff + std::max<size_t>(cf, 1) * sizeof(vx_keyframe_landmark)));
    if (m->c != c && (rc = vx_stream_wait_ctx(c, m->c))) return rc;

    // ---- ONE pinned block: the argument table | the depth images; ONE copy
    size_t o_depth[kP], bytes = align256((size_t)n_cams * sizeof(KfArgs));
    for (int i = 0; i < n_cams; ++i) {
        o_depth[i] = bytes;
        bytes += align64(d_bytes[i]);
    }
    // (the one place this entry can block: until the previous call's upload has left the staging)
    VX_HIP(c, K.in.begin(bytes));
    uint8_t* h = static_cast<uint8_t*>(K.in.host.p);
    const uint8_t* d = K.in.dev.as<uint8_t>();
    uint8_t* H = static_cast<uint8_t*>(K.host.p);
    int* winner = K.aux.as<int>();
    int* qseen = winner + cf;
    int* err = qseen + cl;
    int* cnt = err + kP;
    KfArgs* tab = reinterpret_cast<KfArgs*>(h);
    for (int i = 0; i < n_cams; ++i) {
        const vx_rig_keyframe& k = cams[i];
        Input in{};
        in.xy = reinterpret_cast<const uint8_t*>(&k.curr->kp()->x);
        in.stride = (int64_t)sizeof(vx_keypoint);
        in.n_feat = k.curr->count();
        in.cap_feat = k.curr->cap;
        in.matches = k.d_matches;
        in.n_matches = k.d_n_matches;
        in.cap_matches = k.cap_matches;
        in.depth = has_depth[i] ? d + o_depth[i] : nullptr;
        in.depth_type = k.depth_type;
        in.rows = has_depth[i] ? k.rows : 0;
        in.cols = has_depth[i] ? k.cols : 0;
        in.row_stride = k.row_stride;
        KfArgs a{};
        // (the bases it sets are the CALL's: the kernels advance them by the cameras before this one)
        fill_args(a, m, in, k.kf_id, k.pose7, k.intr4, k.has_last != 0, k.last_kf_id, k_last[i], first_landmark_id, opt);
        a.k_new = (int)(k0 + i);
        a.rec = reinterpret_cast<vx_keyframe_landmark*>(H + kRigRecOff);
        a.dvalid = K.dvalid.as<int>() + o_feat[i];
        a.dpw = K.dpw.as<double>() + 3 * o_feat[i];
        a.tvalid = K.tvalid.as<int>() + o_match[i];
        a.tpw = K.tpw.as<double>() + 3 * o_match[i];
        a.winner = winner + o_feat[i];
        a.qseen = qseen + o_last[i];
        a.err = err + i;
        a.hdr = reinterpret_cast<vx_keyframe_result*>(H) + i;
        std::memcpy(tab + i, &a, sizeof a);
        if (d_bytes[i]) std::memcpy(h + o_depth[i], k.depth, d_bytes[i]);
    }
    VX_HIP(c, K.in.upload(bytes, c->stream));
    const KfArgs* dtab = K.in.dev.as<KfArgs>();

    // ---- one memset (every camera's qseen slice and error word) and four launches
    VX_HIP(c, hipMemsetAsync(qseen, 0, (cl + (size_t)kP) * sizeof(int), c->stream));
    VX_HIP(c, launch(c, kStRigKfFeat, k_rig_kf_feat, dim3(std::max(1, (max_feat + kThreads - 1) / kThreads), n_cams),
                     dim3(kThreads), 0, c->stream, dtab));
    VX_HIP(c, launch(c, kStRigKfMatch, k_rig_kf_match, dim3(std::max(1, (max_m + kThreads - 1) / kThreads), n_cams),
                     dim3(kThreads), 0, c->stream, dtab));
    VX_HIP(c, launch(c, kStRigKfCount, k_rig_kf_count, dim3(n_cams), dim3(kBlock), 0, c->stream, dtab, cnt));
    VX_HIP(c, launch(c, kStRigKfCommit, k_rig_kf_commit, dim3(n_cams), dim3(kBlock), 0, c->stream, dtab, n_cams,
                     (const int*)cnt));
    VX_HIP(c, hipStreamSynchronize(c->stream));
    if (c->prof) prof_collect(c);

    std::memcpy(results, H, (size_t)n_cams * sizeof *results);
    int dev_bits = 0;
    for (int i = 0; i < n_cams; ++i) dev_bits |= results[i].error_bits;
    if (dev_bits) {
        if (dev_bits & VX_KF_ERR_MATCH_RANGE) return set_error(c, VX_ERR_INVALID, "%s: match index out of range", who);
        return set_error(c, VX_ERR_INVALID, "%s: duplicate query index (matches must come from one knnMatch)", who);
    }
    // all cameras' counts first, then the mirrors: nothing is half committed on the host either
    int64_t n_all = 0;
    for (int i = 0; i < n_cams; ++i) {
        if ((rc = check_counts(c, results[i], cams[i].curr->cap))) return rc;
        if (results[i].first_landmark_id != first_landmark_id + (uint64_t)n_all)
            return set_error(c, VX_ERR_STATE, "%s: camera %d's landmark ids do not continue camera %d's", who, i, i - 1);
        n_all += results[i].n_depth + results[i].n_triangulated;
    }
    K.rec.resize((size_t)n_all);
    if (n_all) std::memcpy(K.rec.data(), H + kRigRecOff, (size_t)n_all * sizeof(vx_keyframe_landmark));
    size_t at = 0;
    for (int i = 0; i < n_cams; ++i) {
        commit_mirrors(m, K.rec.data() + at, results[i], cams[i].kf_id, cams[i].last_kf_id, k_last[i]);
        at += (size_t)(results[i].n_depth + results[i].n_triangulated);
    }
    return VX_OK;
}

}  // extern "C"

static_assert(sizeof(vx_rig_keyframe) == 104, "vx_rig_keyframe layout (python RIG_KEYFRAME_DTYPE)");
