// keyframe.hip — Tracking::CreateKeyFrame (core/frontend/tracking.cpp:577-584) on the device-resident
// map: vx_dmap_create_keyframe / vx_dmap_create_keyframe_host.
//
// The reference runs CreateLandmarksFromDepth(curr) (:586-650), TriangulateWithLastKeyFrame(last,
// curr) (:856-945) and Map::InsertKeyFrame(curr) (:581) one after the other, each loop marking
// features as it goes.  Everything those loops read is resident — the new frame's keypoints (an
// extraction slot), the match list (match.hip), the last keyframe's features, pose and intrinsics
// (vx_dmap rows) — and everything they change is a row of the map, so the sequence is
//
//   k_kf_feat (per feature)  ->  k_kf_match (per match)  ->  k_kf_commit (1 workgroup)
//
// with no host step between and one synchronisation after it.
//
//   k_kf_feat    widens feature i's position to double, stores it (with an empty link) at the map's
//                feature end, and evaluates the depth branch: flag + point per feature.
//   k_kf_match   match k: index bounds and the repeated-query test into the error word; the
//                has_landmark tests (the last keyframe's feat_fl row; the depth flag of the train
//                feature, i.e. the sequential outcome of the depth loop having run first); the
//                triangulation gate of lm_math.hpp with the last keyframe's pose and intrinsics read
//                from their map rows; a passing match enters atomicMin(winner[train], k).
//   k_kf_commit  validate-then-commit: reads the error word first and, when it is set, writes the
//                header and nothing else.  Otherwise two ORDERED compactions — the features with a
//                depth point, then the matches that passed and won their train feature — give every
//                created landmark its rank: per chunk of kBlock items a wave64 ballot + mbcnt ranks
//                inside the wave, the wave totals are summed in LDS, a running base carries over.
//                No atomic decides a position, so ids, rows and observation order are the sequential
//                loop's.  Rank r writes landmark row n_lm + r, its observation rows (one for depth,
//                two for a triangulated landmark: last keyframe first, :916-917), their ids and
//                id_row entries, the feature links of both keyframes and its record; thread 0 writes
//                the keyframe's pose / intrinsics rows and the header.  Records and header go to a
//                host-pinned block with plain stores: the end of the kernel releases them and the
//                one stream synchronisation makes them the host's.
//
// The commit is ONE workgroup for the reason k_track_pairs is: both compactions are ordered over at
// most a few thousand items, and a second workgroup would need a second launch or a grid barrier to
// see the first one's totals.  LDS: 16 wave counts.
//
// Every row the kernels write lies beyond the map's used counts (scratch until the host mirrors
// advance them) except the last keyframe's feature links and nothing at all on a rejected call, so a
// rejected call leaves the map as it was.  The arrays are grown for the worst case before the
// launches (cap_feat landmarks, 2 cap_feat observations: a feature is linked at most once), so the
// device sequence needs no count from the host.
//
// The kernels' program text lives in keyframe_bodies.hpp, shared with the rig form (keyframe_rig.hip), as do the
// record's filler (kf::fill_args over kf::Input) and the depth checks; the staging is m->create.in (vx::StagedUpload).
#include "keyframe_bodies.hpp"

namespace vx {
namespace {

using namespace vx::kf;

__global__ __launch_bounds__(kThreads) void k_kf_feat(KfArgs a) {
    feat_body(a, OwnBase{a}, blockIdx.x * kThreads + threadIdx.x);
}

__global__ __launch_bounds__(kThreads) void k_kf_match(KfArgs a) {
    match_body(a, OwnBase{a}, blockIdx.x * kThreads + threadIdx.x);
}

__global__ void __launch_bounds__(kBlock) k_kf_commit(KfArgs a) {
    __shared__ int s_cnt[kWaves];
    const OwnBase b{a};
#define KF_REJECTED(err) ((err) != 0)
#include "keyframe_commit_body.inc"
#undef KF_REJECTED
}

constexpr size_t kRecOff = 64;  // pinned block: vx_keyframe_result | records

int reject(vx_ctx* c, vx_keyframe_result* res, int bits, const char* what) {
    res->error_bits = bits;
    return set_error(c, VX_ERR_INVALID, "vx_dmap_create_keyframe: %s", what);
}

// the sequence over inputs already on the device, its one synchronisation, then the host mirrors
int create_run(vx_ctx* c, vx_dmap* m, uint64_t kf_id, const double* pose7, const double* intr4, const Input& in,
               int has_last, uint64_t last_kf_id, uint64_t first_id, const vx_keyframe_options* opt,
               vx_keyframe_result* res) {
    auto& K = m->create;
    K.rec.clear();
    std::memset(res, 0, sizeof *res);
    res->first_landmark_id = res->next_landmark_id = first_id;
    const int cap_feat = in.cap_feat, cap_m = has_last ? in.cap_matches : 0;
    // what the edit calls refuse, before anything is enqueued
    int bits = 0, k_last = 0;
    if (m->kf_index.count(kf_id)) bits |= VX_KF_ERR_KF_LIVE;
    if (!intr4) bits |= VX_KF_ERR_NO_CAMERA;
    if (has_last) {
        const auto it = m->kf_index.find(last_kf_id);
        if (it == m->kf_index.end()) bits |= VX_KF_ERR_NO_LAST;
        else if (!m->kf_has_cam[k_last = it->second]) bits |= VX_KF_ERR_NO_CAMERA;
    }
    for (int i = 0; i < cap_feat && !(bits & VX_KF_ERR_ID_RANGE); ++i)
        if (m->lm_index.count(first_id + (uint64_t)i)) bits |= VX_KF_ERR_ID_RANGE;
    if (bits & VX_KF_ERR_KF_LIVE) return reject(c, res, bits, "the keyframe is already in the map");
    if (bits & VX_KF_ERR_NO_LAST) return reject(c, res, bits, "the last keyframe is not in the map");
    if (bits & VX_KF_ERR_NO_CAMERA) return reject(c, res, bits, "a keyframe without a camera");
    if (bits) return reject(c, res, bits, "a landmark id of the range is already in the map");
    int rc;
    if (in.has_depth() && (rc = check_depth(c, in.depth_type, in.cols, in.row_stride))) return rc;
    VX_HIP(c, hipSetDevice(c->device));
    const int64_t f0 = m->kf_feat_ptr.back();
    const int nf_last = has_last ? (int)(m->kf_feat_ptr[k_last + 1] - m->kf_feat_ptr[k_last]) : 0;
    if (m->n_lm + cap_feat > (int64_t)INT_MAX || f0 + cap_feat > (int64_t)INT_MAX)
        return set_error(c, VX_ERR_CAPACITY, "the map's rows would pass 2^31");
    const size_t cf = (size_t)cap_feat;
    if ((rc = grow_map(c, m, 1, cf))) return rc;
    VX_HIP(c, K.dvalid.ensure(std::max<size_t>(cf, 1) * sizeof(int)));
    VX_HIP(c, K.dpw.ensure(std::max<size_t>(cf, 1) * 3 * sizeof(double)));
    VX_HIP(c, K.tvalid.ensure((size_t)std::max(cap_m, 1) * sizeof(int)));
    VX_HIP(c, K.tpw.ensure((size_t)std::max(cap_m, 1) * 3 * sizeof(double)));
    VX_HIP(c, K.aux.ensure((cf + (size_t)nf_last + 4) * sizeof(int)));
    VX_HIP(c, K.host.ensure(kRecOff + std::max<size_t>(cf, 1) * sizeof(vx_keyframe_landmark)));
    if (m->c != c && (rc = vx_stream_wait_ctx(c, m->c))) return rc;

    KfArgs a{};
    fill_args(a, m, in, kf_id, pose7, intr4, has_last != 0, last_kf_id, k_last, first_id, opt);
    a.k_new = (int)m->kf_id.size();
    a.dvalid = K.dvalid.as<int>();
    a.dpw = K.dpw.as<double>();
    a.tvalid = K.tvalid.as<int>();
    a.tpw = K.tpw.as<double>();
    a.winner = K.aux.as<int>();
    a.qseen = a.winner + cap_feat;
    a.err = a.qseen + nf_last;
    uint8_t* H = static_cast<uint8_t*>(K.host.p);
    a.hdr = reinterpret_cast<vx_keyframe_result*>(H);
    a.rec = reinterpret_cast<vx_keyframe_landmark*>(H + kRecOff);

    VX_HIP(c, hipMemsetAsync(a.qseen, 0, ((size_t)nf_last + 1) * sizeof(int), c->stream));
    VX_HIP(c, launch(c, kStKfFeat, k_kf_feat, dim3(std::max(1, (cap_feat + kThreads - 1) / kThreads)), dim3(kThreads),
                     0, c->stream, a));
    if (has_last)
        VX_HIP(c, launch(c, kStKfMatch, k_kf_match, dim3(std::max(1, (cap_m + kThreads - 1) / kThreads)),
                         dim3(kThreads), 0, c->stream, a));
    VX_HIP(c, launch(c, kStKfCommit, k_kf_commit, dim3(1), dim3(kBlock), 0, c->stream, a));
    VX_HIP(c, hipStreamSynchronize(c->stream));
    if (c->prof) prof_collect(c);

    std::memcpy(res, H, sizeof *res);
    if (res->error_bits) {
        if (res->error_bits & VX_KF_ERR_MATCH_RANGE) return set_error(c, VX_ERR_INVALID, "match index out of range");
        return set_error(c, VX_ERR_INVALID, "duplicate query index (matches must come from one knnMatch)");
    }
    if ((rc = check_counts(c, *res, cap_feat))) return rc;
    const int n_new = res->n_depth + res->n_triangulated;
    K.rec.resize(n_new);
    if (n_new) std::memcpy(K.rec.data(), H + kRecOff, (size_t)n_new * sizeof(vx_keyframe_landmark));
    commit_mirrors(m, K.rec.data(), *res, kf_id, last_kf_id, k_last);
    return VX_OK;
}

int check_common(vx_ctx* c, const vx_dmap* m, const double* pose7, const vx_keyframe_options* opt,
                 const vx_keyframe_result* res, const char* who) {
    if (!pose7 || !res) return set_error(c, VX_ERR_INVALID, "%s: null argument", who);
    return kf::check_common(c, m, opt, who);
}

}  // namespace
}  // namespace vx

using namespace vx;

extern "C" {

void vx_keyframe_default_options(vx_keyframe_options* o) {
    if (!o) return;
    o->tri_min_angle_deg = 1.0;      // Tracking::Options (tracking.h:43-44)
    o->tri_max_reproj_error = 5.0;
}

int vx_keyframe_block(void) { return kBlock; }

int vx_dmap_create_keyframe(vx_ctx* c, vx_dmap* m, uint64_t kf_id, const double* pose7, const double* intr4,
                            const float* d_xy, int64_t stride_bytes, const int32_t* d_n_feat, int cap_feat,
                            int has_last, uint64_t last_kf_id, const vx_match* d_matches,
                            const int32_t* d_n_matches, int cap_matches, const void* d_depth, int depth_type,
                            int rows, int cols, int64_t row_stride, uint64_t first_landmark_id,
                            const vx_keyframe_options* opt, vx_keyframe_result* result) {
    if (!c) return VX_ERR_INVALID;
    int rc;
    if ((rc = check_common(c, m, pose7, opt, result, "vx_dmap_create_keyframe"))) return rc;
    if (!d_n_feat || cap_feat < 0 || (cap_feat > 0 && !d_xy))
        return set_error(c, VX_ERR_INVALID, "vx_dmap_create_keyframe: feature rows without a count / capacity");
    if (stride_bytes < 8 || (stride_bytes & 3))
        return set_error(c, VX_ERR_INVALID, "position stride %lld: a multiple of 4, at least 8", (long long)stride_bytes);
    if (has_last) {
        if (d_matches) {
            if (!d_n_matches || cap_matches < 0)
                return set_error(c, VX_ERR_INVALID, "match list without a count / capacity");
        } else {
            if (!c->match_valid) return set_error(c, VX_ERR_STATE, "no match enqueued on this context");
            d_matches = c->matches.as<vx_match>();
            d_n_matches = c->match_count.as<int32_t>();
            cap_matches = c->match_cap;
        }
    }
    Input in{};
    in.xy = reinterpret_cast<const uint8_t*>(d_xy);
    in.stride = stride_bytes;
    in.xy_f64 = 0;
    in.n_feat = d_n_feat;
    in.cap_feat = cap_feat;
    in.matches = d_matches;
    in.n_matches = d_n_matches;
    in.cap_matches = cap_matches;
    in.depth = d_depth;
    in.depth_type = depth_type;
    in.rows = rows;
    in.cols = cols;
    in.row_stride = row_stride;
    return create_run(c, m, kf_id, pose7, intr4, in, has_last, last_kf_id, first_landmark_id, opt, result);
}

int vx_dmap_create_keyframe_host(vx_ctx* c, vx_dmap* m, uint64_t kf_id, const double* pose7, const double* intr4,
                                 const double* feat_uv, int n_feat, int has_last, uint64_t last_kf_id,
                                 const vx_match* matches, int n_matches, const void* depth, int depth_type, int rows,
                                 int cols, int64_t row_stride, uint64_t first_landmark_id,
                                 const vx_keyframe_options* opt, vx_keyframe_result* result) {
    if (!c) return VX_ERR_INVALID;
    int rc;
    if ((rc = check_common(c, m, pose7, opt, result, "vx_dmap_create_keyframe_host"))) return rc;
    if (n_feat < 0 || (n_feat > 0 && !feat_uv) || n_matches < 0 || (has_last && n_matches > 0 && !matches))
        return set_error(c, VX_ERR_INVALID, "vx_dmap_create_keyframe_host: bad feature / match arguments");
    const bool has_depth = depth && rows > 0 && cols > 0;
    if (has_depth && (rc = check_depth(c, depth_type, cols, row_stride))) return rc;
    VX_HIP(c, hipSetDevice(c->device));
    auto& K = m->create;
    // one staged block: {n_feat, n_matches} | positions | matches | depth image
    const int nm = has_last ? n_matches : 0;
    const size_t o_uv = 64, o_m = align64(o_uv + (size_t)n_feat * 16), o_d = align64(o_m + (size_t)nm * sizeof(vx_match)),
                 d_bytes = has_depth ? depth_bytes(depth_type, rows, cols, row_stride) : 0, bytes = align64(o_d + d_bytes);
    // (the one place this entry can block: until the previous call's upload has left the staging)
    VX_HIP(c, K.in.begin(bytes));
    uint8_t* h = static_cast<uint8_t*>(K.in.host.p);
    const int32_t counts[4] = {n_feat, nm, 0, 0};
    std::memcpy(h, counts, sizeof counts);
    if (n_feat) std::memcpy(h + o_uv, feat_uv, (size_t)n_feat * 16);
    if (nm) std::memcpy(h + o_m, matches, (size_t)nm * sizeof(vx_match));
    if (d_bytes) std::memcpy(h + o_d, depth, d_bytes);
    VX_HIP(c, K.in.upload(bytes, c->stream));
    const uint8_t* d = K.in.dev.as<uint8_t>();
    Input in{};
    in.xy = d + o_uv;
    in.stride = 16;
    in.xy_f64 = 1;
    in.n_feat = K.in.dev.as<int32_t>();
    in.cap_feat = n_feat;
    in.matches = reinterpret_cast<const vx_match*>(d + o_m);
    in.n_matches = K.in.dev.as<int32_t>() + 1;
    in.cap_matches = nm;
    in.depth = has_depth ? d + o_d : nullptr;
    in.depth_type = depth_type;
    in.rows = rows;
    in.cols = cols;
    in.row_stride = row_stride;
    return create_run(c, m, kf_id, pose7, intr4, in, has_last, last_kf_id, first_landmark_id, opt, result);
}

int vx_dmap_create_keyframe_frame(vx_ctx* c, vx_dmap* m, uint64_t kf_id, const double* pose7, const double* intr4,
                                  const vx_frame* curr, int has_last, uint64_t last_kf_id, const vx_match* d_matches,
                                  const int32_t* d_n_matches, int cap_matches, const void* depth, int depth_type, int rows,
                                  int cols, int64_t row_stride, uint64_t first_landmark_id,
                                  const vx_keyframe_options* opt, vx_keyframe_result* result) {
    if (!c) return VX_ERR_INVALID;
    int rc;
    if ((rc = check_common(c, m, pose7, opt, result, "vx_dmap_create_keyframe_frame"))) return rc;
    if (!curr || !curr->block.p || curr->device != c->device)
        return set_error(c, VX_ERR_INVALID, "vx_dmap_create_keyframe_frame: no frame, or a frame of another device");
    const bool has_depth = depth && rows > 0 && cols > 0;
    const void* d_depth = nullptr;
    if (has_depth) {
        if ((rc = check_depth(c, depth_type, cols, row_stride))) return rc;
        VX_HIP(c, hipSetDevice(c->device));
        // the depth image is the one thing that still comes from the host: one copy per keyframe,
        // through the staging vx_dmap_create_keyframe_host uses (and its event)
        auto& K = m->create;
        const size_t d_bytes = depth_bytes(depth_type, rows, cols, row_stride), bytes = align64(d_bytes);
        VX_HIP(c, K.in.begin(bytes));
        std::memcpy(K.in.host.p, depth, d_bytes);
        VX_HIP(c, K.in.upload(bytes, c->stream));
        d_depth = K.in.dev.p;
    }
    return vx_dmap_create_keyframe(c, m, kf_id, pose7, intr4, &curr->kp()->x, (int64_t)sizeof(vx_keypoint), curr->count(),
                                   curr->cap, has_last, last_kf_id, d_matches, d_n_matches, cap_matches, d_depth, depth_type,
                                   has_depth ? rows : 0, has_depth ? cols : 0, row_stride, first_landmark_id, opt, result);
}

int vx_dmap_create_results(vx_dmap* m, int cap, vx_keyframe_landmark* records, int* n) {
    if (!m) return VX_ERR_INVALID;
    const auto& R = m->create.rec;
    const int k = (int)R.size();
    if (n) *n = k;
    if (records && k > cap) return set_error(m->c, VX_ERR_CAPACITY, "need %d landmark records, cap %d", k, cap);
    if (records && k) std::memcpy(records, R.data(), (size_t)k * sizeof(vx_keyframe_landmark));
    return VX_OK;
}

int vx_dmap_keyframe_features(vx_dmap* m, uint64_t kf_id, int cap, double* uv, uint64_t* lm_id, uint8_t* flags,
                              int* n) {
    if (!m) return VX_ERR_INVALID;
    vx_ctx* c = m->c;
    const auto it = m->kf_index.find(kf_id);
    if (it == m->kf_index.end())
        return set_error(c, VX_ERR_INVALID, "keyframe %llu is not in the map", (unsigned long long)kf_id);
    const int64_t f0 = m->kf_feat_ptr[it->second];
    const int nf = (int)(m->kf_feat_ptr[it->second + 1] - f0);
    if (n) *n = nf;
    if ((uv || lm_id || flags) && nf > cap) return set_error(c, VX_ERR_CAPACITY, "need %d features, cap %d", nf, cap);
    if (!nf) return VX_OK;
    VX_HIP(c, hipSetDevice(c->device));
    VX_HIP(c, hipStreamSynchronize(c->stream));
    if (uv) VX_HIP(c, hipMemcpy(uv, m->feat_uv.as<double>() + 2 * f0, (size_t)nf * 16, hipMemcpyDeviceToHost));
    if (lm_id) VX_HIP(c, hipMemcpy(lm_id, m->feat_lm.as<uint64_t>() + f0, (size_t)nf * 8, hipMemcpyDeviceToHost));
    if (flags) VX_HIP(c, hipMemcpy(flags, m->feat_fl.as<uint8_t>() + f0, (size_t)nf, hipMemcpyDeviceToHost));
    return VX_OK;
}

}  // extern "C"

static_assert(sizeof(vx_keyframe_options) == 16, "vx_keyframe_options layout (python KEYFRAME_OPTIONS_DTYPE)");
static_assert(sizeof(vx_keyframe_result) == 40, "vx_keyframe_result layout (python KEYFRAME_RESULT_DTYPE)");
static_assert(sizeof(vx_keyframe_landmark) == 48, "vx_keyframe_landmark layout (python KEYFRAME_LANDMARK_DTYPE)");
