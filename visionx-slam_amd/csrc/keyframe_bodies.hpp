// keyframe_bodies.hpp — the program text of Tracking::CreateKeyFrame on the device-resident map, shared
// by the single call (keyframe.hip: k_kf_feat / k_kf_match / k_kf_commit) and the rig call
// (keyframe_rig.hip: k_rig_kf_feat / k_rig_kf_match / k_rig_kf_count / k_rig_kf_commit).
//
// A body reads its arguments as (KfArgs, a base): everything a camera's call fixes on the host, and
// the five places its new rows follow.  The single call's kernels pass the record's own counts (OwnBase); the
// rig kernels pass the same record read from a table entry and a RigBase advanced by the counts of the
// cameras before it.  The host side shares the array growth, the record's filler, the argument checks and the host
// mirrors' update (commit_mirrors), which both forms run per camera in camera order.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

#include "vx_internal.hpp"
#include "dmap.hpp"
#include "lm_math.hpp"

namespace vx {
namespace kf {

using namespace vx::lm;

constexpr int kThreads = 256;
constexpr int kBlock = 1024;
constexpr int kWaves = kBlock / 64;

struct KfArgs {
    // the new keyframe
    uint64_t kf_id, last_kf_id, first_id;
    const uint8_t* xy;       // position rows: two floats (or doubles, xy_f64) at xy + i * stride
    int64_t stride;
    int xy_f64;
    const int* n_feat;
    int cap_feat;
    int has_depth;
    DepthView dv;            // depth image + the new keyframe's intrinsics and T_cw
    // the last keyframe (rows of the map)
    int has_last, k_last, nf_last;
    int64_t f0_last;
    const vx_match* m;
    const int* n_matches;
    int cap_matches;
    double min_angle_rad, max_err;
    // the map: arrays and the used counts the new rows follow
    double *kf_pose, *kf_intr, *feat_uv;
    uint64_t* feat_lm;
    uint8_t* feat_fl;
    uint64_t* lm_id;
    double* lm_pos;
    uint8_t* lm_bad;
    int* obs_lm;
    uint64_t *obs_kf, *obs_fi;
    int64_t *obs_id, *id_row;
    int k_new;
    int64_t f0, n_lm0, n_obs0, n_ids0;
    double pose[7], intr[4];
    // scratch
    int* dvalid;             // per feature: CreateLandmarksFromDepth made a landmark
    double* dpw;
    int* tvalid;             // per match: passed the triangulation gate
    double* tpw;
    int *winner, *qseen, *err;
    // host-pinned outputs
    vx_keyframe_result* hdr;
    vx_keyframe_landmark* rec;
};

// Where a camera's new rows begin.  OwnBase: the record's own used counts (the single call; every
// accessor is a read of the kernel argument, so the single kernels' code is what it was before the
// bodies moved here).  RigBase: the rig call's, advanced by the cameras before this one.
struct OwnBase {
    const KfArgs& a;
    __device__ __forceinline__ int64_t f0() const { return a.f0; }
    __device__ __forceinline__ int64_t n_lm0() const { return a.n_lm0; }
    __device__ __forceinline__ int64_t n_obs0() const { return a.n_obs0; }
    __device__ __forceinline__ int64_t n_ids0() const { return a.n_ids0; }
    __device__ __forceinline__ uint64_t first_id() const { return a.first_id; }
    __device__ __forceinline__ vx_keyframe_landmark* rec() const { return a.rec; }
};
struct RigBase {
    int64_t f0_, n_lm0_, n_obs0_, n_ids0_;
    uint64_t first_id_;
    vx_keyframe_landmark* rec_;
    __device__ __forceinline__ int64_t f0() const { return f0_; }
    __device__ __forceinline__ int64_t n_lm0() const { return n_lm0_; }
    __device__ __forceinline__ int64_t n_obs0() const { return n_obs0_; }
    __device__ __forceinline__ int64_t n_ids0() const { return n_ids0_; }
    __device__ __forceinline__ uint64_t first_id() const { return first_id_; }
    __device__ __forceinline__ vx_keyframe_landmark* rec() const { return rec_; }
};
__device__ __forceinline__ RigBase rig_base_of(const KfArgs& a) {
    return RigBase{a.f0, a.n_lm0, a.n_obs0, a.n_ids0, a.first_id, a.rec};
}

__device__ __forceinline__ int clampi(int v, int hi) { return min(max(v, 0), hi); }

// feature i of the new keyframe: its row at the map's feature end and the depth branch
template <class B>
__device__ __forceinline__ void feat_body(const KfArgs& a, const B& b, int i) {
    const int n = clampi(*a.n_feat, a.cap_feat);
    if (i >= n) return;
    const uint8_t* p = a.xy + (int64_t)i * a.stride;
    double x, y;
    if (a.xy_f64) {
        x = reinterpret_cast<const double*>(p)[0];
        y = reinterpret_cast<const double*>(p)[1];
    } else {  // Feature::position from cv::KeyPoint::pt: float -> double, exact
        x = (double)reinterpret_cast<const float*>(p)[0];
        y = (double)reinterpret_cast<const float*>(p)[1];
    }
    const int64_t g = b.f0() + i;
    a.feat_uv[2 * g] = x;
    a.feat_uv[2 * g + 1] = y;
    a.feat_lm[g] = 0;  // the frame arrives without links (tracking.cpp:577)
    a.feat_fl[g] = 0;
    a.winner[i] = INT_MAX;
    int ok = 0;
    if (a.has_depth) {
        D3 pw;
        if (depth_point(a.dv, x, y, pw)) {
            a.dpw[3 * i] = pw.x;
            a.dpw[3 * i + 1] = pw.y;
            a.dpw[3 * i + 2] = pw.z;
            ok = 1;
        }
    }
    a.dvalid[i] = ok;
}

// match k: the error tests, the has_landmark tests and the triangulation gate
template <class B>
__device__ __forceinline__ void match_body(const KfArgs& a, const B& b, int k) {
    const int n = clampi(*a.n_matches, a.cap_matches);
    if (k >= n) return;
    a.tvalid[k] = 0;
    const int n2 = clampi(*a.n_feat, a.cap_feat);
    const vx_match mt = a.m[k];
    const int qi = mt.query_idx, ti = mt.train_idx;
    if (qi < 0 || qi >= a.nf_last || ti < 0 || ti >= n2) {
        atomicOr(a.err, VX_KF_ERR_MATCH_RANGE);
        return;
    }
    if (atomicAdd(&a.qseen[qi], 1) != 0) atomicOr(a.err, VX_KF_ERR_DUP_QUERY);
    const int64_t g1 = a.f0_last + qi, g2 = b.f0() + ti;
    // has_landmark of the last keyframe's feature; of the new one: only the depth loop set any
    if ((a.feat_fl[g1] & 1) || a.dvalid[ti]) return;
    const double x1 = a.feat_uv[2 * g1], y1 = a.feat_uv[2 * g1 + 1];
    const double x2 = a.feat_uv[2 * g2], y2 = a.feat_uv[2 * g2 + 1];
    Pose T1;
    double c1[4];
    for (int j = 0; j < 4; ++j) T1.q[j] = a.kf_pose[7 * (int64_t)a.k_last + j];
    for (int j = 0; j < 3; ++j) T1.t[j] = a.kf_pose[7 * (int64_t)a.k_last + 4 + j];
    for (int j = 0; j < 4; ++j) c1[j] = a.kf_intr[4 * (int64_t)a.k_last + j];
    D3 pw;
    if (!tri_gate(x1, y1, x2, y2, c1, a.intr, T1, a.dv.T, a.min_angle_rad, a.max_err, pw)) return;
    a.tvalid[k] = 1;
    a.tpw[3 * k] = pw.x;
    a.tpw[3 * k + 1] = pw.y;
    a.tpw[3 * k + 2] = pw.z;
    atomicMin(&a.winner[ti], k);
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

template <class B>
__device__ __forceinline__ void put_obs(const KfArgs& a, const B& b, int64_t j, int row, uint64_t kf, uint64_t fi) {
    const int64_t o = b.n_obs0() + j, id = b.n_ids0() + j;
    a.obs_lm[o] = row;
    a.obs_kf[o] = kf;
    a.obs_fi[o] = fi;
    a.obs_id[o] = id;
    a.id_row[id] = o;
}

template <class B>
__device__ __forceinline__ void put_landmark(const KfArgs& a, const B& b, int j, int kind, int feat_curr,
                                             int feat_last, const double* pw) {
    const int64_t row = b.n_lm0() + j;
    const uint64_t id = b.first_id() + (uint64_t)j;
    a.lm_id[row] = id;
    a.lm_pos[3 * row] = pw[0];
    a.lm_pos[3 * row + 1] = pw[1];
    a.lm_pos[3 * row + 2] = pw[2];
    a.lm_bad[row] = 0;
    a.feat_lm[b.f0() + feat_curr] = id;
    a.feat_fl[b.f0() + feat_curr] = 1;  // has_landmark, not outlier
    vx_keyframe_landmark r;
    r.lm_id = id;
    r.row = (int)row;
    r.kind = kind;
    r.feat_curr = feat_curr;
    r.feat_last = feat_last;
    r.pw[0] = pw[0];
    r.pw[1] = pw[1];
    r.pw[2] = pw[2];
    b.rec()[j] = r;
}

// the two compactions' membership tests, shared by the commit and the rig's count
__device__ __forceinline__ bool depth_made(const KfArgs& a, int i, int nf) { return i < nf && a.dvalid[i] != 0; }
__device__ __forceinline__ bool tri_made(const KfArgs& a, int k, int nm, vx_match& mt) {
    bool made = false;
    if (k < nm && a.tvalid[k]) {  // (tvalid: both indices are in range)
        mt = a.m[k];
        made = a.winner[mt.train_idx] == k;
    }
    return made;
}

// The commit workgroup's text is keyframe_commit_body.inc: included, not called, because as a function
// the single call's kernel needed 14 more SGPRs than before and spilled 34 of them.

// the totals of the commit's two compactions and nothing else (every thread returns them)
__device__ __forceinline__ void count_body(const KfArgs& a, int* s_cnt, int* n_depth, int* n_tri) {
    const int tid = threadIdx.x;
    const int nf = clampi(*a.n_feat, a.cap_feat);
    const int nm = a.has_last ? clampi(*a.n_matches, a.cap_matches) : 0;
    int nd = 0, nt = 0, total;
    for (int base = 0; base < nf; base += kBlock) {
        (void)block_rank(depth_made(a, base + tid, nf), s_cnt, &total);
        nd += total;
    }
    for (int base = 0; base < nm; base += kBlock) {
        vx_match mt{};
        (void)block_rank(tri_made(a, base + tid, nm, mt), s_cnt, &total);
        nt += total;
    }
    *n_depth = nd;
    *n_tri = nt;
}

// ---------------------------------------------------------------- host side

// room for `want` bytes keeping the first `used` (doubling, as the map's edit calls grow); the copy
// runs on the map context's stream, and no stream may still use the old block when it is freed
inline int grow(vx_ctx* c, vx_dmap* m, DevBuf& d, size_t used, size_t want) {
    if (want <= d.bytes) return VX_OK;
    size_t cap = std::max<size_t>(d.bytes * 2, 4096);
    while (cap < want) cap *= 2;
    void* np = nullptr;
    VX_HIP(c, hipMalloc(&np, cap));
    hipError_t e = hipSuccess;
    if (used) e = hipMemcpyAsync(np, d.p, used, hipMemcpyDeviceToDevice, m->c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(m->c->stream);
    if (e == hipSuccess && c != m->c) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        (void)hipFree(np);
        return hip_fail(c, e, "growing a map array");
    }
    d.release();
    d.p = np;
    d.bytes = cap;
    return VX_OK;
}

// the map's arrays for n_kf more keyframes of cf features in all — the worst case: every feature
// linked, every link a triangulated landmark's (two observations)
inline int grow_map(vx_ctx* c, vx_dmap* m, int n_kf, size_t cf) {
    const size_t k = m->kf_id.size(), f0 = (size_t)m->kf_feat_ptr.back(), nl = (size_t)m->n_lm, no = (size_t)m->n_obs,
                 ni = (size_t)m->n_ids;
    int rc;
    if ((rc = grow(c, m, m->kf_pose, k * 56, (k + n_kf) * 56))) return rc;
    if ((rc = grow(c, m, m->kf_intr, k * 32, (k + n_kf) * 32))) return rc;
    if ((rc = grow(c, m, m->feat_uv, f0 * 16, (f0 + cf) * 16))) return rc;
    if ((rc = grow(c, m, m->feat_lm, f0 * 8, (f0 + cf) * 8))) return rc;
    if ((rc = grow(c, m, m->feat_fl, f0, f0 + cf))) return rc;
    if ((rc = grow(c, m, m->lm_id, nl * 8, (nl + cf) * 8))) return rc;
    if ((rc = grow(c, m, m->lm_pos, nl * 24, (nl + cf) * 24))) return rc;
    if ((rc = grow(c, m, m->lm_bad, nl, nl + cf))) return rc;
    if ((rc = grow(c, m, m->obs_lm, no * 4, (no + 2 * cf) * 4))) return rc;
    if ((rc = grow(c, m, m->obs_kf, no * 8, (no + 2 * cf) * 8))) return rc;
    if ((rc = grow(c, m, m->obs_fi, no * 8, (no + 2 * cf) * 8))) return rc;
    if ((rc = grow(c, m, m->obs_id, no * 8, (no + 2 * cf) * 8))) return rc;
    if ((rc = grow(c, m, m->id_row, ni * 8, (ni + 2 * cf) * 8))) return rc;
    return VX_OK;
}

// the map's array pointers of an argument record (after grow_map)
inline void map_pointers(KfArgs& a, const vx_dmap* m) {
    a.kf_pose = m->kf_pose.as<double>();
    a.kf_intr = m->kf_intr.as<double>();
    a.feat_uv = m->feat_uv.as<double>();
    a.feat_lm = m->feat_lm.as<uint64_t>();
    a.feat_fl = m->feat_fl.as<uint8_t>();
    a.lm_id = m->lm_id.as<uint64_t>();
    a.lm_pos = m->lm_pos.as<double>();
    a.lm_bad = m->lm_bad.as<uint8_t>();
    a.obs_lm = m->obs_lm.as<int>();
    a.obs_kf = m->obs_kf.as<uint64_t>();
    a.obs_fi = m->obs_fi.as<uint64_t>();
    a.obs_id = m->obs_id.as<int64_t>();
    a.id_row = m->id_row.as<int64_t>();
}

// the new keyframe's camera, pose and options of an argument record
inline void camera_args(KfArgs& a, const double* pose7, const double* intr4, const vx_keyframe_options* opt) {
    a.dv.fx = intr4[0];
    a.dv.fy = intr4[1];
    a.dv.cx = intr4[2];
    a.dv.cy = intr4[3];
    for (int j = 0; j < 4; ++j) a.dv.T.q[j] = pose7[j];
    for (int j = 0; j < 3; ++j) a.dv.T.t[j] = pose7[4 + j];
    a.min_angle_rad = opt->tri_min_angle_deg * M_PI / 180.0;  // tracking.cpp:870-871
    a.max_err = opt->tri_max_reproj_error;
    for (int j = 0; j < 7; ++j) a.pose[j] = pose7[j];
    for (int j = 0; j < 4; ++j) a.intr[j] = intr4[j];
}

// one camera's inputs on the device: feature rows, match list, depth image
struct Input {
    const uint8_t* xy;
    int64_t stride;
    int xy_f64;
    const int32_t* n_feat;
    int cap_feat;
    const vx_match* matches;
    const int32_t* n_matches;
    int cap_matches;
    const void* depth;
    int depth_type, rows, cols;
    int64_t row_stride;
    bool has_depth() const { return depth && rows > 0 && cols > 0; }  // Depth().empty() (tracking.cpp:591-594)
};

// Everything of a camera's record that the single call and the rig call set alike: ids, feature rows, depth
// view, camera, the last keyframe (row k_last), the match list, the map's arrays (after grow_map) and the
// CALL's bases.  The caller adds k_new, its scratch and its pinned outputs.
inline void fill_args(KfArgs& a, const vx_dmap* m, const Input& in, uint64_t kf_id, const double* pose7, const double* intr4,
                      bool has_last, uint64_t last_kf_id, int k_last, uint64_t first_id, const vx_keyframe_options* opt) {
    a.kf_id = kf_id;
    a.last_kf_id = last_kf_id;
    a.first_id = first_id;
    a.xy = in.xy;
    a.stride = in.stride;
    a.xy_f64 = in.xy_f64;
    a.n_feat = in.n_feat;
    a.cap_feat = in.cap_feat;
    a.has_depth = in.has_depth() ? 1 : 0;
    a.dv.depth = static_cast<const uint8_t*>(in.depth);
    a.dv.type = in.depth_type;
    a.dv.rows = in.rows;
    a.dv.cols = in.cols;
    a.dv.stride = in.row_stride;
    camera_args(a, pose7, intr4, opt);
    a.has_last = has_last ? 1 : 0;
    a.k_last = k_last;
    a.f0_last = has_last ? m->kf_feat_ptr[k_last] : 0;
    a.nf_last = has_last ? (int)(m->kf_feat_ptr[k_last + 1] - a.f0_last) : 0;
    a.m = in.matches;
    a.n_matches = in.n_matches;
    a.cap_matches = has_last ? in.cap_matches : 0;
    map_pointers(a, m);
    a.f0 = m->kf_feat_ptr.back();
    a.n_lm0 = m->n_lm;
    a.n_obs0 = m->n_obs;
    a.n_ids0 = m->n_ids;
}

inline int depth_elem(int type) { return type == VX_DEPTH_U16 ? 2 : (type == VX_DEPTH_F32 ? 4 : 8); }

// bytes of a rows x cols image whose last row carries no padding
inline size_t depth_bytes(int type, int rows, int cols, int64_t row_stride) {
    return (size_t)row_stride * (rows - 1) + (size_t)cols * depth_elem(type);
}

inline int check_depth(vx_ctx* c, int depth_type, int cols, int64_t row_stride) {
    if (depth_type < VX_DEPTH_U16 || depth_type > VX_DEPTH_F64)
        return set_error(c, VX_ERR_INVALID, "unknown depth type %d", depth_type);
    if (row_stride < (int64_t)cols * depth_elem(depth_type))
        return set_error(c, VX_ERR_INVALID, "row_stride < cols * element size");
    return VX_OK;
}

inline int check_common(vx_ctx* c, const vx_dmap* m, const vx_keyframe_options* opt, const char* who) {
    if (!m || !m->c || !opt) return set_error(c, VX_ERR_INVALID, "%s: null argument", who);
    if (m->c->device != c->device) return set_error(c, VX_ERR_INVALID, "map and context on different devices");
    if (!(opt->tri_min_angle_deg == opt->tri_min_angle_deg) || !(opt->tri_max_reproj_error == opt->tri_max_reproj_error))
        return set_error(c, VX_ERR_INVALID, "%s: NaN option", who);
    return VX_OK;
}

// a committed header's counts against the camera's capacity
inline int check_counts(vx_ctx* c, const vx_keyframe_result& r, int cap_feat) {
    const int nf = r.n_feat, nd = r.n_depth, nt = r.n_triangulated;
    if (nf < 0 || nf > cap_feat || nd < 0 || nt < 0 || nd + nt > nf)
        return set_error(c, VX_ERR_STATE, "keyframe creation: %d depth + %d triangulated landmarks for %d features", nd,
                         nt, nf);
    return VX_OK;
}

// The host mirrors of one committed keyframe, as vx_dmap_add_landmarks / add_observations /
// set_features / add_keyframe leave them: rec = its n_depth + n_triangulated records, k_last the
// row of its last keyframe (read only by triangulated records).  A rig runs it per camera in camera order.
inline void commit_mirrors(vx_dmap* m, const vx_keyframe_landmark* rec, const vx_keyframe_result& res, uint64_t kf_id,
                           uint64_t last_kf_id, int k_last) {
    const int nf = res.n_feat, nd = res.n_depth, nt = res.n_triangulated, n_new = nd + nt;
    const int64_t k = (int64_t)m->kf_id.size(), f0 = m->kf_feat_ptr.back(), f0_last = m->kf_feat_ptr[k_last];
    m->lm_obs_live.resize(m->n_lm + n_new, 0);
    m->lm_removed.resize(m->n_lm + n_new, 0);
    m->feat_flags.resize((size_t)f0 + nf, 0);
    int64_t oid = m->n_ids;
    for (int i = 0; i < n_new; ++i) {
        const vx_keyframe_landmark& r = rec[i];
        m->lm_index[r.lm_id] = r.row;
        if (r.kind == 1) {
            m->obs_index.emplace(std::make_pair((int)r.row, last_kf_id), oid++);
            const int64_t g = f0_last + r.feat_last;
            m->kf_valid_cnt[k_last] += 1 - (m->feat_flags[g] & 1);
            m->feat_flags[g] = 1;
        }
        m->obs_index.emplace(std::make_pair((int)r.row, kf_id), oid++);
        m->lm_obs_live[r.row] = r.kind == 1 ? 2 : 1;
        m->feat_flags[f0 + r.feat_curr] = 1;
    }
    const int64_t n_obs_new = (int64_t)nd + 2 * (int64_t)nt;
    m->n_lm += n_new;
    m->n_lm_live += n_new;
    m->n_obs += n_obs_new;
    m->n_ids += n_obs_new;
    m->n_obs_live += n_obs_new;
    if (n_new) m->csr_dirty = true;
    m->kf_index[kf_id] = (int)k;
    m->kf_id.push_back(kf_id);
    m->kf_feat_ptr.push_back(f0 + nf);
    m->kf_has_cam.push_back(1);
    m->kf_alive.push_back(1);
    ++m->n_kf_live;
    m->kf_valid_cnt.push_back(n_new);
}

}  // namespace kf
}  // namespace vx
