// track_bodies.hpp — the rules of Tracking::Track's kernels stated ONCE, as __device__ functions over
// the argument records the kernels take: the single-camera kernels (k_track_pairs, track.hip;
// k_track_epairs / k_track_epose, track_ess.hip; k_track_gate / k_track_final, track_frame.hip) hand
// them their kernel argument, the rig kernels (track_rig.hip) an entry of a device table — as
// trk::pnp_status (track_common.hpp) is shared between host and device.  The gate, the pose
// composition and the final block are __forceinline__ functions; the two pair kernels' stages are
// program text (track_pairs_body.inc, track_epairs_body.inc) included into both kernels, because as
// functions over an argument record they cost the single-camera kernels 2 VGPRs and a 28 - 44 KB LDS
// promotion of the record.  Either way the single-camera kernels compile to what they were
// (-Rpass-analysis=kernel-resource-usage figures unchanged: DESIGN.md §32).
// The host section at the end states once how the entry points fill and check these records;
// it is here, not in a header of its own, so that a record and its filler are read and changed together, as
// keyframe_bodies.hpp keeps map_pointers / camera_args / check_depth beside KfArgs.
#pragma once

#include <algorithm>
#include <cstring>
#include <type_traits>

#include "vx_internal.hpp"
#include "dmap.hpp"
#include "lm_hash.hpp"
#include "track_common.hpp"
#include "vx_rows.hpp"

namespace vx {
namespace trk {

// ------------------------------------------------------------------ TrackWithPnP's filter + pair gather
struct TrackArgs {
    // match list (query = last keyframe feature, train = current frame feature)
    const vx_match* matches;
    const int* n_matches;
    int cap_matches;
    // current frame positions: two floats at curr_xy + i * stride
    const uint8_t* curr_xy;
    int64_t stride;
    const int* n_curr;
    // last keyframe: resident feature rows [f0, f0 + nf)
    int64_t f0;
    int nf;
    const double* feat_uv;
    const uint64_t* feat_lm;
    const uint8_t* feat_fl;
    // landmarks
    const uint64_t* ht_key;
    const int* ht_val;
    unsigned ht_mask;
    const uint8_t* lm_bad;
    const double* lm_pos;
    // options
    int min_matches, min_inliers;
    vx_pnp_options pnp;
    double intr[4];
    // scratch + outputs
    int* good;              // cap_matches: kept match indices, match order
    float* obj;             // 3 per pair
    float* img;             // 2 per pair
    int* pair_match;        // per pair
    uint8_t* mask;          // per pair (zeroed here, written by k_pnp_refine)
    vx_track_result* res;
    int* offsets;           // 2
    double* intr_out;       // 4
    vx_pnp_options* opt_out;
};

__device__ __forceinline__ void curr_pos(const TrackArgs& a, int i, float* x, float* y) {
    const float* p = reinterpret_cast<const float*>(a.curr_xy + (int64_t)i * a.stride);
    *x = p[0];
    *y = p[1];
}

// ------------------------------------------------------------------ TrackLastFrame's filter + 2D-2D pair gather
struct EPairArgs {
    // match list (query = last frame feature, train = current frame feature)
    const vx_match* matches;
    const int* n_matches;
    int cap_matches;
    // positions: two floats at *_xy + i * stride, *n_* rows
    const uint8_t* last_xy;
    int64_t last_stride;
    const int* n_last;
    const uint8_t* curr_xy;
    int64_t curr_stride;
    const int* n_curr;
    // options
    int min_matches;
    vx_essential_options ess;
    double intr[4];
    // scratch + outputs
    int* good;              // cap_matches: kept match indices, match order
    float* p1;              // 2 per pair (pts_last)
    float* p2;              // 2 per pair (pts_curr)
    int* pair_match;        // per pair
    uint8_t* mask;          // per pair (zeroed here, written by k_em_cheir / k_em_final)
    vx_track_essential_result* res;
    int* offsets;           // 2
    double* intr_out;       // 4
    vx_essential_options* opt_out;
};

// ------------------------------------------------------------------ T_cl * T_lw
struct EPoseArgs {
    vx_track_essential_result* res;
    double pose_last[7];  // T_lw: qx qy qz qw tx ty tz
};

// Sophus::SE3d(R, t) * T_lw by the calling lane (tracking.cpp:539-541); zero when recoverPose gave nothing
__device__ __forceinline__ void track_epose(const EPoseArgs a) {
    const vx_essential_result* e = &a.res->ess;
    double out[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (e->ok) {
        double R[9];
        for (int k = 0; k < 9; ++k) R[k] = e->R[k];
        // q_cl: Shepperd's method, as PoseFromRt (Eigen::Quaterniond(Matrix3d))
        double x, y, z, w;
        const double tr = R[0] + R[4] + R[8];
        if (tr > 0.0) {
            const double s = sqrt(tr + 1.0) * 2.0;
            w = 0.25 * s; x = (R[7] - R[5]) / s; y = (R[2] - R[6]) / s; z = (R[3] - R[1]) / s;
        } else if (R[0] > R[4] && R[0] > R[8]) {
            const double s = sqrt(1.0 + R[0] - R[4] - R[8]) * 2.0;
            w = (R[7] - R[5]) / s; x = 0.25 * s; y = (R[1] + R[3]) / s; z = (R[2] + R[6]) / s;
        } else if (R[4] > R[8]) {
            const double s = sqrt(1.0 + R[4] - R[0] - R[8]) * 2.0;
            w = (R[2] - R[6]) / s; x = (R[1] + R[3]) / s; y = 0.25 * s; z = (R[5] + R[7]) / s;
        } else {
            const double s = sqrt(1.0 + R[8] - R[0] - R[4]) * 2.0;
            w = (R[3] - R[1]) / s; x = (R[2] + R[6]) / s; y = (R[5] + R[7]) / s; z = 0.25 * s;
        }
        const double inv = 1.0 / sqrt(x * x + y * y + z * z + w * w);
        const double ax = x * inv, ay = y * inv, az = z * inv, aw = w * inv;
        const double bx = a.pose_last[0], by = a.pose_last[1], bz = a.pose_last[2], bw = a.pose_last[3];
        // q = q_cl (x) q_lw, Eigen's coefficient order
        double qw = aw * bw - ax * bx - ay * by - az * bz;
        double qx = aw * bx + ax * bw + ay * bz - az * by;
        double qy = aw * by + ay * bw + az * bx - ax * bz;
        double qz = aw * bz + az * bw + ax * by - ay * bx;
        // Sophus's first-order renormalisation
        const double n2 = qx * qx + qy * qy + qz * qz + qw * qw;
        if (n2 != 1.0) {
            const double sc = 2.0 / (1.0 + n2);
            qx *= sc; qy *= sc; qz *= sc; qw *= sc;
        }
        // t = T_cl * t_lw (SE3d::operator*(Vec3d))
        const double px = a.pose_last[4], py = a.pose_last[5], pz = a.pose_last[6];
        const double ux = ay * pz - az * py, uy = az * px - ax * pz, uz = ax * py - ay * px;
        const double wx = 2 * ux, wy = 2 * uy, wz = 2 * uz;
        out[0] = qx; out[1] = qy; out[2] = qz; out[3] = qw;
        out[4] = px + aw * wx + (ay * wz - az * wy) + e->t[0];
        out[5] = py + aw * wy + (az * wx - ax * wz) + e->t[1];
        out[6] = pz + aw * wz + (ax * wy - ay * wx) + e->t[2];
    }
    for (int k = 0; k < 7; ++k) a.res->pose[k] = out[k];
}

// ------------------------------------------------------------------ Track()'s PnP -> essential decision
struct GateArgs {
    const vx_track_result* pnp;  // NULL: no last keyframe
    int min_matches, min_inliers;
    const int* n_last;           // NULL: no last frame
    int cap_last;
    const int* n_matches0;       // list 0's count, when list 1 shares its rows (else NULL)
    int* n_matches1;             // ... and list 1's gated count
    int* gate;                   // {gated query count, PnP status, gate open, 0}
};

// The decision of tracking.cpp:269-273 by the calling lane (a record read, a rule, four stores)
__device__ __forceinline__ void track_gate(const GateArgs a) {
    const int status = a.pnp ? pnp_status(*a.pnp, a.min_matches, a.min_inliers) : VX_TRACK_OK;
    const bool open = !a.pnp || status != VX_TRACK_OK;  // (:269-273)
    a.gate[0] = open && a.n_last ? min(max(*a.n_last, 0), a.cap_last) : 0;
    a.gate[1] = status;
    a.gate[2] = open ? 1 : 0;
    a.gate[3] = 0;
    if (a.n_matches0) *a.n_matches1 = open ? *a.n_matches0 : 0;
}

// ------------------------------------------------------------------ Track()'s result head and packed block
struct FinalArgs {
    const uint8_t* tk;   // vx_track_pnp_async's packed block (NULL: no last keyframe)
    int tk_cap;
    const uint8_t* te;   // vx_track_essential_async's packed block
    int te_cap;
    const int* gate;
    int has_last;
    int ess_min_matches, ess_min_inliers;
    const uint8_t* kp;   // the current frame's keypoint rows
    const int* n_kp;
    int cap_kp;
    uint8_t* out;
    size_t o_pm0, o_mask0, o_pm1, o_mask1, o_kp;
};

// k_track_final's body by the threads t of nt (a whole grid, or the workgroups of one camera of a rig).
// mask0 / mask1: where the two paths' masks are read.  kBytes = false: 4-byte aligned like the packed
// blocks' own (grid_copy_range over the count rounded up to 4, as the fetch never reads past the count);
// true: any alignment (a problem's slice of a batch's contiguous RANSAC mask), copied byte by byte up
// to the count.
template <bool kBytes>
__device__ __forceinline__ void track_final(const FinalArgs a, const uint8_t* mask0, const uint8_t* mask1, size_t t,
                                            size_t nt) {
    vx_track_frame_result* out = reinterpret_cast<vx_track_frame_result*>(a.out);
    const vx_track_essential_result* er = reinterpret_cast<const vx_track_essential_result*>(a.te);
    // the records without their first dword (status: written below by the lane that evaluates it)
    uint32_t* o_pnp = reinterpret_cast<uint32_t*>(&out->pnp);
    if (a.tk) {
        const vx_track_result* pr = reinterpret_cast<const vx_track_result*>(a.tk);
        grid_copy_range(o_pnp + 1, reinterpret_cast<const uint32_t*>(pr) + 1, sizeof(vx_track_result) - 4, t, nt);
        const int np = min(max(pr->n_pairs, 0), a.tk_cap);
        grid_copy_range(a.out + a.o_pm0, a.tk + off_pair_match<vx_track_result>(), (size_t)np * 4, t, nt);
        if (kBytes) {
            for (size_t k = t; k < (size_t)np; k += nt) a.out[a.o_mask0 + k] = mask0[k];
        } else {
            grid_copy_range(a.out + a.o_mask0, mask0, ((size_t)np + 3) & ~(size_t)3, t, nt);
        }
    } else {
        for (size_t k = 1 + t; k < sizeof(vx_track_result) / 4; k += nt) o_pnp[k] = 0;
    }
    grid_copy_range(reinterpret_cast<uint32_t*>(&out->ess) + 1, reinterpret_cast<const uint32_t*>(er) + 1,
                    sizeof(vx_track_essential_result) - 4, t, nt);
    const int ne = min(max(er->n_pairs, 0), a.te_cap);
    grid_copy_range(a.out + a.o_pm1, a.te + off_pair_match<vx_track_essential_result>(), (size_t)ne * 4, t, nt);
    if (kBytes) {
        for (size_t k = t; k < (size_t)ne; k += nt) a.out[a.o_mask1 + k] = mask1[k];
    } else {
        grid_copy_range(a.out + a.o_mask1, mask1, ((size_t)ne + 3) & ~(size_t)3, t, nt);
    }
    const int nk = min(max(*a.n_kp, 0), a.cap_kp);
    grid_copy_range(a.out + a.o_kp, a.kp, (size_t)nk * sizeof(vx_keypoint), t, nt);
    if (t != 0) return;

    const int pnp_ran = a.tk ? 1 : 0, open = a.gate[2];
    const int ess_ran = open && a.has_last ? 1 : 0;
    const int pnp_st = a.gate[1];
    const int ess_st = ess_status(*er, a.ess_min_matches, a.ess_min_inliers);  // (:306, :317)
    out->pnp.status = pnp_ran ? pnp_st : 0;
    out->ess.status = ess_st;
    int path = VX_TRACK_PATH_NONE, status, n_inliers = 0;
    double parallax = 0.0, pose[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (pnp_ran && pnp_st == VX_TRACK_OK) {  // (:269-273)
        const vx_track_result* pr = reinterpret_cast<const vx_track_result*>(a.tk);
        path = VX_TRACK_PATH_PNP;
        status = VX_TRACK_OK;
        n_inliers = pr->pnp.n_inliers;
        parallax = pr->parallax;
        for (int k = 0; k < 7; ++k) pose[k] = pr->pnp.pose[k];
    } else if (ess_ran) {  // (:278)
        status = ess_st;
        if (ess_st == VX_TRACK_OK) {
            path = VX_TRACK_PATH_ESSENTIAL;
            n_inliers = er->ess.n_inliers;
            parallax = er->parallax;
            for (int k = 0; k < 7; ++k) pose[k] = er->pose[k];
        }
    } else {
        status = pnp_st;  // no last frame (:282): PnP's failure stands
    }
    out->path = path;
    out->status = status;
    out->n_inliers = n_inliers;
    out->n_keypoints = nk;
    out->parallax = parallax;
    for (int k = 0; k < 7; ++k) out->pose[k] = pose[k];
    out->pnp_ran = pnp_ran;
    out->ess_ran = ess_ran;
}

// ---------------------------------------------------------------- host side
// How the entry points (track.hip, track_ess.hip, track_frame.hip, track_rig.hip) fill the records
// above and check what goes into them: ONE statement of each, beside the record it fills.

// Track()'s packed block: vx_track_frame_result | pair_match0 | mask0 | pair_match1 | mask1 | keypoint
// rows, each part on a 16-byte boundary.  The only place the chain is written.
inline size_t FrameBlock::pm(int which) const {
    return align16(sizeof(vx_track_frame_result)) + (which ? align16((size_t)cap0 * 4) + align16((size_t)cap0) : 0);
}
inline size_t FrameBlock::mask(int which) const { return pm(which) + align16((size_t)(which ? cap1 : cap0) * 4); }
inline size_t FrameBlock::kp() const { return mask(1) + align16((size_t)cap1); }
inline size_t FrameBlock::bytes(bool with_keypoints) const {
    return kp() + (with_keypoints ? align16((size_t)cap_kp * sizeof(vx_keypoint)) : 0);
}

// a path's pair arrays out of a fetched block h (vx_track_frame_pairs, vx_track_rig_pairs)
inline int copy_pairs(vx_ctx* c, const uint8_t* h, const FrameBlock& b, int which, int32_t* pair_match, uint8_t* mask,
                      int cap_pairs) {
    const vx_track_frame_result* r = reinterpret_cast<const vx_track_frame_result*>(h);
    const int np = which ? r->ess.n_pairs : r->pnp.n_pairs;
    if ((pair_match || mask) && np > cap_pairs) return set_error(c, VX_ERR_CAPACITY, "need %d pairs, cap %d", np, cap_pairs);
    if (pair_match && np) std::memcpy(pair_match, h + b.pm(which), (size_t)np * 4);
    if (mask && np) std::memcpy(mask, h + b.mask(which), (size_t)np);
    return VX_OK;
}

// the map side of TrackArgs: keyframe row k's feature rows, the landmark arrays and their id table
inline void map_side(TrackArgs& a, const vx_dmap* m, int k) {
    a.f0 = m->kf_feat_ptr[k];
    a.nf = (int)(m->kf_feat_ptr[k + 1] - m->kf_feat_ptr[k]);
    a.feat_uv = m->feat_uv.as<double>();
    a.feat_lm = m->feat_lm.as<uint64_t>();
    a.feat_fl = m->feat_fl.as<uint8_t>();
    a.ht_key = m->ht_key.as<uint64_t>();
    a.ht_val = m->ht_val.as<int>();
    a.ht_mask = m->ht_cap - 1;
    a.lm_bad = m->lm_bad.as<uint8_t>();
    a.lm_pos = m->lm_pos.as<double>();
}

// options and intrinsics of the two pair records
inline void set_options(TrackArgs& a, const vx_track_options& o, const double* intr4) {
    a.min_matches = o.min_matches;
    a.min_inliers = o.min_inliers;
    a.pnp = o.pnp;
    for (int i = 0; i < 4; ++i) a.intr[i] = intr4[i];
}
inline void set_options(EPairArgs& a, const vx_track_essential_options& o, const double* intr4) {
    a.min_matches = o.min_matches;
    a.ess = o.ess;
    for (int i = 0; i < 4; ++i) a.intr[i] = intr4[i];
}
// PnP's hypothesis grid: the host-side bound of the budget (k_pnp_hyp exits beyond the resolved one)
inline int pnp_hyp_bound(const vx_pnp_options& o) { return std::max(1, o.max_iterations < 0 ? 100 : o.max_iterations); }

// A = TrackArgs or EPairArgs: its packed block R | pair_match[cap] | mask[cap] (track_common.hpp) at `block`
template <class A>
inline void packed_outputs(A& a, uint8_t* block, int cap) {
    using R = typename std::remove_pointer<decltype(a.res)>::type;
    a.pair_match = reinterpret_cast<int*>(block + off_pair_match<R>());
    a.mask = block + off_mask<R>(cap);
    a.res = reinterpret_cast<R*>(block);
}

// The problem record a pair kernel leaves for its RANSAC.  One problem: offsets[2] | intr[4] | options.
// A batch: offsets[P + 1] | the cameras' {0, n} records | intr[4 P] | options[P].
template <class A>
using OptOf = typename std::remove_pointer<decltype(A::opt_out)>::type;
constexpr size_t kProb1Intr = 16, kProb1Opt = kProb1Intr + 4 * sizeof(double);
template <class A>
constexpr size_t prob1_bytes() { return kProb1Opt + sizeof(OptOf<A>); }
template <class A>
inline void prob1_pointers(A& a, uint8_t* prob) {
    a.offsets = reinterpret_cast<int*>(prob);
    a.intr_out = reinterpret_cast<double*>(prob + kProb1Intr);
    a.opt_out = reinterpret_cast<OptOf<A>*>(prob + kProb1Opt);
}
constexpr int kProbMax = VX_MAX_RIG_CAMERAS;
constexpr size_t kProbOffsets = 0, kProbCnt = 128, kProbIntr = 256, kProbOpt = 768;
static_assert((kProbMax + 1) * sizeof(int) <= 128 && 2 * kProbMax * sizeof(int) <= 128 && 4 * kProbMax * sizeof(double) <= 512,
              "problem record");
template <class A>
constexpr size_t prob_bytes() { return kProbOpt + kProbMax * sizeof(OptOf<A>); }
template <class A>
inline void prob_pointers(A& a, uint8_t* prob, int i) {  // problem i of a batch
    a.offsets = reinterpret_cast<int*>(prob + kProbCnt) + 2 * i;
    a.intr_out = reinterpret_cast<double*>(prob + kProbIntr) + 4 * i;
    a.opt_out = reinterpret_cast<OptOf<A>*>(prob + kProbOpt) + i;
}

// pnp: the PnP record the decision reads (NULL: no last keyframe; po is not read then); last: NULL without a
// last frame.  n_matches0 / n_matches1 (list 1 sharing list 0's rows) stay with the caller.
inline void gate_args(GateArgs& g, const vx_track_result* pnp, const vx_track_options* po, const vx_frame* last, int* gate) {
    g.pnp = pnp;
    g.min_matches = pnp ? po->min_matches : 0;
    g.min_inliers = pnp ? po->min_inliers : 0;
    g.n_last = last ? last->count() : nullptr;
    g.cap_last = last ? last->cap : 0;
    g.gate = gate;
}

inline void epose_args(EPoseArgs& p, vx_track_essential_result* res, const double* pose_last7) {
    p.res = res;
    for (int i = 0; i < 7; ++i) p.pose_last[i] = pose_last7 ? pose_last7[i] : (i == 3 ? 1.0 : 0.0);
}

// tk (NULL: no last keyframe) / te: the two paths' packed blocks, of b.cap0 / b.cap1 pairs
inline void final_args(FinalArgs& f, const uint8_t* tk, const uint8_t* te, const FrameBlock& b, const int* gate,
                       bool has_last, const vx_track_essential_options& eo, const vx_frame* curr, uint8_t* out) {
    f.tk = tk;
    f.tk_cap = b.cap0;
    f.te = te;
    f.te_cap = b.cap1;
    f.gate = gate;
    f.has_last = has_last ? 1 : 0;
    f.ess_min_matches = eo.min_matches;
    f.ess_min_inliers = eo.min_inliers;
    f.kp = reinterpret_cast<const uint8_t*>(curr->kp());
    f.n_kp = curr->count();
    f.cap_kp = b.cap_kp;
    f.out = out;
    f.o_pm0 = b.pm(0);
    f.o_mask0 = b.mask(0);
    f.o_pm1 = b.pm(1);
    f.o_mask1 = b.mask(1);
    f.o_kp = b.kp();
}

// The checks, each under the text that names the call (and the camera).  NOTE the two focal-length
// predicates differ: vx_track_pnp_async tests fx != 0 && fy != 0 only (track.hip), the essential path and
// the rig also fx + fy != 0 (check_focal).  Left as they are: unifying them changes what is refused.
inline int check_focal(vx_ctx* c, const char* who, const double* intr4) {
    if (intr4[0] != 0.0 && intr4[1] != 0.0 && intr4[0] + intr4[1] != 0.0) return VX_OK;
    return set_error(c, VX_ERR_INVALID, "%s: zero focal length", who);
}
inline int check_pnp_options(vx_ctx* c, const char* who, const vx_pnp_options& o) {
    if (o.max_iterations > 4096) return set_error(c, VX_ERR_INVALID, "%s: max_iterations %d > 4096", who, o.max_iterations);
    if (o.refine_iterations < 0 || !(o.reproj_error >= 0.0)) return set_error(c, VX_ERR_INVALID, "%s: bad PnP options", who);
    return VX_OK;
}
inline int check_ess_options(vx_ctx* c, const char* who, const vx_essential_options& o) {
    if (o.max_iterations > 4096) return set_error(c, VX_ERR_INVALID, "%s: max_iterations %d > 4096", who, o.max_iterations);
    if (!(o.threshold >= 0.0)) return set_error(c, VX_ERR_INVALID, "%s: bad essential options", who);
    return VX_OK;
}
// the host values of the essential path, before anything touches a device
inline int check_ess_host_args(vx_ctx* c, const char* who, const double* intr4, const vx_track_essential_options* opt) {
    if (!intr4 || !opt) return set_error(c, VX_ERR_INVALID, "%s: null intrinsics / options", who);
    int rc;
    if ((rc = check_focal(c, who, intr4))) return rc;
    return check_ess_options(c, who, opt->ess);
}
// One camera's frames: a current frame and intrinsics, a last keyframe or a last frame, all on the context's
// device, the last keyframe in the map.  map_ok: a last keyframe has the map and the options it needs.
inline int check_frames(vx_ctx* c, const char* who, const vx_dmap* m, bool map_ok, uint64_t last_kf_id,
                        const vx_frame* last_kf, const vx_frame* last, const vx_frame* curr, const double* intr4) {
    if (!curr || !curr->block.p || !intr4) return set_error(c, VX_ERR_INVALID, "%s: null argument", who);
    if (!last_kf && !last) return set_error(c, VX_ERR_INVALID, "%s: neither a last keyframe nor a last frame", who);
    if (last_kf && !map_ok) return set_error(c, VX_ERR_INVALID, "%s: a last keyframe without a map / options", who);
    for (const vx_frame* f : {last_kf, last, curr})
        if (f && (!f->block.p || f->device != c->device))
            return set_error(c, VX_ERR_INVALID, "%s: frame and context on different devices", who);
    if (last_kf && m->kf_index.find(last_kf_id) == m->kf_index.end())
        return set_error(c, VX_ERR_INVALID, "%s: keyframe %llu is not in the map", who, (unsigned long long)last_kf_id);
    return VX_OK;
}

}  // namespace trk
}  // namespace vx
