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
#pragma once

#include "vx_internal.hpp"
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

}  // namespace trk
}  // namespace vx
