// landmarks.hip — landmark creation on keyframe insertion.
//
// Replaces the two per-feature / per-match loops Tracking::CreateKeyFrame runs right before
// LocalBA (core/frontend/tracking.cpp:577-580):
//   CreateLandmarksFromDepth (tracking.cpp:586-650)  one thread per feature: rounding to the depth
//        pixel (static_cast<int>(x + 0.5)), TUM depth scale 5000 (u16) / metres (f32, f64),
//        0.1 <= d <= 10, Camera::pixelToCamera (camera.cpp:30-34), T_cw.inverse() * pc (Sophus).
//   TriangulateWithLastKeyFrame + TriangulatePoint (tracking.cpp:856-945)  one thread per match:
//        parallax angle of the two bearing rays (>= triangulation_min_angle_deg), the 4x4 DLT
//        system of ProjectionMatrix (K [R | t] with the CURRENT frame's camera for both views,
//        tracking.cpp:864-867), its right singular vector of the smallest singular value
//        (Eigen::JacobiSVD in the reference; here a one-sided Jacobi SVD in registers — the null
//        vector is unique up to sign for a rank-3 system, so the point is the same to rounding),
//        ProjectToPixel in both views (projection.h:11-31) and the reprojection gate.
// The reference marks features as it goes, so a later match whose train feature an earlier match
// already triangulated is skipped: the first passing match per train feature wins (atomicMin),
// which is the sequential outcome because the matcher's query indices are unique.  Created
// landmarks are numbered in input order (an order-preserving scan), as landmark_id_++ numbers them.
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "vx_internal.hpp"
#include "ba_common.hpp"
#include "lm_math.hpp"

namespace vx {
namespace {

using namespace vx::ba;

constexpr int kThreads = 256;
constexpr int kScanThreads = 1024;

using namespace vx::lm;  // Pose, inv_apply, depth_point, tri_gate (lm_math.hpp)

// ---------------------------------------------------------------- CreateLandmarksFromDepth
struct DepthArgs {
    const double* uv;        // 2 per feature (Feature::position)
    const uint8_t* has;      // Feature::has_landmark
    int n;
    DepthView v;             // depth image, intrinsics, T_cw
    int* valid;
    double* pw;              // 3 per feature (uncompacted)
};

__global__ __launch_bounds__(kThreads) void k_depth_lm(DepthArgs a) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.n) return;
    int ok = 0;
    if (!a.has[i]) {
        D3 p;
        if (depth_point(a.v, a.uv[2 * i], a.uv[2 * i + 1], p)) {
            a.pw[3 * i] = p.x;
            a.pw[3 * i + 1] = p.y;
            a.pw[3 * i + 2] = p.z;
            ok = 1;
        }
    }
    a.valid[i] = ok;
}

// ---------------------------------------------------------------- TriangulateWithLastKeyFrame
struct TriArgs {
    const double* uv1;
    const uint8_t* has1;
    int n1;
    const double* uv2;
    const uint8_t* has2;
    int n2;
    const vx_match* m;
    int n;
    double c1[4], c2[4];     // fx fy cx cy of the last / current frame camera
    Pose T1, T2;
    double min_angle_rad, max_err;
    int* valid;
    double* pw;
    int* winner;             // n2: first passing match per train feature
    int* qseen;              // n1: duplicate query detection
    int* err;
};

__global__ __launch_bounds__(kThreads) void k_triangulate(TriArgs a) {
    const int k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= a.n) return;
    a.valid[k] = 0;
    const vx_match mt = a.m[k];
    const int qi = mt.query_idx, ti = mt.train_idx;
    if (qi < 0 || qi >= a.n1 || ti < 0 || ti >= a.n2) {
        atomicOr(a.err, 1);
        return;
    }
    if (atomicAdd(&a.qseen[qi], 1) != 0) atomicOr(a.err, 2);
    if (a.has1[qi] || a.has2[ti]) return;
    const double x1 = a.uv1[2 * qi], y1 = a.uv1[2 * qi + 1];
    const double x2 = a.uv2[2 * ti], y2 = a.uv2[2 * ti + 1];
    D3 pw;
    if (!tri_gate(x1, y1, x2, y2, a.c1, a.c2, a.T1, a.T2, a.min_angle_rad, a.max_err, pw)) return;
    a.valid[k] = 1;
    a.pw[3 * k] = pw.x;
    a.pw[3 * k + 1] = pw.y;
    a.pw[3 * k + 2] = pw.z;
    atomicMin(&a.winner[ti], k);
}

__global__ __launch_bounds__(kThreads) void k_tri_resolve(int* valid, const vx_match* m, const int* winner, int n) {
    const int k = blockIdx.x * kThreads + threadIdx.x;
    if (k < n && valid[k] && winner[m[k].train_idx] != k) valid[k] = 0;
}

// Order-preserving compaction: index[i] = rank of i among the valid entries (-1 otherwise), the
// valid points packed in that order; one workgroup, each thread owns a contiguous chunk.
__global__ __launch_bounds__(kScanThreads) void k_compact(const int* valid, const double* pw, int n, int* index,
                                                          double* out, int* count) {
    __shared__ int part[kScanThreads];
    const int t = threadIdx.x;
    const int chunk = (n + kScanThreads - 1) / kScanThreads;
    const int b = min(n, t * chunk), e = min(n, b + chunk);
    int c = 0;
    for (int i = b; i < e; ++i) c += valid[i];
    part[t] = c;
    __syncthreads();
    for (int o = 1; o < kScanThreads; o <<= 1) {  // inclusive Hillis-Steele scan
        const int v = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int r = part[t] - c;
    for (int i = b; i < e; ++i) {
        if (valid[i]) {
            index[i] = r;
            out[3 * r] = pw[3 * i];
            out[3 * r + 1] = pw[3 * i + 1];
            out[3 * r + 2] = pw[3 * i + 2];
            ++r;
        } else {
            index[i] = -1;
        }
    }
    if (t == kScanThreads - 1) *count = part[t];
}

template <class T>
int to_dev(vx_ctx* c, DevBuf& d, const T* h, size_t n) {
    VX_HIP(c, d.ensure(std::max<size_t>(1, n) * sizeof(T)));
    if (n) VX_HIP(c, hipMemcpyAsync(d.p, h, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    return VX_OK;
}

Pose host_pose(const double* p) {
    Pose T;
    for (int j = 0; j < 4; ++j) T.q[j] = p[j];
    for (int j = 0; j < 3; ++j) T.t[j] = p[4 + j];
    return T;
}

int fetch_compacted(vx_ctx* c, int n, int32_t* out_index, double* out_pw, int* n_created) {
    int cnt = 0;
    VX_HIP(c, hipMemcpyAsync(&cnt, c->lm_count.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    VX_HIP(c, hipStreamSynchronize(c->stream));
    if (out_index) VX_HIP(c, hipMemcpy(out_index, c->lm_index.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    if (out_pw && cnt) VX_HIP(c, hipMemcpy(out_pw, c->lm_out.p, (size_t)cnt * 3 * sizeof(double), hipMemcpyDeviceToHost));
    *n_created = cnt;
    return VX_OK;
}

int compact(vx_ctx* c, int n) {
    VX_HIP(c, c->lm_index.ensure((size_t)std::max(n, 1) * sizeof(int)));
    VX_HIP(c, c->lm_out.ensure((size_t)std::max(n, 1) * 3 * sizeof(double)));
    VX_HIP(c, c->lm_count.ensure(4 * sizeof(int)));
    ProfScope ps(c, kStLmCompact);
    hipLaunchKernelGGL(k_compact, dim3(1), dim3(kScanThreads), 0, c->stream, c->lm_valid.as<int>(),
                       c->lm_pw.as<double>(), n, c->lm_index.as<int>(), c->lm_out.as<double>(), c->lm_count.as<int>());
    VX_LAUNCH_CHECK(c, "k_compact");
    return VX_OK;
}

}  // namespace
}  // namespace vx

using namespace vx;

extern "C" {

int vx_depth_landmarks(vx_ctx* c, const double* feat_uv, const uint8_t* feat_has_lm, int n_feat, const void* depth,
                       int depth_type, int rows, int cols, int64_t row_stride, const double* intr4,
                       const double* pose7, int32_t* out_index, double* out_pw, int* n_created) {
    if (!c || !n_created || n_feat < 0 || (n_feat > 0 && (!feat_uv || !feat_has_lm)) || !intr4 || !pose7)
        return c ? set_error(c, VX_ERR_INVALID, "vx_depth_landmarks: bad arguments") : VX_ERR_INVALID;
    *n_created = 0;
    if (depth_type < VX_DEPTH_U16 || depth_type > VX_DEPTH_F64)
        return set_error(c, VX_ERR_INVALID, "unknown depth type %d", depth_type);
    const int esz = depth_type == VX_DEPTH_U16 ? 2 : (depth_type == VX_DEPTH_F32 ? 4 : 8);
    if (n_feat == 0 || !depth || rows <= 0 || cols <= 0) {  // depth.empty() (tracking.cpp:591-594)
        for (int i = 0; out_index && i < n_feat; ++i) out_index[i] = -1;
        return VX_OK;
    }
    if (row_stride < (int64_t)cols * esz) return set_error(c, VX_ERR_INVALID, "row_stride < cols * element size");
    VX_HIP(c, hipSetDevice(c->device));
    int rc;
    if ((rc = to_dev(c, c->lm_in0, feat_uv, (size_t)n_feat * 2))) return rc;
    if ((rc = to_dev(c, c->lm_in1, feat_has_lm, (size_t)n_feat))) return rc;
    if ((rc = to_dev(c, c->lm_depth, static_cast<const uint8_t*>(depth), (size_t)row_stride * rows))) return rc;
    VX_HIP(c, c->lm_valid.ensure((size_t)n_feat * sizeof(int)));
    VX_HIP(c, c->lm_pw.ensure((size_t)n_feat * 3 * sizeof(double)));
    DepthArgs a{};
    a.uv = c->lm_in0.as<double>();
    a.has = c->lm_in1.as<uint8_t>();
    a.n = n_feat;
    a.v.depth = c->lm_depth.as<uint8_t>();
    a.v.type = depth_type;
    a.v.rows = rows;
    a.v.cols = cols;
    a.v.stride = row_stride;
    a.v.fx = intr4[0];
    a.v.fy = intr4[1];
    a.v.cx = intr4[2];
    a.v.cy = intr4[3];
    a.v.T = host_pose(pose7);
    a.valid = c->lm_valid.as<int>();
    a.pw = c->lm_pw.as<double>();
    VX_HIP(c, launch(c, kStLmDepth, k_depth_lm, dim3((n_feat + kThreads - 1) / kThreads), dim3(kThreads), 0,
                     c->stream, a));
    if ((rc = compact(c, n_feat))) return rc;
    return fetch_compacted(c, n_feat, out_index, out_pw, n_created);
}

int vx_triangulate(vx_ctx* c, const double* uv1, const uint8_t* has1, int n1, const double* intr1, const double* pose1,
                   const double* uv2, const uint8_t* has2, int n2, const double* intr2, const double* pose2,
                   const vx_match* matches, int n_matches, double min_angle_deg, double max_reproj_error,
                   int32_t* out_index, double* out_pw, int* n_created) {
    if (!c || !n_created || n_matches < 0 || n1 < 0 || n2 < 0 || !intr1 || !intr2 || !pose1 || !pose2 ||
        (n_matches > 0 && (!matches || !uv1 || !uv2 || !has1 || !has2)))
        return c ? set_error(c, VX_ERR_INVALID, "vx_triangulate: bad arguments") : VX_ERR_INVALID;
    *n_created = 0;
    if (n_matches == 0) return VX_OK;
    VX_HIP(c, hipSetDevice(c->device));
    int rc;
    if ((rc = to_dev(c, c->lm_in0, uv1, (size_t)n1 * 2))) return rc;
    if ((rc = to_dev(c, c->lm_in1, has1, (size_t)n1))) return rc;
    if ((rc = to_dev(c, c->lm_in2, uv2, (size_t)n2 * 2))) return rc;
    if ((rc = to_dev(c, c->lm_in3, has2, (size_t)n2))) return rc;
    if ((rc = to_dev(c, c->lm_in4, matches, (size_t)n_matches))) return rc;
    VX_HIP(c, c->lm_valid.ensure((size_t)n_matches * sizeof(int)));
    VX_HIP(c, c->lm_pw.ensure((size_t)n_matches * 3 * sizeof(double)));
    VX_HIP(c, c->lm_aux.ensure(((size_t)n2 + n1 + 4) * sizeof(int)));
    int* winner = c->lm_aux.as<int>();
    int* qseen = winner + n2;
    int* err = qseen + n1;
    VX_HIP(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(winner), INT_MAX, (size_t)std::max(n2, 0), c->stream));
    VX_HIP(c, hipMemsetAsync(qseen, 0, ((size_t)n1 + 1) * sizeof(int), c->stream));
    TriArgs a{};
    a.uv1 = c->lm_in0.as<double>();
    a.has1 = c->lm_in1.as<uint8_t>();
    a.n1 = n1;
    a.uv2 = c->lm_in2.as<double>();
    a.has2 = c->lm_in3.as<uint8_t>();
    a.n2 = n2;
    a.m = c->lm_in4.as<vx_match>();
    a.n = n_matches;
    for (int j = 0; j < 4; ++j) {
        a.c1[j] = intr1[j];
        a.c2[j] = intr2[j];
    }
    a.T1 = host_pose(pose1);
    a.T2 = host_pose(pose2);
    a.min_angle_rad = min_angle_deg * M_PI / 180.0;  // tracking.cpp:870-871
    a.max_err = max_reproj_error;
    a.valid = c->lm_valid.as<int>();
    a.pw = c->lm_pw.as<double>();
    a.winner = winner;
    a.qseen = qseen;
    a.err = err;
    const dim3 grid((n_matches + kThreads - 1) / kThreads);
    VX_HIP(c, launch(c, kStLmTriangulate, k_triangulate, grid, dim3(kThreads), 0, c->stream, a));
    hipLaunchKernelGGL(k_tri_resolve, grid, dim3(kThreads), 0, c->stream, a.valid, a.m, winner, n_matches);
    VX_LAUNCH_CHECK(c, "k_tri_resolve");
    if ((rc = compact(c, n_matches))) return rc;
    int herr = 0;
    VX_HIP(c, hipMemcpyAsync(&herr, err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if ((rc = fetch_compacted(c, n_matches, out_index, out_pw, n_created))) return rc;
    if (herr & 1) return set_error(c, VX_ERR_INVALID, "match index out of range");
    if (herr & 2) return set_error(c, VX_ERR_INVALID, "duplicate query index (matches must come from one knnMatch)");
    return VX_OK;
}

}  // extern "C"
