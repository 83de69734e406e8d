// lm_math.hpp — the device arithmetic of landmark creation, shared by the host-array entry points
// (landmarks.hip: vx_depth_landmarks, vx_triangulate) and the resident-map sequence (keyframe.hip:
// vx_dmap_create_keyframe): Sophus' T.inverse() * p, ProjectToPixel, the DLT null vector, the
// depth-pixel conversion of CreateLandmarksFromDepth (tracking.cpp:596-640) and the gate of
// TriangulateWithLastKeyFrame + TriangulatePoint (tracking.cpp:856-945).  One body, so both paths
// produce the same bits for the same inputs.
#pragma once
#include <cmath>
#include <cstdint>

#include "vx_internal.hpp"
#include "ba_common.hpp"

namespace vx {
namespace lm {

using namespace vx::ba;

struct Pose {  // Sophus SE3d: unit quaternion (x y z w) + translation, T_cw
    double q[4], t[3];
};

// Eigen _transformVector: q * v
__device__ __forceinline__ D3 qrot(const double* q, D3 v) {
    const D3 qv{q[0], q[1], q[2]};
    D3 uv{qv.y * v.z - qv.z * v.y, qv.z * v.x - qv.x * v.z, qv.x * v.y - qv.y * v.x};
    uv = {uv.x + uv.x, uv.y + uv.y, uv.z + uv.z};
    const D3 c{qv.y * uv.z - qv.z * uv.y, qv.z * uv.x - qv.x * uv.z, qv.x * uv.y - qv.y * uv.x};
    return {v.x + q[3] * uv.x + c.x, v.y + q[3] * uv.y + c.y, v.z + q[3] * uv.z + c.z};
}

// Sophus T.inverse() * p: inverse = (conj(q), conj(q) * (-t)), then rotate + translate
__device__ __forceinline__ D3 inv_apply(const Pose& T, D3 p) {
    const double qc[4] = {-T.q[0], -T.q[1], -T.q[2], T.q[3]};
    const D3 ti = qrot(qc, {T.t[0] * -1.0, T.t[1] * -1.0, T.t[2] * -1.0});
    const D3 r = qrot(qc, p);
    return {r.x + ti.x, r.y + ti.y, r.z + ti.z};
}

// The depth image CreateLandmarksFromDepth reads and the frame it back-projects through.
struct DepthView {
    const uint8_t* depth;
    int type, rows, cols;
    long long stride;        // bytes per depth row
    double fx, fy, cx, cy;
    Pose T;
};

// One feature of CreateLandmarksFromDepth (tracking.cpp:596-640): the rounded depth pixel, the TUM
// scale, the range gate, pixelToCamera and T_cw.inverse() * pc.  False when no landmark is made.
__device__ __forceinline__ bool depth_point(const DepthView& a, double x, double y, D3& out) {
    const int u = (int)(x + 0.5), v = (int)(y + 0.5);  // static_cast<int>: truncation
    if (!(u >= 0 && u < a.cols && v >= 0 && v < a.rows)) return false;
    const uint8_t* row = a.depth + (long long)v * a.stride;
    double d = 0.0;
    bool have = true;
    if (a.type == VX_DEPTH_U16) {
        const uint16_t raw = reinterpret_cast<const uint16_t*>(row)[u];
        have = raw != 0;
        d = (double)raw / 5000.0;  // kDepthScale (tracking.cpp:601)
    } else if (a.type == VX_DEPTH_F32) {
        d = (double)reinterpret_cast<const float*>(row)[u];
    } else {
        d = reinterpret_cast<const double*>(row)[u];
    }
    if (!(have && !(d < 0.1 || d > 10.0))) return false;  // kMinDepth / kMaxDepth (tracking.cpp:602-603)
    const double xn = (x - a.cx) / a.fx, yn = (y - a.cy) / a.fy;
    out = inv_apply(a.T, {xn * d, yn * d, d});
    return true;
}

// rotation matrix of a unit quaternion (Eigen toRotationMatrix)
__device__ __forceinline__ void qmat(const double* q, double* R) { rot_from_quat(q, R); }

// ProjectToPixel (projection.h:11-31)
__device__ __forceinline__ bool project(const double* c, const Pose& T, D3 pw, double& u, double& v) {
    const D3 r = qrot(T.q, pw);
    const D3 pc{r.x + T.t[0], r.y + T.t[1], r.z + T.t[2]};
    if (pc.z <= 1e-6) return false;
    const double inv_z = 1.0 / pc.z;
    u = c[0] * (pc.x * inv_z) + c[2];
    v = c[1] * (pc.y * inv_z) + c[3];
    return true;
}

// Right singular vector of the smallest singular value of the 4x4 A (row-major) by one-sided
// Jacobi (Hestenes): rotate column pairs of A V until they are orthogonal, V accumulates the
// rotations; the column of least norm of A V gives the singular vector.
__device__ inline void null_vector4(double* A, double* X) {
    double V[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    for (int sweep = 0; sweep < 12; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    al += A[4 * r + p] * A[4 * r + p];
                    be += A[4 * r + q] * A[4 * r + q];
                    ga += A[4 * r + p] * A[4 * r + q];
                }
                if (!(fabs(ga) > 1e-15 * sqrt(al * be))) continue;
                rotated = true;
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double ap = A[4 * r + p], aq = A[4 * r + q];
                    A[4 * r + p] = cs * ap - sn * aq;
                    A[4 * r + q] = sn * ap + cs * aq;
                    const double vp = V[4 * r + p], vq = V[4 * r + q];
                    V[4 * r + p] = cs * vp - sn * vq;
                    V[4 * r + q] = sn * vp + cs * vq;
                }
            }
        if (!rotated) break;
    }
    int best = 0;
    double bn = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) s += A[4 * r + c] * A[4 * r + c];
        if (c == 0 || s < bn) {
            bn = s;
            best = c;
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) X[r] = best == 0 ? V[4 * r] : best == 1 ? V[4 * r + 1] : best == 2 ? V[4 * r + 2] : V[4 * r + 3];
}

// One match of TriangulateWithLastKeyFrame after its has_landmark tests: feature (x1, y1) of the
// last keyframe (camera c1, pose T1) against (x2, y2) of the current frame (c2, T2).  False when a
// gate rejects the pair, else the triangulated point in pw.
__device__ __forceinline__ bool tri_gate(double x1, double y1, double x2, double y2, const double* c1, const double* c2,
                                         const Pose& T1, const Pose& T2, double min_angle_rad, double max_err, D3& out) {
    // parallax (tracking.cpp:878-890): bearings of pixelToCamera(px, 1), normalized, rotated by
    // T_cw.inverse().rotationMatrix()
    double f1[3] = {(x1 - c1[2]) / c1[0], (y1 - c1[3]) / c1[1], 1.0};
    double f2[3] = {(x2 - c2[2]) / c2[0], (y2 - c2[3]) / c2[1], 1.0};
    {
        const double n1 = sqrt(f1[0] * f1[0] + f1[1] * f1[1] + f1[2] * f1[2]);
        const double n2 = sqrt(f2[0] * f2[0] + f2[1] * f2[1] + f2[2] * f2[2]);
        for (int j = 0; j < 3; ++j) {
            f1[j] = f1[j] / n1;
            f2[j] = f2[j] / n2;
        }
    }
    double R1[9], R2[9];
    {
        const double q1c[4] = {-T1.q[0], -T1.q[1], -T1.q[2], T1.q[3]};
        const double q2c[4] = {-T2.q[0], -T2.q[1], -T2.q[2], T2.q[3]};
        qmat(q1c, R1);
        qmat(q2c, R2);
    }
    double g1[3], g2[3];
    for (int r = 0; r < 3; ++r) {
        g1[r] = R1[3 * r] * f1[0] + R1[3 * r + 1] * f1[1] + R1[3 * r + 2] * f1[2];
        g2[r] = R2[3 * r] * f2[0] + R2[3 * r + 1] * f2[1] + R2[3 * r + 2] * f2[2];
    }
    const double dot = g1[0] * g2[0] + g1[1] * g2[1] + g1[2] * g2[2];
    const double m1 = sqrt(g1[0] * g1[0] + g1[1] * g1[1] + g1[2] * g1[2]);
    const double m2 = sqrt(g2[0] * g2[0] + g2[1] * g2[1] + g2[2] * g2[2]);
    const double cosa = fmin(fmax(dot / (m1 * m2), -1.0), 1.0);
    if (acos(cosa) < min_angle_rad) return false;
    // DLT (tracking.cpp:931-945): P = K [R | t] with the current frame's camera for both views
    double P1[12], P2[12];
    {
        double Ra[9], Rb[9];
        qmat(T1.q, Ra);
        qmat(T2.q, Rb);
        const double* K = c2;
        for (int c = 0; c < 4; ++c) {
            const double r0a = c < 3 ? Ra[c] : T1.t[0], r1a = c < 3 ? Ra[3 + c] : T1.t[1], r2a = c < 3 ? Ra[6 + c] : T1.t[2];
            const double r0b = c < 3 ? Rb[c] : T2.t[0], r1b = c < 3 ? Rb[3 + c] : T2.t[1], r2b = c < 3 ? Rb[6 + c] : T2.t[2];
            P1[c] = K[0] * r0a + K[2] * r2a;
            P1[4 + c] = K[1] * r1a + K[3] * r2a;
            P1[8 + c] = r2a;
            P2[c] = K[0] * r0b + K[2] * r2b;
            P2[4 + c] = K[1] * r1b + K[3] * r2b;
            P2[8 + c] = r2b;
        }
    }
    double A[16];
    for (int c = 0; c < 4; ++c) {
        A[c] = x1 * P1[8 + c] - P1[c];
        A[4 + c] = y1 * P1[8 + c] - P1[4 + c];
        A[8 + c] = x2 * P2[8 + c] - P2[c];
        A[12 + c] = y2 * P2[8 + c] - P2[4 + c];
    }
    double X[4];
    null_vector4(A, X);
    const D3 pw{X[0] / X[3], X[1] / X[3], X[2] / X[3]};
    if (!(isfinite(pw.x) && isfinite(pw.y) && isfinite(pw.z))) return false;
    double u1, v1, u2, v2;
    if (!project(c1, T1, pw, u1, v1)) return false;
    if (!project(c2, T2, pw, u2, v2)) return false;
    const double e1 = sqrt((u1 - x1) * (u1 - x1) + (v1 - y1) * (v1 - y1));
    const double e2 = sqrt((u2 - x2) * (u2 - x2) + (v2 - y2) * (v2 - y2));
    if (e1 > max_err || e2 > max_err) return false;
    out = pw;
    return true;
}

}  // namespace lm
}  // namespace vx
