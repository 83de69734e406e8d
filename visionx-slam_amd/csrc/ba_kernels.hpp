// ba_kernels.hpp — device code of ba.hip, included by it alone (ba.hip is one translation unit): the
// constants of the LocalBA kernels, the helpers every path shares (pose_in / pose_out, solve_pose, the
// stop rule, one pose-stage observation, one landmark-stage observation) and the two-kernel path
// k_pose_kf -> k_landmark_solve (large windows: k_pose_solve_g + k_landmark), with k_ba_reset.  ba.hip's
// header comment describes the path; BAState and BAArgs are declared in ba_plan.hpp.
#pragma once
#include "vx_internal.hpp"
#include "vx_ktrace.hpp"
#include "ba_common.hpp"
#include "ba_plan.hpp"

namespace vx {
namespace {

using namespace vx::ba;

constexpr int kPoseBlock = kBaPoseBlock;  // threads per pose-stage workgroup
constexpr int kNTerms = 29;      // 21 H (upper) + 6 b + cost + count
constexpr int kStride = kBaStride;  // doubles per keyframe block in global memory
// LDS slot stride of k_landmark_solve: 33, not 32 doubles — a 256-B stride is one full turn of the
// 64 four-byte LDS banks, so lanes reading different keyframes' slots would all hit one bank
constexpr int kLdsStride = 33;
constexpr int kMaxIter = kBaMaxIter;
// keyframes whose LDS slots fit k_landmark_solve: 448 * 33 * 8 B + kLmBlock * (9 * 8 + 4) B =
// 157,184 B of gfx950's 160 KB per workgroup
constexpr int kMaxKfLds = kBaMaxKfLds;
constexpr int kMaxSplit = kBaMaxSplit;    // pose-stage workgroups per keyframe
constexpr int kCombine = 6;      // (keyframe, term) pairs per thread per combine pass
constexpr int kLmBlock = kBaLmBlock;      // k_landmark_solve: threads = max observations = max landmarks
static_assert(kLmBlock >= kMaxKfLds, "k_landmark_solve solves one keyframe per thread");
static_assert((size_t)kMaxKfLds * kLdsStride * sizeof(double) + (size_t)kLmBlock * (9 * sizeof(double) + sizeof(int)) <=
                  160 * 1024, "k_landmark_solve LDS exceeds gfx950's 160 KB per workgroup");

VX_KT_TABLE();

// (BAState and BAArgs: ba_plan.hpp)

// A lean plan's counts from the device (the launch grid is a capacity bound; surplus workgroups of
// the landmark stage exit); false when nothing runs (no optimisable landmark, local_ba.cpp:106-108)
__device__ __forceinline__ bool dyn_counts(BAArgs& a) {
    if (!a.dyn) return true;
    if (a.dyn[kDynStatus]) return false;
    a.n_opt = a.dyn[kDynNOpt];
    a.n_lm = a.dyn[kDynNLm];
    return true;
}


// Iteration `it` reads the poses of iteration it-1 (the initial poses at it == 0) and writes the
// other buffer, so no launch ever reads a pose another workgroup of the same launch writes.  The
// landmarks [n_opt, n_lm) are never optimised (other shards' landmarks) and always read initial.
__device__ __forceinline__ const double* pose_in(const BAArgs& a, int it) {
    return it == 0 ? a.kf_pose0 : a.kf_pose + (long long)(it & 1) * a.n_kf * 8;
}
__device__ __forceinline__ double* pose_out(const BAArgs& a, int it) {
    return a.kf_pose + (long long)((it + 1) & 1) * a.n_kf * 8;
}
__device__ __forceinline__ const double* lm_in(const BAArgs& a, int it, int s) {
    return (it == 0 || s >= a.n_opt ? a.lm_pos0 : a.lm_pos) + 4 * (long long)s;
}


// Pose step of one keyframe from its summed terms S (local_ba.cpp:163-173): skipped below
// min_pose_observations or without a camera; T updated in place, R = its rotation (:173, :220).
// kFew: the kernels of plans with min_pose_observations < 3 (k_landmark_solve, k_pose_solve_g; such
// plans do not take the fused layout, fused_eligible).  A keyframe with fewer than three observations
// has a J^T J that lacks two ranks or more, and spd6_block_solve returns noise where the reference's
// LDLT steps: those lanes solve by ldlt6_packed_solve.  The wave-uniform vote keeps the rare solve a
// real branch (see se3_left_update).  The fused kernels keep the block solve alone: k_ba_win sits at
// its scalar-register limit and the 1024-thread k_ba_iter at its 128 vector registers, and the branch
// cost them 3 % and 17 % of a C3 / C4 window.
template <bool kFew = false>
__device__ __forceinline__ void solve_pose(const BAArgs& a, int flags, const double* S, double* T, double* R) {
    const int obs = (int)S[28];
    if (obs >= a.min_pose_obs && (flags & 1)) {
        double U[21], b[6], dx[6];
#pragma unroll
        for (int t = 0; t < 21; ++t) U[t] = S[t];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            U[hidx(r, r)] += 1e-6;
            b[r] = S[21 + r];
        }
        if constexpr (kFew) {
            const bool few = obs < 3;
            if (__ballot(few) != 0ull) {
                if (few)
                    ldlt6_packed_solve(U, b, dx);
                else
                    spd6_block_solve(U, b, dx);
            } else {
                spd6_block_solve(U, b, dx);
            }
        } else {
            spd6_block_solve(U, b, dx);
        }
        bool fin = true;
#pragma unroll
        for (int r = 0; r < 6; ++r) fin = fin && isfinite(dx[r]);
        if (fin) se3_left_update(dx, T);
    }
    rot_from_quat(T, R);
}

// Relative-cost stop rule (local_ba.cpp:240-247) -> active[it + 1].  Iteration 0 starts the run's
// state (last_cost = numeric_limits<double>::max(), local_ba.cpp:110); a stop clears every later
// flag, a continue sets the next one (later ones are rewritten before they are read).
__device__ void stop_rule(const BAArgs& a, int it, double total, int tobs) {
    BAState* s = a.state;
    if (it == 0)
        for (int k = 1; k < 16; ++k) {
            s->cost[k] = 0;
            s->obs[k] = 0;
        }
    if (it < 16) {
        s->cost[it] = total;
        s->obs[it] = tobs;
    }
    s->iterations = it + 1;
    const double last = it == 0 ? 1.7976931348623157e308 : s->last_cost;
    const bool stop = tobs == 0 || fabs(last - total) < 1e-6 * last;
    if (!stop) s->last_cost = total;
    if (!stop && it + 1 < a.max_iter)
        s->active[it + 1] = 1;
    else
        for (int k = it + 1; k <= a.max_iter; ++k) s->active[k] = 0;
}

// Ordered (fixed-tree) pose-stage totals over the keyframes; the calling wave must be complete.
__device__ void totals_and_stop(const BAArgs& a, int it, int lane) {
    double total = 0.0;
    int tobs = 0;
    for (int j = lane; j < a.n_kf; j += 64) {
        total += a.kf_cost[2 * j];
        tobs += (int)a.kf_cost[2 * j + 1];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        total += __shfl_xor(total, o, 64);
        tobs += __shfl_xor(tobs, o, 64);
    }
    if (lane == 0) stop_rule(a, it, total, tobs);
}

// Only for max_iterations == 0 (nothing runs): the result is the initial state.  Iteration 0 of
// the kernels below reads the initial arrays directly, so a normal run has no reset launch.
__global__ void k_ba_reset(BAArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.n_kf * 8) a.kf_pose[i] = a.kf_pose0[i];
    if (i < a.n_lm * 4) a.lm_pos[i] = a.lm_pos0[i];
    if (i == 0) {
        BAState* s = a.state;
        for (int k = 0; k <= kMaxIter; ++k) s->active[k] = 0;
        s->iterations = 0;
        for (int k = 0; k < 16; ++k) { s->cost[k] = 0; s->obs[k] = 0; }
    }
}

__device__ __forceinline__ int mbcnt_lo_hi(unsigned long long m) {  // lanes below this one in m
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// Camera-frame point of pose (R, t) (T_cw * p, projection.h:16): R p + t as three FMA chains (the
// rotation matrix of the pose's quaternion, Eigen toRotationMatrix, instead of Eigen's quaternion
// _transformVector: the same map up to rounding, a third of the dependent depth).
__device__ __forceinline__ D3 rt_apply(const double* R, const double* t, D3 p) {
    return {fma(R[2], p.z, fma(R[1], p.y, fma(R[0], p.x, t[0]))), fma(R[5], p.z, fma(R[4], p.y, fma(R[3], p.x, t[1]))),
            fma(R[8], p.z, fma(R[7], p.y, fma(R[6], p.x, t[2])))};
}

// One pose-stage observation (local_ba.cpp:131-159) against pose T (rotation R) / intrinsics C,
// added to the 29 running terms v (21 H upper, 6 b, cost, count): projection with the z > 1e-6
// check, the gate, the Huber weight and the 2x6 PoseJacobian.  The gate and the Huber switch compare
// |e|^2 with max_reproj_error^2 / huber_delta^2, so 1 / |e| (v_rsq) is only evaluated for
// observations beyond huber_delta; |e| > max_err <=> |e|^2 > max_err^2 except within one rounding of
// the boundary.  tests/test_gpu_ba_step.py places residuals exactly on the gate (kept, as by the
// reference) and 2^-20 beside it in every kernel variant, and nothing with 0 < ||e|^2 - max_err^2| <
// 2^-40; the !kFma form compares |e|^2 rsq(|e|^2) with max_err, within 20 ulp of the
// same boundary.
template <bool kFma = true>
__device__ __forceinline__ void pose_obs_accum(const BAArgs& a, const double* T, const double* R, const double* C,
                                               D3 Pw, double2 uv, double* v, bool valid = true) {
    // kFma: branch-free — a rejected observation (invalid lane, behind the camera, beyond the gate)
    // gets weight 0 with finite stand-ins (z = 1), so its terms are exactly +0.0 and the count is not
    // raised (early returns made the running terms a control-flow merge: 27 register moves per
    // observation in the pose-stage loop)
    const double fx = C[0], fy = C[1];
    if constexpr (!kFma) {
        // the round-1 form with early returns, the quaternion rotation, |e| by v_rsq and products
        // then sums: fewer live registers (the 1024-thread kernel's 128-VGPR budget)
        if (!valid) return;
        const D3 pc = se3_apply(T, Pw);
        if (!(pc.z > 1e-6)) return;
        const double inv_z = frcp(pc.z);
        const double x = pc.x * inv_z, y = pc.y * inv_z;
        const double e0 = uv.x - (fx * x + C[2]);
        const double e1 = uv.y - (fy * y + C[3]);
        const double e2 = e0 * e0 + e1 * e1;
        const double re = e2 > 0.0 ? frsq(e2) : 0.0;
        const double en = e2 * re;
        if (en > a.max_err) return;
        const double w = en <= a.huber ? 1.0 : a.huber * re;
        const double jp0 = fx * inv_z, jp2 = -jp0 * x, jp4 = fy * inv_z, jp5 = -jp4 * y;
        const double J0[6] = {jp0, 0.0, jp2, jp2 * pc.y, fma(jp0, pc.z, -jp2 * pc.x), -jp0 * pc.y};
        const double J1[6] = {0.0, jp4, jp5, fma(jp5, pc.y, -jp4 * pc.z), -jp5 * pc.x, jp4 * pc.x};
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = r; c < 6; ++c) {
                const bool u0 = r != 1 && c != 1, u1 = r != 0 && c != 0;  // compile-time after unroll
                const double t0 = u0 ? (w * J0[r]) * J0[c] : 0.0;
                const double t1 = u1 ? (w * J1[r]) * J1[c] : 0.0;
                v[hidx(r, c)] += (u0 && u1) ? t0 + t1 : (u0 ? t0 : t1);
            }
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            const double g = r == 0 ? J0[0] * e0 : (r == 1 ? J1[1] * e1 : J0[r] * e0 + J1[r] * e1);
            v[21 + r] -= w * g;
        }
        v[27] += w * e2;
        v[28] += 1.0;
        return;
    }
    const D3 pc = rt_apply(R, T + 4, Pw);
    const bool front = pc.z > 1e-6;
    const double inv_z = frcp(front ? pc.z : 1.0);
    const double x = pc.x * inv_z, y = pc.y * inv_z;
    const double e0 = uv.x - (fx * x + C[2]);
    const double e1 = uv.y - (fy * y + C[3]);
    const double e2 = e0 * e0 + e1 * e1;
    const bool ok = valid && front && !(e2 > a.max_err2);
    const double w = ok ? (e2 > a.huber2 ? a.huber * frsq(e2) : 1.0) : 0.0;
    const double zz = front ? pc.z : 1.0, xx = front ? pc.x : 0.0, yy = front ? pc.y : 0.0;
    // J = Jp * [I | -hat(pc)] (local_ba.cpp:15-33) with Jp = [[jp0, 0, jp2], [0, jp4, jp5]],
    // written out without its structural zeros (J0[1] = J1[0] = 0)
    const double jp0 = fx * inv_z, jp2 = -jp0 * x, jp4 = fy * inv_z, jp5 = -jp4 * y;
    const double J0[6] = {jp0, 0.0, jp2, jp2 * yy, fma(jp0, zz, -jp2 * xx), -jp0 * yy};
    const double J1[6] = {0.0, jp4, jp5, fma(jp5, yy, -jp4 * zz), -jp5 * xx, jp4 * xx};
    // w J^T J, -w J^T e and w |e|^2 accumulated as FMA chains (the FP64 issue rate bounds this loop,
    // ~2 FMAs per term instead of 2 products and 2 sums)
    double wJ0[6], wJ1[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        wJ0[r] = w * J0[r];
        wJ1[r] = w * J1[r];
    }
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c) {
            const bool u0 = r != 1 && c != 1, u1 = r != 0 && c != 0;  // compile-time after unroll
            double acc = v[hidx(r, c)];
            if (u0) acc = fma(wJ0[r], J0[c], acc);
            if (u1) acc = fma(wJ1[r], J1[c], acc);
            v[hidx(r, c)] = acc;
        }
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        double acc = v[21 + r];
        if (r != 1) acc = fma(-wJ0[r], e0, acc);
        if (r != 0) acc = fma(-wJ1[r], e1, acc);
        v[21 + r] = acc;
    }
    v[27] = fma(w, e2, v[27]);
    v[28] += ok ? 1.0 : 0.0;
}

// Pose stage (local_ba.cpp:116-161): n_split workgroups per keyframe, each over a contiguous
// slice of the keyframe's observations.  Each thread accumulates the 29 terms of its observations
// (strided) in registers; a fixed-order wave butterfly + LDS tree reduces them into the slice's
// partial block kf_part[k * n_split + slice].  Partials are summed later in slice order, so the
// result is deterministic (and identical on every rank after the sharded all-reduce).
__global__ __launch_bounds__(kPoseBlock) void k_pose_kf(BAArgs a0, int it) {
    BAArgs a = a0;
    if (!dyn_counts(a)) return;
    if (it > 0 && !a.state->active[it]) return;
    __shared__ double red[kPoseBlock / 64][kNTerms];
    VX_KT(0);
    const int k = blockIdx.x / a.n_split, slice = blockIdx.x - k * a.n_split;
    const int p0 = a.kf_obs_ptr[k], p1 = a.kf_obs_ptr[k + 1];
    const int len = (p1 - p0 + a.n_split - 1) / a.n_split;
    const int i0 = p0 + slice * len, i1 = min(p1, i0 + len);
    // the thread's first observation and its landmark are requested before the pose, so the
    // dependent gather overlaps the pose / intrinsics loads
    const int ifirst = i0 + (int)threadIdx.x;
    D3 P0{0, 0, 0};
    double2 uv0 = make_double2(0.0, 0.0);
    if (ifirst < i1) {
        uv0 = a.pobs_uv[ifirst];
        const double* P = lm_in(a, it, a.pobs_lm[ifirst]);
        P0 = {P[0], P[1], P[2]};
    }
    const double* Tin = pose_in(a, it);
    double T[8], C[4], R[9];
#pragma unroll
    for (int j = 0; j < 8; ++j) T[j] = Tin[8 * k + j];
#pragma unroll
    for (int j = 0; j < 4; ++j) C[j] = a.kf_intr[4 * k + j];
    rot_from_quat(T, R);
    VX_KT(1);
    double v[kNTerms];
#pragma unroll
    for (int t = 0; t < kNTerms; ++t) v[t] = 0.0;
    for (int i = ifirst; i < i1; i += kPoseBlock) {
        D3 Pw = P0;
        double2 uv = uv0;
        if (i != ifirst) {
            uv = a.pobs_uv[i];
            const double* P = lm_in(a, it, a.pobs_lm[i]);
            Pw = {P[0], P[1], P[2]};
        }
        pose_obs_accum(a, T, R, C, Pw, uv, v);
    }
    VX_KT(2);
    // wave reduction of the 29 terms (halving butterfly, wave_sum32)
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double r[kStride];
#pragma unroll
    for (int t = 0; t < kStride; ++t) r[t] = t < kNTerms ? v[t] : 0.0;
    const double tot = wave_sum32(r);
    VX_KT(3);
    if ((lane & 1) == 0 && (lane >> 1) < kNTerms) red[wv][lane >> 1] = tot;
    __syncthreads();
    VX_KT(4);
    if (threadIdx.x < kStride) {
        double s = 0.0;
        if (threadIdx.x < kNTerms) {
            s = red[0][threadIdx.x];
#pragma unroll
            for (int w2 = 1; w2 < kPoseBlock / 64; ++w2) s += red[w2][threadIdx.x];
        }
        a.kf_part[(long long)blockIdx.x * kStride + threadIdx.x] = s;
    }
    VX_KT(5);
}

// Sum of keyframe k's slice partials for term t, in slice order (absent slices add +0.0).
__device__ __forceinline__ double combine_term(const BAArgs& a, int k, int t) {
    const double* src = a.kf_part + (long long)k * a.n_split * kStride + t;
    double v[kMaxSplit];
#pragma unroll
    for (int c = 0; c < kMaxSplit; ++c) v[c] = c < a.n_split ? src[c * kStride] : 0.0;
    double s = v[0];
#pragma unroll
    for (int c = 1; c < kMaxSplit; ++c) s += v[c];
    return s;
}

// The 9 normal-equation terms {H00 H01 H02 H11 H12 H22 b0 b1 b2} of one landmark observation
// (local_ba.cpp:206-224) against keyframe k of tables T/R/C (strides in doubles), branch-free:
// returns false for a gated-out observation (behind the camera or beyond max_reproj_error),
// whose terms are then exactly +0.0.
template <bool kFma = true>
__device__ __forceinline__ bool obs_terms(const BAArgs& a, D3 P, int k, double2 uv, const double* T0, int tst,
                                          const double* R0, int rst, const double* C0, int cst, double* h) {
    const double* T = T0 + (long long)tst * k;
    const double* C = C0 + (long long)cst * k;
    const double* R = R0 + (long long)rst * k;
    const D3 pc = kFma ? rt_apply(R, T + 4, P) : se3_apply(T, P);
    const bool front = pc.z > 1e-6;
    const double inv_z = frcp(pc.z);
    const double x = pc.x * inv_z, y = pc.y * inv_z;
    const double fx = C[0], fy = C[1];
    const double e0 = uv.x - (fx * x + C[2]);
    const double e1 = uv.y - (fy * y + C[3]);
    const double e2 = e0 * e0 + e1 * e1;
    const bool ok = front && !(e2 > a.max_err2);  // (squared gate, see pose_obs_accum)
    double w = 1.0;
    if (e2 > a.huber2) w = a.huber * frsq(e2);
    const double jp0 = fx * inv_z, jp2 = -jp0 * x, jp4 = fy * inv_z, jp5 = -jp4 * y;
    // J = Jp * R with Jp's structural zeros dropped (local_ba.cpp:219-221); the 9 terms as FMAs with
    // w folded into one factor (a gated-out observation gets w = 0: its terms are exactly +0.0 as
    // long as J and e are finite, and they are selected to 0 below regardless)
    if constexpr (!kFma) {
        double J0[3], J1[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            J0[c] = jp0 * R[c] + jp2 * R[6 + c];
            J1[c] = jp4 * R[3 + c] + jp5 * R[6 + c];
        }
        h[0] = ok ? (w * J0[0]) * J0[0] + (w * J1[0]) * J1[0] : 0.0;
        h[1] = ok ? (w * J0[0]) * J0[1] + (w * J1[0]) * J1[1] : 0.0;
        h[2] = ok ? (w * J0[0]) * J0[2] + (w * J1[0]) * J1[2] : 0.0;
        h[3] = ok ? (w * J0[1]) * J0[1] + (w * J1[1]) * J1[1] : 0.0;
        h[4] = ok ? (w * J0[1]) * J0[2] + (w * J1[1]) * J1[2] : 0.0;
        h[5] = ok ? (w * J0[2]) * J0[2] + (w * J1[2]) * J1[2] : 0.0;
        h[6] = ok ? w * ((-J0[0]) * e0 + (-J1[0]) * e1) : 0.0;
        h[7] = ok ? w * ((-J0[1]) * e0 + (-J1[1]) * e1) : 0.0;
        h[8] = ok ? w * ((-J0[2]) * e0 + (-J1[2]) * e1) : 0.0;
        return ok;
    }
    double J0[3], J1[3], wJ0[3], wJ1[3];
    const double wv = ok ? w : 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        J0[c] = fma(jp0, R[c], jp2 * R[6 + c]);
        J1[c] = fma(jp4, R[3 + c], jp5 * R[6 + c]);
        wJ0[c] = wv * J0[c];
        wJ1[c] = wv * J1[c];
    }
    h[0] = fma(wJ0[0], J0[0], wJ1[0] * J1[0]);
    h[1] = fma(wJ0[0], J0[1], wJ1[0] * J1[1]);
    h[2] = fma(wJ0[0], J0[2], wJ1[0] * J1[2]);
    h[3] = fma(wJ0[1], J0[1], wJ1[1] * J1[1]);
    h[4] = fma(wJ0[1], J0[2], wJ1[1] * J1[2]);
    h[5] = fma(wJ0[2], J0[2], wJ1[2] * J1[2]);
    h[6] = fma(-wJ0[0], e0, -wJ1[0] * e1);
    h[7] = fma(-wJ0[1], e0, -wJ1[1] * e1);
    h[8] = fma(-wJ0[2], e0, -wJ1[2] * e1);
#pragma unroll
    for (int j = 0; j < 9; ++j) h[j] = ok ? h[j] : 0.0;
    return ok;
}

// Landmark update from its summed terms (local_ba.cpp:228-237): skipped below min_point_obs or
// for a non-finite step; the position is written either way (iteration 0 reads lm_pos0).
__device__ __forceinline__ D3 lm_update(const BAArgs& a, int l, D3 P, const double* h, int obs) {
    D3 out = P;
    if (obs >= a.min_point_obs) {
        double H[9] = {h[0] + 1e-6, h[1], h[2], h[1], h[3] + 1e-6, h[4], h[2], h[4], h[5] + 1e-6};
        const double b[3] = {h[6], h[7], h[8]};
        double dp[3];
        ldlt_spd_solve<3>(H, b, dp);
        if (isfinite(dp[0]) && isfinite(dp[1]) && isfinite(dp[2])) out = {P.x + dp[0], P.y + dp[1], P.z + dp[2]};
    }
    double* Pp = a.lm_pos + 4 * l;
    Pp[0] = out.x;
    Pp[1] = out.y;
    Pp[2] = out.z;
    return out;
}

// Pose solve of every window keyframe (redundantly in each workgroup) + landmark stage, one launch.
// Workgroup b covers the whole landmarks [lm_blk[b], lm_blk[b+1]) (at most kLmBlock landmarks
// and kLmBlock observations, packed on the host).  Thread t projects observation o0 + t and
// leaves its 9 terms in LDS; the thread owning landmark l0 + t then sums its observations' terms
// in CSR order (the order of the per-landmark loop, local_ba.cpp:186) and solves the 3x3.
// Every load of the landmark stage is issued first, so it lands during the combine and solve.
// LDS: one kLdsStride-double slot per keyframe (combined normal equations S, then T 8 | R 9 | C 4) and
// 9 x kLmBlock observation terms.
__global__ __launch_bounds__(kLmBlock) void k_landmark_solve(BAArgs a0, int it) {
    BAArgs a = a0;
    if (!dyn_counts(a) || (a.dyn && (int)blockIdx.x >= a.dyn[kDynBlocks])) return;
    if (it > 0 && !a.state->active[it]) return;
    extern __shared__ __attribute__((aligned(16))) double kf_lds[];
    double* terms = kf_lds + (long long)a.n_kf * kLdsStride;  // [9][kLmBlock]
    const int tid = threadIdx.x;
    VX_KT(8);
    const int2 b0 = reinterpret_cast<const int2*>(a.lm_blk)[blockIdx.x];
    const int2 b1 = reinterpret_cast<const int2*>(a.lm_blk)[blockIdx.x + 1];
    const int l0 = b0.x, l1 = b1.x, ob0 = b0.y, ob1 = b1.y;
    // this thread's observation ...
    const int o = ob0 + tid;
    const bool has_o = o < ob1;
    const int ol = has_o ? a.lobs_lm[o] : l0;
    const int ok_kf = has_o ? a.lobs_kf[o] : 0;
    const double2 ouv = has_o ? a.lobs_uv[o] : make_double2(1e300, 1e300);
    const double* Po = lm_in(a, it, ol);
    const D3 PO{Po[0], Po[1], Po[2]};
    // ... and the landmark it owns
    const int l = l0 + tid;
    const bool own = l < l1;
    const int r0 = own ? a.lobs_ptr[l] - ob0 : 0, r1 = own ? a.lobs_ptr[l + 1] - ob0 : 0;
    const double* Pl = lm_in(a, it, own ? l : l0);
    const D3 PL{Pl[0], Pl[1], Pl[2]};
    // ... and the keyframe it solves (pose of the previous iteration, intrinsics, flags): their
    // load latency also passes during the combine instead of after it
    double kT[8] = {0, 0, 0, 0, 0, 0, 0, 0}, kC[4] = {0, 0, 0, 0};
    int kflg = 0;
    if (tid < a.n_kf) {
        const double* Tin = pose_in(a, it);
#pragma unroll
        for (int j = 0; j < 8; ++j) kT[j] = Tin[8 * tid + j];
#pragma unroll
        for (int j = 0; j < 4; ++j) kC[j] = a.kf_intr[4 * tid + j];
        kflg = a.kf_flags[tid];
    }
    VX_KT(9);
    // slice partials -> S: kCombine (keyframe, term) pairs per thread and pass, all their slice
    // loads issued together
    {
        const int ne = a.n_kf * kNTerms;
        for (int e0 = tid; e0 < ne; e0 += kCombine * blockDim.x) {
            double v[kCombine][kMaxSplit];
#pragma unroll
            for (int q = 0; q < kCombine; ++q) {
                const int e = e0 + q * blockDim.x;
                const int k = e / kNTerms, t = e - k * kNTerms;
                const double* src = a.kf_part + (long long)k * a.n_split * kStride + t;
#pragma unroll
                for (int c = 0; c < kMaxSplit; ++c) v[q][c] = (e < ne && c < a.n_split) ? src[c * kStride] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < kCombine; ++q) {
                const int e = e0 + q * blockDim.x;
                if (e >= ne) continue;
                const int k = e / kNTerms, t = e - k * kNTerms;
                double s = v[q][0];
#pragma unroll
                for (int c = 1; c < kMaxSplit; ++c) s += v[q][c];
                kf_lds[k * kLdsStride + t] = s;
            }
        }
    }
    __syncthreads();
    VX_KT(10);
    double* Tout = pose_out(a, it);
    if (tid < a.n_kf) {  // kLmBlock >= kMaxKfLds: one keyframe per thread at most
        const int k = tid;
        double* slot = kf_lds + k * kLdsStride;
        double S[kNTerms];
#pragma unroll
        for (int t = 0; t < kNTerms; ++t) S[t] = slot[t];
        double T[8], R[9];
#pragma unroll
        for (int j = 0; j < 8; ++j) T[j] = kT[j];
        solve_pose<true>(a, kflg, S, T, R);
#pragma unroll
        for (int j = 0; j < 8; ++j) slot[j] = T[j];
#pragma unroll
        for (int j = 0; j < 9; ++j) slot[8 + j] = R[j];
#pragma unroll
        for (int j = 0; j < 4; ++j) slot[17 + j] = kC[j];
        if (blockIdx.x == 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) Tout[8 * k + j] = T[j];
#pragma unroll
            for (int j = 0; j < 9; ++j) a.kf_rot[9 * k + j] = R[j];
            a.kf_cost[2 * k] = S[27];
            a.kf_cost[2 * k + 1] = S[28];
        }
    }
    __syncthreads();  // also makes block 0's kf_cost stores visible inside block 0
    VX_KT(11);
    if (blockIdx.x == 0 && tid < 64) totals_and_stop(a, it, tid);
    {
        double h[9];
        const bool ok = obs_terms(a, PO, ok_kf, ouv, kf_lds, kLdsStride, kf_lds + 8, kLdsStride, kf_lds + 17,
                                  kLdsStride, h);
#pragma unroll
        for (int j = 0; j < 9; ++j) terms[j * kLmBlock + tid] = h[j];
        reinterpret_cast<int*>(terms + 9 * kLmBlock)[tid] = (has_o && ok) ? 1 : 0;  // counted observation
    }
    __syncthreads();
    VX_KT(13);
    if (own) {
        double h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        int obs = 0;
        const int* okf = reinterpret_cast<const int*>(terms + 9 * kLmBlock);
        for (int r = r0; r < r1; ++r) {
#pragma unroll
            for (int j = 0; j < 9; ++j) h[j] += terms[j * kLmBlock + r];
            obs += okf[r];
        }
        lm_update(a, l, PL, h, obs);
    }
    VX_KT(12);
}

// Large-window fallback (n_kf > kMaxKfLds): one thread per keyframe solves into global memory...
__global__ __launch_bounds__(256) void k_pose_solve_g(BAArgs a, int it) {
    if (it > 0 && !a.state->active[it]) return;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.n_kf) return;
    double S[kNTerms];
#pragma unroll
    for (int t = 0; t < kNTerms; ++t) S[t] = combine_term(a, k, t);
    const double* Tin = pose_in(a, it);
    double* Tout = pose_out(a, it);
    double T[8], R[9];
#pragma unroll
    for (int j = 0; j < 8; ++j) T[j] = Tin[8 * k + j];
    solve_pose<true>(a, a.kf_flags[k], S, T, R);
#pragma unroll
    for (int j = 0; j < 8; ++j) Tout[8 * k + j] = T[j];
#pragma unroll
    for (int j = 0; j < 9; ++j) a.kf_rot[9 * k + j] = R[j];
    a.kf_cost[2 * k] = S[27];
    a.kf_cost[2 * k + 1] = S[28];
}

// ... and the landmark stage reads the poses from global memory, one thread per landmark; wave 0
// of block 0 evaluates the stop rule (active[it + 1] is read by no block of this launch).
__global__ __launch_bounds__(256) void k_landmark(BAArgs a, int it) {
    if (it > 0 && !a.state->active[it]) return;
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < 64) totals_and_stop(a, it, threadIdx.x);
    if (l >= a.n_opt) return;
    const double* Pin = lm_in(a, it, l);
    const D3 P{Pin[0], Pin[1], Pin[2]};
    double h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, t[9];
    int obs = 0;
    const double* T0 = pose_out(a, it);
    for (int o = a.lobs_ptr[l]; o < a.lobs_ptr[l + 1]; ++o) {
        obs += obs_terms(a, P, a.lobs_kf[o], a.lobs_uv[o], T0, 8, a.kf_rot, 9, a.kf_intr, 4, t) ? 1 : 0;
#pragma unroll
        for (int j = 0; j < 9; ++j) h[j] += t[j];
    }
    lm_update(a, l, P, h, obs);
}

}  // namespace
}  // namespace vx
