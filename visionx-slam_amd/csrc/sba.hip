// sba.hip — Schur-complement joint bundle adjustment on gfx950 (vx_sba_*).
//
// Not a reference entry point: the reference's LocalBA (core/backend/local_ba.cpp:66-249) alternates
// per-keyframe and per-landmark steps (ba.hip reproduces that bit-for-bit semantics).  BASELINE.json's
// north_star asks for the Schur-complement marginalisation of the landmark blocks into the dense
// 6N x 6N pose system with a dense (MFMA) pose solve; SURVEY.md §8f rank 4.  This solver keeps the
// reference's window / landmark set (local_ba.cpp:42-108), observation set (:126-138), residual,
// Jacobians, Huber weight and gates (:15-40, projection.h:11-31) and the 1e-6 regulariser, and
// solves ONE damped Gauss-Newton system per iteration (b = +J^T W e, Marquardt damping, accept /
// reject on the Huber cost, oldest `fixed_keyframes` held fixed).  CPU restatement:
// oracle/sba_oracle.cpp.  Per iteration (all launches early-exit once the stop rule fired):
//
//   k_sba_lm     one thread per observation of an optimised landmark, whole landmarks per
//                workgroup: residual, gates, weight, J_T (2x6) and J_p (2x3); the landmark's owner
//                thread sums V = sum w J_p^T J_p and g_p = sum w J_p^T e in CSR order, damps and
//                inverts V (3x3 adjugate); every thread then writes W_o = w J_T^T J_p and
//                Y_o = W_o V^-1 (6x3 each) for the Schur products.
//   k_sba_blocks one workgroup per nonzero 6x6 block (i, j), i >= j, of the reduced system:
//                diagonal blocks add every observation's w J_T^T J_T, g_T, Huber cost and count,
//                minus Y_o g_p; every block subtracts sum Y_o1 W_o2^T over the co-observation
//                pairs the host listed for it (fixed order: deterministic).  Blocks of a
//                connected component of the covisibility graph land in that component's dense
//                matrix; all blocks of a sharded run are all-reduced (one ncclAllReduce).
//   k_sba_solve  one workgroup (16 waves) per connected component: Levenberg-Marquardt decision,
//                then a right-looking tiled Cholesky of the damped component matrix with the
//                right-hand side as an extra tile row (forward substitution for free): per 16 x 16
//                diagonal tile, one wave factors it and forms L_kk^-1 from registers
//                (v_readlane broadcasts); the panel L_ik = A_ik L_kk^-T and the trailing update
//                A_ij -= L_ik L_jk^T are v_mfma_f64_16x16x4 tiles (panel staged in LDS); then the
//                blocked back-substitution L^T x = y.  ($VX_SBA_FACTOR=single; the default spreads the
//                same factorisation over G workgroups per component, one launch per tile step:
//                k_sba_fac_begin / k_sba_fac_step / k_sba_backsub below.)
//   k_sba_update landmark back-substitution dp = V^-1 (g_p - sum W_o^T dx) and T <- exp(dx) T into
//                the trial buffers.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <unordered_map>
#include <atomic>
#include <thread>
#include <vector>

#include "vx_internal.hpp"
#include "vx_ktrace.hpp"
#include "ba_common.hpp"
#include "sba_plan.hpp"
#include "dmap.hpp"
#include "vx_copy.hpp"

namespace vx {
namespace {

using namespace vx::ba;

constexpr int kSbaMaxIter = 64;
constexpr int kLmThreads = kSbaLmThreads;  // k_sba_lm: max observations (and landmarks) per workgroup
constexpr int kBlkThreads = 256;    // k_sba_blocks
constexpr int kSolveThreads = 256;  // k_sba_solve: 4 waves, one per SIMD (512 registers each: no spills)
constexpr int kSolveWaves = kSolveThreads / 64;
constexpr int kUpdThreads = 256;
constexpr int kMaxCompKf = 448;     // keyframes of one connected component (dense n <= 2688)
constexpr int kWy = 36;             // doubles per optimised observation: W (6x3) | Y (6x3)
constexpr int kLmSys = 12;          // doubles per optimised landmark: V^-1 (6) | g_p (3) | pad
constexpr int kBlkTerms = 50;       // 36 block + 6 rhs + 6 D + cost + count
constexpr int kPanelStride = 256;   // doubles per LDS panel tile (operand order)
// smallest Marquardt damping after accepted steps (keeps gauge directions regularised)
constexpr double kLambdaMin = 1e-6;

typedef double d4 __attribute__((ext_vector_type(4)));

VX_KT_TABLE();

// Levenberg-Marquardt variables; k_sba_solve of iteration it reads lm[it & 1] and writes
// lm[(it + 1) & 1] (so no workgroup of the launch reads what another writes).
struct LMVars {
    int sel;          // buffer with the best state: -1 = initial arrays, 0 / 1
    int eval_trial;   // the next assembly evaluates the trial buffer
    int do_solve;     // k_sba_update of this iteration applies a step
    int accepted;
    double lambda;    // damping of the next assembly
    double best_cost;
};

struct SBAState {
    int active[kSbaMaxIter + 1];
    int fail[kSbaMaxIter];       // a component's Cholesky hit a non-positive pivot
    LMVars lm[2];
    int iterations;
    int pad;
    double initial_cost;
    double cost[16];
    int obs[16];
    int step[16];
};

struct SBAArgs {
    int nk, n_opt, n_lm, n_oo, n_obs;
    int max_iter, min_point_obs;
    double huber, max_err, lambda0, rel_tol;
    double rho_gate;        // Huber cost of an observation at the gate (max_reproj_error)
    const double* pose0;    // nk x 8
    double* pose;           // 2 x nk x 8
    const double* intr;     // nk x 4
    const int* kf_flags;    // bit0 camera, bit1 fixed
    const int* kf_comp;     // component of a free keyframe (-1 fixed)
    const int* kf_local;    // keyframe index inside its component
    const double* lm0;      // n_lm x 4
    double* lm;             // 2 x n_opt x 4
    const double2* obs_uv;
    const int* obs_kf;
    const int* obs_lm;
    const int* lm_ptr;      // n_opt + 1
    const int* lm_blk;      // k_sba_lm workgroup -> first landmark
    const int* kf_ptr;      // nk + 1 into kf_obs
    const int* kf_obs;
    const int2* blk_ij;
    const int* blk_ptr;
    const int2* pairs;
    const int* comp_kf_ptr; // component -> keyframe list (comp_kf)
    const int* comp_kf;
    const long long* comp_off;   // component -> offset of its dense matrix in red (ld = comp_np)
    const long long* comp_loff;  // component -> offset of its factor in L ((np + 16) x np)
    const int* comp_np;
    const int* comp_hdr;    // component -> kHdrN ints (tile program offsets, nt)
    const int* tl;          // tile programs
    double* wy;             // n_oo x kWy
    double* lm_sys;         // n_opt x kLmSys
    int diag_split;         // k_sba_blocks workgroups per diagonal block (D)
    double* bpart;          // D > 1: nk x D x kBlkTerms partial sums of the diagonal blocks
    double* red;            // local: S blocks | rhs (6 nk) | D (6 nk) | kf_cost (2 nk)
    const double* red_sum;  // == red unless sharded
    long long s_total;      // doubles of all component matrices
    double* L;
    double* Linv;           // per component: nt x 256, at the component's L offset
    double* dx;             // 6 nk
    SBAState* st;
    int panel_slots;        // k_sba_solve: LDS panel tiles (a step with more panel tiles reads global)
    const int* fac_steps;   // k_sba_fac_step descriptors (vx_sba_plan::fac_steps), fac_nk per component
    int fac_nk;
    const int* fac_pairs;   // k_sba_fac_pair descriptors (vx_sba_plan::fac_pairs), fac_np per component
    int fac_np;
    const int* fac_blks;    // k_sba_fac_blk descriptors (vx_sba_plan::fac_blks), fac_nb per component
    int fac_nb;
    int bs_np, bs_nt;       // k_sba_backsub's LDS: the largest component's np doubles, nt + 1 pointers
    int n_comp;             // covisibility components (k_sba_update clears their factors' touched tiles)
};

// one launch of the two-column schedule for one component (vx_sba_plan::fac_pairs)
struct FacPair {
    long long loff;
    int l1b, l1e, l2b, l2e, rb, re, p0, p1, q0, q1, nt, c0;
};

// one launch of the multi-workgroup factor for one component (vx_sba_plan::fac_steps)
struct FacStep {
    long long loff;
    int la_beg, split, t_end, p0, p1, nt;
};

// one launch of the blocked factor for one component (vx_sba_plan::fac_blks, 16 ints): block t's
// columns [K0, K0 + W) and tile list, block t - 1's columns and tile list (its steps' pattern), the
// trailing tiles block t - 1's steps update beyond block t (entries i << 16 | j << 4 | step mask)
struct FacBlk {
    long long loff;
    int K0, W, bt_beg, bt_end, pb_beg, pb_end, K0p, Wp, tr_beg, tr_end, nt, la_beg, la_end;
};

// ------------------------------------------------------------------------- state selection
__device__ __forceinline__ int trial_idx(int sel) { return sel == 0 ? 1 : 0; }

// Pose / landmark tables the assembly of iteration it evaluates.
__device__ __forceinline__ const double* eval_pose(const SBAArgs& a, int it) {
    if (it == 0) return a.pose0;
    const LMVars& v = a.st->lm[it & 1];
    const int b = v.eval_trial ? trial_idx(v.sel) : v.sel;
    return b < 0 ? a.pose0 : a.pose + (long long)b * a.nk * 8;
}
__device__ __forceinline__ const double* eval_lm(const SBAArgs& a, int it) {
    if (it == 0) return a.lm0;
    const LMVars& v = a.st->lm[it & 1];
    const int b = v.eval_trial ? trial_idx(v.sel) : v.sel;
    return b < 0 ? a.lm0 : a.lm + (long long)b * a.n_opt * 4;
}

// One observation at a state: residual, gates, IRLS weight, Huber cost and the Jacobians.
struct ObsEval {
    bool ok;
    double w, rho, e0, e1;
    double JT0[6], JT1[6];  // d(uv)/d(upsilon, omega), rows u and v (PoseJacobian, local_ba.cpp:26-33)
    double JP0[3], JP1[3];  // d(uv)/dp = Jp R (local_ba.cpp:219-221)
};

__device__ __forceinline__ void eval_obs(const SBAArgs& a, const double* T, const double* C, D3 P, double2 uv,
                                         bool need_jp, ObsEval& o) {
    const D3 pc = se3_apply(T, P);
    const bool front = pc.z > 1e-6;
    const double inv_z = frcp(pc.z);
    const double x = pc.x * inv_z, y = pc.y * inv_z;
    const double fx = C[0], fy = C[1];
    o.e0 = uv.x - (fx * x + C[2]);
    o.e1 = uv.y - (fy * y + C[3]);
    const double e2 = o.e0 * o.e0 + o.e1 * o.e1;
    const double re = e2 > 0.0 ? frsq(e2) : 0.0;
    const double en = e2 * re;
    o.ok = front && !(en > a.max_err);
    const double d = a.huber;
    o.w = en <= d ? 1.0 : d * re;
    o.rho = en <= d ? e2 : 2.0 * d * en - d * d;
    const double jp0 = fx * inv_z, jp2 = -jp0 * x, jp4 = fy * inv_z, jp5 = -jp4 * y;
    o.JT0[0] = jp0; o.JT0[1] = 0.0; o.JT0[2] = jp2;
    o.JT0[3] = jp2 * pc.y; o.JT0[4] = jp0 * pc.z - jp2 * pc.x; o.JT0[5] = -jp0 * pc.y;
    o.JT1[0] = 0.0; o.JT1[1] = jp4; o.JT1[2] = jp5;
    o.JT1[3] = jp5 * pc.y - jp4 * pc.z; o.JT1[4] = -jp5 * pc.x; o.JT1[5] = jp4 * pc.x;
    if (need_jp) {
        double R[9];
        rot_from_quat(T, R);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            o.JP0[c] = jp0 * R[c] + jp2 * R[6 + c];
            o.JP1[c] = jp4 * R[3 + c] + jp5 * R[6 + c];
        }
    }
}

// Inverse of the symmetric {a b c; b d e; c e f} by its adjugate (the restatement uses the same).
__device__ __forceinline__ void sym3_inverse(const double* V, double* out) {
    const double a = V[0], b = V[1], c = V[2], d = V[3], e = V[4], f = V[5];
    const double A = d * f - e * e, B = c * e - b * f, C = b * e - c * d;
    const double D = a * f - c * c, E = b * c - a * e, F = a * d - b * b;
    const double det = a * A + b * B + c * C;
    const double id = frcp(det);
    out[0] = A * id; out[1] = B * id; out[2] = C * id; out[3] = D * id; out[4] = E * id; out[5] = F * id;
}

// ------------------------------------------------------------------------- k_sba_lm
__global__ __launch_bounds__(kLmThreads) void k_sba_lm(SBAArgs a, int it) {
    if (it > 0 && !a.st->active[it]) return;
    __shared__ double terms[10][kLmThreads];
    __shared__ double vinv[6][kLmThreads];
    const int tid = threadIdx.x;
    const int l0 = a.lm_blk[blockIdx.x], l1 = a.lm_blk[blockIdx.x + 1];
    const int ob0 = a.lm_ptr[l0], ob1 = a.lm_ptr[l1];
    const int o = ob0 + tid;
    const bool has = o < ob1;
    const double* Tb = eval_pose(a, it);
    const double* Pb = eval_lm(a, it);
    const double lambda = it == 0 ? a.lambda0 : a.st->lm[it & 1].lambda;
    ObsEval e;
    int s = l0;
    if (has) {
        const int k = a.obs_kf[o];
        s = a.obs_lm[o];
        const double* P = Pb + 4 * (long long)s;
        double T[8], C[4];
#pragma unroll
        for (int j = 0; j < 8; ++j) T[j] = Tb[8 * k + j];
#pragma unroll
        for (int j = 0; j < 4; ++j) C[j] = a.intr[4 * k + j];
        eval_obs(a, T, C, {P[0], P[1], P[2]}, a.obs_uv[o], true, e);
    } else {
        e.ok = false;
    }
    {
        const double w = e.ok ? e.w : 0.0;
        const double* J0 = e.JP0;
        const double* J1 = e.JP1;
        terms[0][tid] = e.ok ? (w * J0[0]) * J0[0] + (w * J1[0]) * J1[0] : 0.0;
        terms[1][tid] = e.ok ? (w * J0[0]) * J0[1] + (w * J1[0]) * J1[1] : 0.0;
        terms[2][tid] = e.ok ? (w * J0[0]) * J0[2] + (w * J1[0]) * J1[2] : 0.0;
        terms[3][tid] = e.ok ? (w * J0[1]) * J0[1] + (w * J1[1]) * J1[1] : 0.0;
        terms[4][tid] = e.ok ? (w * J0[1]) * J0[2] + (w * J1[1]) * J1[2] : 0.0;
        terms[5][tid] = e.ok ? (w * J0[2]) * J0[2] + (w * J1[2]) * J1[2] : 0.0;
        terms[6][tid] = e.ok ? w * (J0[0] * e.e0 + J1[0] * e.e1) : 0.0;
        terms[7][tid] = e.ok ? w * (J0[1] * e.e0 + J1[1] * e.e1) : 0.0;
        terms[8][tid] = e.ok ? w * (J0[2] * e.e0 + J1[2] * e.e1) : 0.0;
        terms[9][tid] = e.ok ? 1.0 : 0.0;
    }
    __syncthreads();
    const int l = l0 + tid;
    if (l < l1) {
        const int r0 = a.lm_ptr[l] - ob0, r1 = a.lm_ptr[l + 1] - ob0;
        double h[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int r = r0; r < r1; ++r)
#pragma unroll
            for (int j = 0; j < 10; ++j) h[j] += terms[j][r];
        double Vd[6] = {h[0], h[1], h[2], h[3], h[4], h[5]};
        Vd[0] += lambda * h[0] + 1e-6;
        Vd[3] += lambda * h[3] + 1e-6;
        Vd[5] += lambda * h[5] + 1e-6;
        // fewer valid observations than min_point_observations: the landmark is held fixed in
        // this iteration (V^-1 = 0, so no Schur term and dp = 0), as local_ba.cpp:228-229 skips it
        double Vi[6] = {0, 0, 0, 0, 0, 0};
        if (h[9] >= (double)a.min_point_obs) sym3_inverse(Vd, Vi);
        double* out = a.lm_sys + (long long)l * kLmSys;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            vinv[j][tid] = Vi[j];
            out[j] = Vi[j];
        }
        out[6] = h[6];
        out[7] = h[7];
        out[8] = h[8];
    }
    __syncthreads();
    if (!has) return;
    const int ls = s - l0;
    const double Vi[6] = {vinv[0][ls], vinv[1][ls], vinv[2][ls], vinv[3][ls], vinv[4][ls], vinv[5][ls]};
    const double w = e.ok ? e.w : 0.0;
    double W[18], Y[18];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) W[3 * r + c] = e.ok ? w * (e.JT0[r] * e.JP0[c] + e.JT1[r] * e.JP1[c]) : 0.0;
        Y[3 * r + 0] = Vi[0] * W[3 * r] + Vi[1] * W[3 * r + 1] + Vi[2] * W[3 * r + 2];
        Y[3 * r + 1] = Vi[1] * W[3 * r] + Vi[3] * W[3 * r + 1] + Vi[4] * W[3 * r + 2];
        Y[3 * r + 2] = Vi[2] * W[3 * r] + Vi[4] * W[3 * r + 1] + Vi[5] * W[3 * r + 2];
    }
    double2* dst = reinterpret_cast<double2*>(a.wy + (long long)o * kWy);
#pragma unroll
    for (int j = 0; j < 9; ++j) dst[j] = make_double2(W[2 * j], W[2 * j + 1]);
#pragma unroll
    for (int j = 0; j < 9; ++j) dst[9 + j] = make_double2(Y[2 * j], Y[2 * j + 1]);
}

// ------------------------------------------------------------------------- k_sba_blocks
__device__ __forceinline__ void load18(const double* src, double* v) {
    const double2* s2 = reinterpret_cast<const double2*>(src);
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const double2 t = s2[j];
        v[2 * j] = t.x;
        v[2 * j + 1] = t.y;
    }
}

// block b's reduced terms v (thread tid < kBlkTerms holds term tid): the 6x6 block into the
// component matrix, a diagonal block's rhs / D / cost rows
__device__ __forceinline__ void blocks_write(const SBAArgs& a, int i, int j, bool diag, int tid, double v) {
    const int n6 = 6 * a.nk;
    double* rhs = a.red + a.s_total;
    if (tid < 36) {
        const int c = a.kf_comp[i];
        if (c < 0) return;  // a fixed keyframe's block: its row is the identity (k_sba_solve)
        const int np = a.comp_np[c];
        const int li = a.kf_local[i], lj = a.kf_local[j];
        const int r = tid / 6, cc = tid - 6 * r;
        a.red[a.comp_loff[c] + (long long)(6 * li + r) * np + 6 * lj + cc] = v;
    } else if (diag) {
        if (tid < 42) rhs[6 * i + tid - 36] = v;
        else if (tid < 48) rhs[n6 + 6 * i + tid - 42] = v;
        else rhs[2 * n6 + 2 * i + tid - 48] = v;
    }
}

// Workgroups [0, nk D): the diagonal blocks, D per keyframe (workgroup x: keyframe x mod nk, part
// x / nk) — a diagonal block walks all its keyframe's observations (~1300-1700 at C3 / C5) and as
// many self pairs, a chain of dependent loads per 256 of them that set the launch's length; the D
// parts' sums land in bpart and k_sba_blocks_diag adds them in part order.  Then one workgroup per
// off-diagonal block.
__global__ __launch_bounds__(kBlkThreads) void k_sba_blocks(SBAArgs a, int it) {
    if (it > 0 && !a.st->active[it]) return;
    __shared__ double red[kBlkThreads / 64][64];
    const int tid = threadIdx.x, D = a.diag_split, nd = a.nk * D;
    if (blockIdx.x == 0 && tid == 0) a.st->fail[it] = 0;
    const int x = blockIdx.x;
    const int b = x < nd ? x % a.nk : a.nk + (x - nd);
    const int part = x < nd ? x / a.nk : 0, pstride = x < nd ? D * kBlkThreads : kBlkThreads;
    const int2 ij = a.blk_ij[b];
    const int i = ij.x, j = ij.y;
    const bool diag = i == j;
    const bool fixed_i = (a.kf_flags[i] & 2) != 0;
    double acc[kBlkTerms];
#pragma unroll
    for (int t = 0; t < kBlkTerms; ++t) acc[t] = 0.0;
    if (diag) {
        const double* Tb = eval_pose(a, it);
        const double* Pb = eval_lm(a, it);
        double T[8], C[4];
#pragma unroll
        for (int q = 0; q < 8; ++q) T[q] = Tb[8 * i + q];
#pragma unroll
        for (int q = 0; q < 4; ++q) C[q] = a.intr[4 * i + q];
        for (int idx = a.kf_ptr[i] + part * kBlkThreads + tid; idx < a.kf_ptr[i + 1]; idx += pstride) {
            const int o = a.kf_obs[idx];
            const int s = a.obs_lm[o];
            const double* P = (s < a.n_opt ? Pb : a.lm0) + 4 * (long long)s;
            ObsEval e;
            eval_obs(a, T, C, {P[0], P[1], P[2]}, a.obs_uv[o], false, e);
            // a gated observation costs the constant rho(max_reproj_error) (truncated robust cost)
            acc[48] += e.ok ? e.rho : a.rho_gate;
            if (!e.ok) continue;
            acc[49] += 1.0;
            if (fixed_i) continue;
            const double w = e.w;
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                const double wr0 = w * e.JT0[r], wr1 = w * e.JT1[r];
#pragma unroll
                for (int c = 0; c < 6; ++c) acc[6 * r + c] += wr0 * e.JT0[c] + wr1 * e.JT1[c];
                acc[36 + r] += wr0 * e.e0 + wr1 * e.e1;
                acc[42 + r] += wr0 * e.JT0[r] + wr1 * e.JT1[r];
            }
            if (s < a.n_opt) {  // rhs -= Y_o g_p
                double Y[18];
                load18(a.wy + (long long)o * kWy + 18, Y);
                const double* g = a.lm_sys + (long long)s * kLmSys + 6;
                const double g0 = g[0], g1 = g[1], g2 = g[2];
#pragma unroll
                for (int r = 0; r < 6; ++r) acc[36 + r] -= Y[3 * r] * g0 + Y[3 * r + 1] * g1 + Y[3 * r + 2] * g2;
            }
        }
    }
    for (int p = a.blk_ptr[b] + part * kBlkThreads + tid; p < a.blk_ptr[b + 1]; p += pstride) {
        const int2 pr = a.pairs[p];
        double Y[18], W[18];
        load18(a.wy + (long long)pr.x * kWy + 18, Y);
        load18(a.wy + (long long)pr.y * kWy, W);
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = 0; c < 6; ++c)
                acc[6 * r + c] -= Y[3 * r] * W[3 * c] + Y[3 * r + 1] * W[3 * c + 1] + Y[3 * r + 2] * W[3 * c + 2];
    }
    // workgroup reduction: two halving butterflies (terms 0-31, 32-49), then the 4 waves in order
    const int wv = tid >> 6, lane = tid & 63;
    {
        double r[32];
#pragma unroll
        for (int t = 0; t < 32; ++t) r[t] = acc[t];
        const double tot = wave_sum32(r);
        if ((lane & 1) == 0) red[wv][lane >> 1] = tot;
    }
    {
        double r[32];
#pragma unroll
        for (int t = 0; t < 32; ++t) r[t] = t < kBlkTerms - 32 ? acc[32 + t] : 0.0;
        const double tot = wave_sum32(r);
        if ((lane & 1) == 0) red[wv][32 + (lane >> 1)] = tot;
    }
    __syncthreads();
    if (tid >= kBlkTerms) return;
    double v = red[0][tid];
#pragma unroll
    for (int w2 = 1; w2 < kBlkThreads / 64; ++w2) v += red[w2][tid];
    if (diag && D > 1) {
        a.bpart[((long long)i * D + part) * kBlkTerms + tid] = v;
        return;
    }
    blocks_write(a, i, j, diag, tid, v);
}

// D > 1: the diagonal blocks' parts summed in part order (deterministic), then written as above
__global__ __launch_bounds__(64) void k_sba_blocks_diag(SBAArgs a, int it) {
    if (it > 0 && !a.st->active[it]) return;
    const int i = blockIdx.x, tid = threadIdx.x, D = a.diag_split;
    if (tid >= kBlkTerms) return;
    const double* bp = a.bpart + (long long)i * D * kBlkTerms + tid;
    double v = bp[0];
    for (int d = 1; d < D; ++d) v += bp[(long long)d * kBlkTerms];
    blocks_write(a, i, i, true, tid, v);
}

// ------------------------------------------------------------------------- k_sba_solve
__device__ __forceinline__ double rl(double v, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane),
                            __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// Levenberg-Marquardt decision of iteration it (identical in every workgroup): returns the step
// code (2 initial, 1 accepted, 0 rejected, 3 re-assembled after a reject) and the next variables.
__device__ int lm_decide(const SBAArgs& a, int it, double cost, int cnt, LMVars& nx, bool& active_next) {
    LMVars pv;
    if (it == 0) {
        pv.sel = -1;
        pv.eval_trial = 0;
        pv.do_solve = 0;
        pv.accepted = 0;
        pv.lambda = a.lambda0;
        pv.best_cost = cost;
    } else {
        pv = a.st->lm[it & 1];
    }
    nx = pv;
    int step;
    bool stop = false;
    if (it == 0) {
        step = 2;
    } else if (pv.eval_trial) {
        if (cost < pv.best_cost) {
            const double rel = (pv.best_cost - cost) / pv.best_cost;
            nx.sel = trial_idx(pv.sel);
            nx.best_cost = cost;
            nx.lambda = fmax(pv.lambda * 0.1, kLambdaMin);
            nx.accepted = pv.accepted + 1;
            step = 1;
            stop = rel < a.rel_tol;
        } else {
            nx.lambda = pv.lambda * 10.0;
            step = 0;
            stop = nx.lambda > 1e12;
        }
    } else {
        step = 3;
    }
    if (cnt == 0) stop = true;
    const bool last = stop || it + 1 >= a.max_iter;
    nx.do_solve = (!last && step != 0) ? 1 : 0;
    nx.eval_trial = nx.do_solve;
    active_next = !last;
    return step;
}

// Operand-order LDS image of a 16x16 tile: lane l's MFMA operands (row l & 15, columns
// 4 (l >> 4) .. + 3) are 4 consecutive doubles at 4 l: conflict-free 32-byte reads.
__device__ __forceinline__ int opo(int row, int col) { return 4 * (row + 16 * (col >> 2)) + (col & 3); }

// C += s * A B^T over one 16x16 tile pair given as operand-order LDS images.
__device__ __forceinline__ d4 mfma_abt(const double* A, const double* B, d4 c, bool neg) {
    const int lane = threadIdx.x & 63;
    const double4 av = *reinterpret_cast<const double4*>(A + 4 * lane);
    const double4 bv = *reinterpret_cast<const double4*>(B + 4 * lane);
    c = __builtin_amdgcn_mfma_f64_16x16x4f64(neg ? -av.x : av.x, bv.x, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f64_16x16x4f64(neg ? -av.y : av.y, bv.y, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f64_16x16x4f64(neg ? -av.z : av.z, bv.z, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f64_16x16x4f64(neg ? -av.w : av.w, bv.w, c, 0, 0, 0);
    return c;
}

// The same product with both tiles read in operand order straight from the row-major factor in
// global memory (ld = np): for the steps whose panel does not fit the LDS slots.
__device__ __forceinline__ d4 mfma_abt_g(const double* A, const double* B, int ld, d4 c) {
    const int lane = threadIdx.x & 63, r0 = lane >> 4, cl = lane & 15;
    const double4 av = *reinterpret_cast<const double4*>(A + (long long)cl * ld + 4 * r0);
    const double4 bv = *reinterpret_cast<const double4*>(B + (long long)cl * ld + 4 * r0);
    c = __builtin_amdgcn_mfma_f64_16x16x4f64(-av.x, bv.x, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f64_16x16x4f64(-av.y, bv.y, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f64_16x16x4f64(-av.z, bv.z, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f64_16x16x4f64(-av.w, bv.w, c, 0, 0, 0);
    return c;
}

// Accumulator layout of v_mfma_f64_16x16x4: lane l, register r -> row (l >> 4) + 4 r, col l & 15.
__device__ __forceinline__ d4 load_acc(const double* T, int ld) {
    const int lane = threadIdx.x & 63, r0 = lane >> 4, c = lane & 15;
    d4 v;
    v[0] = T[(long long)(r0) * ld + c];
    v[1] = T[(long long)(r0 + 4) * ld + c];
    v[2] = T[(long long)(r0 + 8) * ld + c];
    v[3] = T[(long long)(r0 + 12) * ld + c];
    return v;
}
__device__ __forceinline__ void store_acc(double* T, int ld, d4 v) {
    const int lane = threadIdx.x & 63, r0 = lane >> 4, c = lane & 15;
    T[(long long)(r0) * ld + c] = v[0];
    T[(long long)(r0 + 4) * ld + c] = v[1];
    T[(long long)(r0 + 8) * ld + c] = v[2];
    T[(long long)(r0 + 12) * ld + c] = v[3];
}
__device__ __forceinline__ void store_acc_opo(double* S, d4 v) {
    const int lane = threadIdx.x & 63, r0 = lane >> 4, c = lane & 15;
#pragma unroll
    for (int r = 0; r < 4; ++r) S[opo(r0 + 4 * r, c)] = v[r];
}

// One wave: Cholesky of the symmetric 16x16 tile at A (lower triangle read) and the inverse of its
// factor.  Lane i holds row i in registers.  Per column j the pivot comes from lane j
// (v_readlane), every lane scales its entry and takes the column's other entries from their lanes
// by v_readlane for its rank-1 update — no LDS round trip on the chain, which per column is
// readlane -> rsq (+ Newton) -> mul -> readlane -> fma.
// L^-1 (lane i = column i): the forward substitution's step j needs only column j of L and its
// 1 / L_jj — the same readlanes and the same (uniform) reciprocal square root the factor's column
// j uses — so it runs inside the same loop, its two-op chain beside the factor's (the same
// operations in the same order per lane as a separate substitution after the factor: bitwise the
// same L^-1).  Written as an operand-order LDS image and row-major to Lg.  Returns false on a
// non-positive pivot.  (lcol: unused scratch, kept for the callers' LDS layout.)
// rd(r, c): element (r, c) of the tile, lower triangle read (c <= r)
template <class Rd>
__device__ __forceinline__ bool potrf_inv16_t(Rd rd, double* lds_inv, double* Lg) {
    const int lane = threadIdx.x & 63, i = lane & 15;
    double a[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) a[c] = c <= i ? rd(i, c) : rd(c, i);
    double x[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) x[r] = r == i ? 1.0 : 0.0;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const double d = rl(a[j], j);
        ok = ok && d > 0.0 && d < 1e300;
        const double r = frsq(d > 0.0 ? d : 1.0);  // (uniform: 1 / L_jj)
        const double l = a[j] * r;  // L[i][j] for i >= j
        a[j] = l;
        x[j] *= r;
#pragma unroll
        for (int c = j + 1; c < 16; ++c) {
            const double lc = rl(l, c);  // L[c][j] from lane c
            a[c] = fma(-l, lc, a[c]);
            x[c] = fma(-lc, x[j], x[c]);
        }
    }
    if (lane < 16) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            lds_inv[opo(r, i)] = x[r];
            Lg[r * 16 + i] = x[r];
        }
    }
    return ok;
}
// The same factor + inverse with four lanes per row (lane 4 i + q: row i, columns 4 q .. 4 q + 3):
// per column j the pivot comes by v_readlane, L_ij = a_ij / L_jj is formed on the quad lane that holds
// column j and spread over its quad by a quad_perm DPP move, and each lane forms the L_cj of its own
// four columns from row j's copies a_jc (ds_bpermute from lane 4 j + q, issued before the pivot's
// square root) — four FMAs per lane per column instead of fifteen, and four permutes instead of
// fifteen scalar broadcasts.  The whole symmetric tile is held and every update is symmetric
// (fma(-L_ik, L_ck, a_ic) and fma(-L_ck, L_ik, a_ci) round the same product), so a_jc == a_cj
// bitwise and every element sees the same operations in the same order as potrf_inv16_t: bitwise
// the same L^-1.
template <int J>
__device__ __forceinline__ double quad_bcast(double v) {
    constexpr int ctrl = J | (J << 2) | (J << 4) | (J << 6);  // quad_perm [J, J, J, J]
    // (every lane has a source inside its quad: no "old" operand to initialise)
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), ctrl, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), ctrl, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
template <class Rd>
__device__ __forceinline__ bool potrf_inv16_quad(Rd rd, double* lds_inv, double* Lg) {
    const int lane = threadIdx.x & 63, i = lane >> 2, q = lane & 3;
    double a[4], x[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int c = 4 * q + m;
        a[m] = c <= i ? rd(i, c) : rd(c, i);
        x[m] = c == i ? 1.0 : 0.0;
    }
    bool ok = true;
    static_for<0, 16>([&](auto jc) {
        constexpr int j = decltype(jc)::value, jq = j >> 2, jm = j & 3;
        const double d = rl(a[jm], 4 * j + jq);
        ok = ok && d > 0.0 && d < 1e300;
        // row j's entries a_jc (c > j), taken before the pivot is known: the permute overlaps the
        // reciprocal square root's chain instead of following it
        double aj[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) aj[m] = __shfl(a[m], 4 * j + q, 64);
        // (uniform: 1 / L_jj; |d| as a free source modifier instead of a select on the chain — a
        // non-positive pivot fails the factorisation either way, and the step is rejected)
        const double r = frsq(fabs(d));
        const double l = quad_bcast<jq>(a[jm] * r);  // L[i][j] for i >= j
        if (q == jq) x[jm] *= r;
        const double xj = quad_bcast<jq>(x[jm]);
        double lc[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) lc[m] = aj[m] * r;  // L[c][j] = a_jc / L_jj (a_jc == a_cj bitwise, below)
#pragma unroll
        for (int m = 0; m < 4; ++m)
            if (4 * q + m > j) {
                a[m] = fma(-l, lc[m], a[m]);
                x[m] = fma(-lc[m], xj, x[m]);
            }
    });
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        lds_inv[opo(4 * q + m, i)] = x[m];
        Lg[(4 * q + m) * 16 + i] = x[m];
    }
    return ok;
}
__device__ __forceinline__ bool potrf_inv16(const double* A, int ld, double* lcol, double* lds_inv, double* Lg) {
    (void)lcol;
    return potrf_inv16_t([&](int r, int c) { return A[(long long)r * ld + c]; }, lds_inv, Lg);
}

// Per-component tile program (host symbolic factorisation, vx_sba_plan): int offsets into a.tl.
enum {
    kHdrCopy = 0,   // nonzero tiles of L + the rhs tile row (packed ti << 16 | tj)
    kHdrNCopy,
    kHdrPanel,      // nt + 1 pointers (absolute into tl), then per step the panel tile rows
    kHdrTrail,      // nt + 1 pointers, then per step the trailing tiles
    kHdrBack,       // nt + 1 pointers, then per step k the tile columns m < k of row k
    kHdrNt,
    kHdrTrailSplit, // nt pointers: per step k, the end of its column-(k + 1) tiles (listed first)
    kHdrN = 8
};

// Levenberg-Marquardt decision (wave 0 of every workgroup computes it from the fixed-order totals,
// identically; workgroup 0 of component 0 publishes the state): *s_solve / *s_lambda in LDS.
__device__ __forceinline__ void solve_decide(const SBAArgs& a, int it, bool publish, int* s_solve, double* s_lambda) {
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int n6 = 6 * a.nk;
    const double* rhs_g = a.red_sum + a.s_total;
    if (wv == 0) {
        double tot = 0.0, cnt = 0.0;
        for (int q = lane; q < a.nk; q += 64) {
            tot += rhs_g[2 * n6 + 2 * q];
            cnt += rhs_g[2 * n6 + 2 * q + 1];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            tot += __shfl_xor(tot, o, 64);
            cnt += __shfl_xor(cnt, o, 64);
        }
        if (lane == 0) {
            LMVars nx;
            bool act;
            const int step = lm_decide(a, it, tot, (int)cnt, nx, act);
            *s_solve = nx.do_solve;
            *s_lambda = it == 0 ? a.lambda0 : a.st->lm[it & 1].lambda;  // the damping S was assembled with
            if (publish) {
                SBAState* st = a.st;
                st->lm[(it + 1) & 1] = nx;
                if (it == 0) {
                    st->initial_cost = tot;
                    for (int q = 1; q < 16; ++q) {
                        st->cost[q] = 0;
                        st->obs[q] = 0;
                        st->step[q] = 0;
                    }
                }
                if (it < 16) {
                    st->cost[it] = tot;
                    st->obs[it] = (int)cnt;
                    st->step[it] = step;
                }
                st->iterations = it + 1;
                if (act)
                    st->active[it + 1] = 1;
                else
                    for (int q = it + 1; q <= a.max_iter; ++q) st->active[q] = 0;
            }
        }
    }
    __syncthreads();
}

// k_sba_blocks wrote the component matrix straight into L (the all-reduce did, sharded): add the
// damping on the diagonal, the identity on padding rows and the rhs tile row
__device__ __forceinline__ void solve_damp(const SBAArgs& a, int comp, double lambda, double* L, int np, int threads) {
    const int n6 = 6 * a.nk;
    const double* rhs_g = a.red_sum + a.s_total;
    const int kq0 = a.comp_kf_ptr[comp], nc = 6 * (a.comp_kf_ptr[comp + 1] - kq0);
    for (int e = threadIdx.x; e < np; e += threads) {
        double* dg = L + (long long)e * np + e;
        if (e < nc) {
            const int g = 6 * a.comp_kf[kq0 + e / 6] + e % 6;
            *dg += lambda * rhs_g[n6 + g] + 1e-6;
            L[(long long)np * np + e] = rhs_g[g];
        } else {
            *dg = 1.0;
            L[(long long)np * np + e] = 0.0;
        }
    }
}

// Blocked back-substitution L^T x = y over the component's tile rows, descending (ys: y in LDS,
// overwritten with x): x_k = L_kk^-T y_k, then y_m -= L_km^T x_k over row k's nonzero tiles.  Lanes
// work in 16-lane groups, lane c of a group forming column c's dot product over the 16 rows in order
// (no cross-lane reduction); the 16 groups of the workgroup take one tile each per step, wave 0's
// first group also x_k.  The operands of step k - 1 (L_kk^-1 and one tile per group) are loaded,
// unconditionally (absent tiles read a valid one and are not used), while step k runs: they do not
// depend on x, so a step waits on LDS and two barriers, not on global memory.  Rows with more than 16
// nonzero tiles take the rest in place.
constexpr int kBsGroups = kSolveThreads / 16;
constexpr int kBsDepth = 3;  // steps of operands in flight (default; $VX_SBA_BS_DEPTH=6 for A/B)
// operands of step k: L_kk^-1 column c (wave 0 only: a wave-uniform branch) and the group's tile of
// row k (absent: a valid tile, unused); sbp / sbl: the row pointers / tile columns in LDS
__device__ __forceinline__ void bs_load(const double* L, const double* Linv, int np, int k, const int* sbp,
                                        const int* sbl, double (&li)[16], double (&tv)[16], int& tm) {
    const int grp = threadIdx.x >> 4, c = threadIdx.x & 15;
    if ((threadIdx.x >> 6) == 0) {
        const double* Li = Linv + 256 * k;
#pragma unroll
        for (int r = 0; r < 16; ++r) li[r] = Li[r * 16 + c];
    }
    const int q = sbp[k] + grp;
    tm = q < sbp[k + 1] ? sbl[q] : -1;
    const double* Lkm = L + (long long)(16 * k) * np + 16 * (tm >= 0 ? tm : k);
#pragma unroll
    for (int r = 0; r < 16; ++r) tv[r] = Lkm[(long long)r * np + c];
}
// column c's dot product over 16 rows: four interleaved FMA chains, combined pairwise
__device__ __forceinline__ double bs_dot(const double (&w)[16], const double* x) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r & 3] = fma(w[r], x[r], acc[r & 3]);
    return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}
// Blocked back-substitution L^T x = y over the component's tile rows, descending (ys: y in LDS,
// overwritten with x): x_k = L_kk^-T y_k, then y_m -= L_km^T x_k over row k's nonzero tiles.  Lanes
// work in 16-lane groups, lane c of a group forming column c's dot product (no cross-lane
// reduction); the 16 groups take one tile each per step, wave 0's first group also x_k.  The
// operands of step k - kBsDepth are loaded right after step k's use of their register stage (the
// k loop unrolled by kBsDepth, so each stage keeps its registers): they do not depend on x, so a step
// waits on LDS and two barriers, not on memory.  Rows of more than 16 tiles take the rest in place.
// sbp / sbl: LDS for the back lists (nt + 1 pointers, then the tile columns).
template <int kBsD>
__device__ __forceinline__ void back_substitute(const double* L, const double* Linv, int np, int nt, const int* tl,
                                                const int* bptr, double* ys, int* sbp, int* sbl) {
    const int tid = threadIdx.x, grp = tid >> 4, c = tid & 15;
    const int b0 = bptr[0], nb = bptr[nt] - b0;
    for (int e = tid; e < np; e += kSolveThreads) ys[e] = L[(long long)np * np + e];
    for (int e = tid; e <= nt; e += kSolveThreads) sbp[e] = bptr[e] - b0;
    for (int e = tid; e < nb; e += kSolveThreads) sbl[e] = tl[b0 + e];
    __syncthreads();
    double li[kBsD][16], tv[kBsD][16];
    int tm[kBsD];
#pragma unroll
    for (int s = 0; s < kBsD; ++s) {
        tm[s] = -1;
        if (nt - 1 - s >= 0) bs_load(L, Linv, np, nt - 1 - s, sbp, sbl, li[s], tv[s], tm[s]);
    }
    for (int k0 = nt - 1; k0 >= 0; k0 -= kBsD) {
#pragma unroll
        for (int s = 0; s < kBsD; ++s) {
            const int k = k0 - s;
            if (k < 0) break;
            if (grp == 0) {  // x_k = L_kk^-T y_k (lane c: column c of L_kk^-1)
                double yk[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) yk[r] = ys[16 * k + r];
                ys[16 * k + c] = bs_dot(li[s], yk);  // (the group's reads of y_k precede its writes)
            }
            __syncthreads();
            double xk[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) xk[r] = ys[16 * k + r];
            if (tm[s] >= 0) ys[16 * tm[s] + c] -= bs_dot(tv[s], xk);  // y_m -= L_km^T x_k
            for (int q = sbp[k] + kBsGroups + grp; q < sbp[k + 1]; q += kBsGroups) {
                const int mm = sbl[q];
                const double* Lkm = L + (long long)(16 * k) * np + 16 * mm;
                double w[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) w[r] = Lkm[(long long)r * np + c];
                ys[16 * mm + c] -= bs_dot(w, xk);
            }
            if (k - kBsD >= 0) bs_load(L, Linv, np, k - kBsD, sbp, sbl, li[s], tv[s], tm[s]);
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(kSolveThreads) void k_sba_solve(SBAArgs a, int it) {
    if (it > 0 && !a.st->active[it]) return;
    extern __shared__ __attribute__((aligned(32))) double smem[];
    __shared__ int s_solve;
    __shared__ double s_lambda;
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int comp = blockIdx.x;
    solve_decide(a, it, comp == 0, &s_solve, &s_lambda);
    if (!s_solve) return;
    VX_KT(0);
    const double lambda = s_lambda;
    const int* hdr = a.comp_hdr + kHdrN * comp;
    const int nt = hdr[kHdrNt], np = 16 * nt;
    double* L = a.L + a.comp_loff[comp];
    double* Linv = a.Linv + a.comp_loff[comp];  // same offsets as L (>= 16 np per component)
    const int* tl = a.tl;
    // LDS: the step's panel tiles in slots (position in the column's panel list), L_kk^-1, the POTRF
    // column images, y / x, and tile row -> panel slot of the current step.  A column with more
    // panel tiles than slots (dense components of several hundred keyframes) is read from global.
    const int ps = a.panel_slots;
    double* panel = smem;                                       // ps operand-order tiles
    double* dlds = smem + (long long)ps * kPanelStride;         // L_kk^-1 of the current step
    double* lcol = dlds + kPanelStride;                         // POTRF column images (272 doubles)
    double* ys = lcol + 2 * kPanelStride;                       // np: y, then x
    int* slot_of = reinterpret_cast<int*>(ys + np);             // nt + 1
    const int r0 = lane >> 4, cl = lane & 15;
    solve_damp(a, comp, lambda, L, np, kSolveThreads);
    __syncthreads();
    VX_KT(1);
    bool ok = true;
    const int* pptr = tl + hdr[kHdrPanel];
    const int* tptr = tl + hdr[kHdrTrail];
    for (int k = 0; k < nt; ++k) {
        // trace slots: steps 0, 1 and nt / 2 (factor | panel | trailing update)
        const int kts = k == 0 ? 2 : (k == 1 ? 5 : (k == nt / 2 ? 8 : -1));
        double* Lkk = L + (long long)(16 * k) * np + 16 * k;
        if (wv == 0) ok = potrf_inv16(Lkk, np, lcol, dlds, Linv + 256 * k) && ok;
        __syncthreads();
        if (kts >= 0) VX_KT(kts);
        // panel: L_ik = A_ik L_kk^-T over the nonzero tiles of column k (and the rhs row)
        const bool in_lds = pptr[k + 1] - pptr[k] <= ps;
        for (int q = pptr[k] + wv; q < pptr[k + 1]; q += kSolveWaves) {
            const int i = tl[q];
            const int slot = q - pptr[k];
            double* Aik = L + (long long)(16 * i) * np + 16 * k;
            // the A operand in operand order straight from global: row l & 15, columns 4 (l >> 4) ..
            const double4 av = *reinterpret_cast<const double4*>(Aik + (long long)cl * np + 4 * r0);
            const double4 bv = *reinterpret_cast<const double4*>(dlds + 4 * lane);
            d4 c = {0.0, 0.0, 0.0, 0.0};
            c = __builtin_amdgcn_mfma_f64_16x16x4f64(av.x, bv.x, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f64_16x16x4f64(av.y, bv.y, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f64_16x16x4f64(av.z, bv.z, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f64_16x16x4f64(av.w, bv.w, c, 0, 0, 0);
            store_acc(Aik, np, c);
            if (in_lds) store_acc_opo(panel + (long long)slot * kPanelStride, c);
            if (lane == 0) slot_of[i] = slot;
        }
        __syncthreads();
        if (kts >= 0) VX_KT(kts + 1);
        // trailing update A_ij -= L_ik L_jk^T over the tiles the symbolic factorisation lists,
        // four tiles per wave in flight
        const int t_beg = tptr[k], t_end = tptr[k + 1];
        for (int t0 = t_beg + wv * 4; t0 < t_end; t0 += kSolveWaves * 4) {
            d4 c[4];
            int ti[4], tj[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int t = t0 + q;
                ti[q] = -1;
                if (t < t_end) {
                    ti[q] = tl[t] >> 16;
                    tj[q] = tl[t] & 0xffff;
                    c[q] = load_acc(L + (long long)(16 * ti[q]) * np + 16 * tj[q], np);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (ti[q] < 0) continue;
                if (in_lds)
                    c[q] = mfma_abt(panel + (long long)slot_of[ti[q]] * kPanelStride,
                                    panel + (long long)slot_of[tj[q]] * kPanelStride, c[q], true);
                else
                    c[q] = mfma_abt_g(L + (long long)(16 * ti[q]) * np + 16 * k, L + (long long)(16 * tj[q]) * np + 16 * k,
                                      np, c[q]);
                store_acc(L + (long long)(16 * ti[q]) * np + 16 * tj[q], np, c[q]);
            }
        }
        __syncthreads();
        if (kts >= 0) VX_KT(kts + 2);
    }
    VX_KT(11);
    if (wv == 0 && lane == 0 && !ok) atomicOr(&a.st->fail[it], 1);
    // (the back-substitution and dx: k_sba_backsub; the clearing of the touched tiles: k_sba_update)
}

// ------------------------------------------------------------------------- multi-workgroup factor
// The same right-looking tiled Cholesky as k_sba_solve, spread over G workgroups per component and
// one launch per step (the kernel boundary is the step's synchronisation): launch k applies step k's
// trailing update A_ij -= L_ik L_jk^T — workgroup 0 to the tiles of column k + 1 (listed first by
// the symbolic factorisation), which it then factors (POTRF + L_kk^-1 of tile k + 1) and turns into
// the panel L_i,k+1 (look-ahead), the other G - 1 workgroups to the rest, operands read in operand
// order from the factor in global memory.  Every tile sees the same operations in the same order as
// in k_sba_solve, so the factor is bitwise the same; a connected window's 75-column factor no longer
// runs on one CU.  k_sba_fac_begin: decision, damping, step 0's factor + panel; k_sba_backsub: the
// back-substitution, dx and the clearing of the touched tiles (k_sba_solve's tail).

// wave-parallel panel of column k: L_ik = A_ik L_kk^-T (dlds: L_kk^-1 in operand order)
__device__ __forceinline__ void panel_column(double* L, int np, const int* tl, int p0, int p1, int k,
                                             const double* dlds, int waves) {
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, r0 = lane >> 4, cl = lane & 15;
    for (int q = p0 + wv; q < p1; q += waves) {
        double* Aik = L + (long long)(16 * tl[q]) * np + 16 * k;
        const double4 av = *reinterpret_cast<const double4*>(Aik + (long long)cl * np + 4 * r0);
        const double4 bv = *reinterpret_cast<const double4*>(dlds + 4 * lane);
        d4 c = {0.0, 0.0, 0.0, 0.0};
        c = __builtin_amdgcn_mfma_f64_16x16x4f64(av.x, bv.x, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f64_16x16x4f64(av.y, bv.y, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f64_16x16x4f64(av.z, bv.z, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f64_16x16x4f64(av.w, bv.w, c, 0, 0, 0);
        store_acc(Aik, np, c);
    }
}

// trailing tiles tl[beg + m * stride] (m = 0, 1, ..., < end) of step k, four per wave in flight
__device__ __forceinline__ void trail_tiles(double* L, int np, const int* tl, int k, int beg, int end, int stride,
                                            int waves) {
    const int wv = threadIdx.x >> 6;
    const int cnt = end > beg ? (end - beg + stride - 1) / stride : 0;
    for (int m0 = wv * 4; m0 < cnt; m0 += waves * 4) {
        d4 c[4];
        int ti[4], tj[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            ti[q] = -1;
            if (m0 + q < cnt) {
                const int e = tl[beg + (m0 + q) * stride];
                ti[q] = e >> 16;
                tj[q] = e & 0xffff;
                c[q] = load_acc(L + (long long)(16 * ti[q]) * np + 16 * tj[q], np);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (ti[q] < 0) continue;
            c[q] = mfma_abt_g(L + (long long)(16 * ti[q]) * np + 16 * k, L + (long long)(16 * tj[q]) * np + 16 * k, np,
                              c[q]);
            store_acc(L + (long long)(16 * ti[q]) * np + 16 * tj[q], np, c[q]);
        }
    }
}

// factor of tile column k (wave 0) and its panel (all waves); a non-positive pivot flags the iteration
__device__ __forceinline__ void factor_column(const SBAArgs& a, int it, double* L, double* Linv, int np, const int* tl,
                                              int p0, int p1, int k, double* lcol, double* dlds) {
    const int wv = threadIdx.x >> 6;
    if (wv == 0) {
        const bool ok = potrf_inv16(L + (long long)(16 * k) * np + 16 * k, np, lcol, dlds, Linv + 256 * k);
        if (!ok && threadIdx.x == 0) atomicOr(&a.st->fail[it], 1);
    }
    __syncthreads();
    panel_column(L, np, tl, p0, p1, k, dlds, kSolveWaves);
}

// pair: also column 1 (step 0's update of it, then its factor) for the two-column schedule
__global__ __launch_bounds__(kSolveThreads) void k_sba_fac_begin(SBAArgs a, int it, int pair) {
    if (it > 0 && !a.st->active[it]) return;
    __shared__ int s_solve;
    __shared__ double s_lambda;
    __shared__ __attribute__((aligned(32))) double lds[3 * kPanelStride];  // L_kk^-1 | POTRF columns
    const int comp = blockIdx.x;
    solve_decide(a, it, comp == 0, &s_solve, &s_lambda);
    if (!s_solve) return;
    const int* hdr = a.comp_hdr + kHdrN * comp;
    const int nt = hdr[kHdrNt], np = 16 * nt;
    double* L = a.L + a.comp_loff[comp];
    solve_damp(a, comp, s_lambda, L, np, kSolveThreads);
    __syncthreads();
    const int* pptr = a.tl + hdr[kHdrPanel];
    factor_column(a, it, L, a.Linv + a.comp_loff[comp], np, a.tl, pptr[0], pptr[1], 0, lds + kPanelStride, lds);
    if (pair && nt > 1) {
        const int* tptr = a.tl + hdr[kHdrTrail];
        __syncthreads();
        trail_tiles(L, np, a.tl, 0, tptr[0], a.tl[hdr[kHdrTrailSplit]], 1, kSolveWaves);
        __syncthreads();
        factor_column(a, it, L, a.Linv + a.comp_loff[comp], np, a.tl, pptr[1], pptr[2], 1, lds + kPanelStride, lds);
    }
}

// Workgroup 0's look-ahead in launch k: column k + 1 kept in LDS from its step-k update to its panel.
// The updated diagonal tile goes to LDS row-major (POTRF reads it there), the updated panel tiles as
// MFMA operand images (the panel reads them there); neither is stored to global memory, since the
// panel overwrites the off-diagonal ones and only L_kk^-1 of a diagonal tile is read later.  Same
// operations, same order as factor_column over global memory.  sm: diagonal tile | L_kk^-1 | POTRF
// columns (2 tiles) | ps panel images | tile row -> slot (nt + 1) | updated flags (ps).
__device__ __forceinline__ void lookahead_column(const SBAArgs& a, int it, double* L, double* Linv, int np, int nt, const int* tl,
                                 int p0, int p1, int k, int la_beg, int la_end, double* sm, int ps, bool kt) {
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, r0 = lane >> 4, cl = lane & 15;
    double* dtile = sm;
    double* dlds = sm + kPanelStride;
    double* lcol = sm + 2 * kPanelStride;
    double* pan = sm + 4 * kPanelStride;
    int* slot_of = reinterpret_cast<int*>(pan + (size_t)ps * kPanelStride);
    int* upd = slot_of + nt + 1;
    const int c1 = k + 1, pn = p1 - p0;
    const bool in_lds = pn <= ps;
    for (int q = tid; q < pn; q += kSolveThreads) {
        slot_of[tl[p0 + q]] = q;
        if (in_lds) upd[q] = 0;
    }
    __syncthreads();
    if (kt) VX_KT(2);
    // step k's update of column k + 1 (the diagonal tile is the first entry when the column has one)
    const bool diag = la_end > la_beg;
    const int cnt = la_end - la_beg;
    for (int m0 = wv * 4; m0 < cnt; m0 += kSolveWaves * 4) {
        d4 c[4];
        int ti[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            ti[q] = -1;
            if (m0 + q < cnt) {
                ti[q] = tl[la_beg + m0 + q] >> 16;
                c[q] = load_acc(L + (long long)(16 * ti[q]) * np + 16 * c1, np);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (ti[q] < 0) continue;
            c[q] = mfma_abt_g(L + (long long)(16 * ti[q]) * np + 16 * k, L + (long long)(16 * c1) * np + 16 * k, np, c[q]);
            if (ti[q] == c1) {
                store_acc(dtile, 16, c[q]);
            } else if (in_lds) {
                const int sl = slot_of[ti[q]];
                store_acc_opo(pan + (size_t)sl * kPanelStride, c[q]);
                if (lane == 0) upd[sl] = 1;
            } else {
                store_acc(L + (long long)(16 * ti[q]) * np + 16 * c1, np, c[q]);
            }
        }
    }
    if (kt) VX_KT(3);
    __syncthreads();
    if (kt) VX_KT(4);
    if (wv == 0) {
        const bool ok = diag ? potrf_inv16(dtile, 16, lcol, dlds, Linv + 256 * c1)
                             : potrf_inv16(L + (long long)(16 * c1) * np + 16 * c1, np, lcol, dlds, Linv + 256 * c1);
        if (!ok && tid == 0) atomicOr(&a.st->fail[it], 1);
    }
    __syncthreads();
    if (kt) VX_KT(5);
    // the panel L_i,k+1 = A_i,k+1 L_k+1,k+1^-T: updated tiles from LDS, the others from global
    for (int q = wv; q < pn; q += kSolveWaves) {
        double* Aik = L + (long long)(16 * tl[p0 + q]) * np + 16 * c1;
        const double4 av = (in_lds && upd[q]) ? *reinterpret_cast<const double4*>(pan + (size_t)q * kPanelStride + 4 * lane)
                                              : *reinterpret_cast<const double4*>(Aik + (long long)cl * np + 4 * r0);
        const double4 bv = *reinterpret_cast<const double4*>(dlds + 4 * lane);
        d4 c = {0.0, 0.0, 0.0, 0.0};
        c = __builtin_amdgcn_mfma_f64_16x16x4f64(av.x, bv.x, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f64_16x16x4f64(av.y, bv.y, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f64_16x16x4f64(av.z, bv.z, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f64_16x16x4f64(av.w, bv.w, c, 0, 0, 0);
        store_acc(Aik, np, c);
    }
    if (kt) VX_KT(6);
}

// launch k of the factorisation (k = 0 .. max_nt - 2): blockIdx.x = component * G + g; ps: LDS panel
// images of workgroup 0's look-ahead (0: the look-ahead over global memory, factor_column).  The
// step's list bounds come as the launch argument sd for a one-component plan (sd.nt > 0), else from
// the plan's descriptor table — loaded with the run flags, so the tile lists are the first dependent
// loads.
__global__ __launch_bounds__(kSolveThreads) void k_sba_fac_step(SBAArgs a, int it, int k, int G, int ps, FacStep sd) {
    const int comp = blockIdx.x / G, g = blockIdx.x - comp * G;
    if (sd.nt == 0) {
        const int* d = a.fac_steps + 8 * ((size_t)comp * a.fac_nk + k);
        const int4 d0 = *reinterpret_cast<const int4*>(d), d1 = *reinterpret_cast<const int4*>(d + 4);
        sd.loff = (long long)(((unsigned long long)(unsigned)d0.y << 32) | (unsigned)d0.x);
        sd.la_beg = d0.z;
        sd.split = d0.w;
        sd.t_end = d1.x;
        sd.p0 = d1.y;
        sd.p1 = d1.z;
        sd.nt = d1.w;
    }
    // trace build: the phases of launch k = nt / 2 (slots 0-7, workgroup 0 and the rest)
    const bool kt = k == sd.nt / 2;
    if (kt) VX_KT(0);
    if (it > 0 && !a.st->active[it]) return;
    if (!a.st->lm[(it + 1) & 1].do_solve) return;  // (k_sba_fac_begin's decision)
    if (kt) VX_KT(1);
    extern __shared__ __attribute__((aligned(32))) double sm[];
    const int nt = sd.nt, np = 16 * nt;
    if (k + 1 >= nt) return;
    double* L = a.L + sd.loff;
    double* Linv = a.Linv + sd.loff;
    const int* tl = a.tl;
    if (g == 0) {
        if (G == 1) trail_tiles(L, np, tl, k, sd.split, sd.t_end, 1, kSolveWaves);
        if (ps > 0) {
            lookahead_column(a, it, L, Linv, np, nt, tl, sd.p0, sd.p1, k, sd.la_beg, sd.split, sm, ps, kt);
        } else {
            trail_tiles(L, np, tl, k, sd.la_beg, sd.split, 1, kSolveWaves);
            __syncthreads();
            factor_column(a, it, L, Linv, np, tl, sd.p0, sd.p1, k + 1, sm + kPanelStride, sm);
        }
    } else {
        trail_tiles(L, np, tl, k, sd.split + (g - 1), sd.t_end, G - 1, kSolveWaves);
        if (kt) VX_KT(7);
    }
}

// Tiles of the two-column schedule, entries i << 16 | c << 2 | mask, taking steps s0 (mask bit 0)
// and s0 + 1 (bit 1) in that order — the per-tile sequence of the one-step schedule, one load and one
// store instead of two; entries beg, beg + stride, ...; four per wave in flight
__device__ __forceinline__ void masked_tiles(double* L, int np, const int* tl, int s0, int beg, int end, int stride,
                                             int waves) {
    const int wv = threadIdx.x >> 6;
    const int cnt = end > beg ? (end - beg + stride - 1) / stride : 0;
    for (int m0 = wv * 4; m0 < cnt; m0 += waves * 4) {
        d4 c[4];
        int ti[4], tj[4], mk[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            ti[q] = -1;
            if (m0 + q < cnt) {
                const int e = tl[beg + (m0 + q) * stride];
                ti[q] = e >> 16;
                tj[q] = (e >> 2) & 0x3fff;
                mk[q] = e & 3;
                c[q] = load_acc(L + (long long)(16 * ti[q]) * np + 16 * tj[q], np);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (ti[q] < 0) continue;
            if (mk[q] & 1)
                c[q] = mfma_abt_g(L + (long long)(16 * ti[q]) * np + 16 * s0, L + (long long)(16 * tj[q]) * np + 16 * s0,
                                  np, c[q]);
            if (mk[q] & 2)
                c[q] = mfma_abt_g(L + (long long)(16 * ti[q]) * np + 16 * (s0 + 1),
                                  L + (long long)(16 * tj[q]) * np + 16 * (s0 + 1), np, c[q]);
            store_acc(L + (long long)(16 * ti[q]) * np + 16 * tj[q], np, c[q]);
        }
    }
}

// Launch t of the two-column schedule (columns 0 and 1 factored by k_sba_fac_begin): steps 2t and
// 2t + 1 are applied — workgroup 0 to columns c0 = 2t + 2 and c0 + 1 (phase 1), then it factors c0,
// applies step c0 to column c0 + 1 (phase 2) and factors that; the other G - 1 workgroups apply both
// steps to the columns beyond.  Every tile still receives its steps in ascending order, so the
// factor is bitwise the one-step schedule's; half the launches.
__global__ __launch_bounds__(kSolveThreads) void k_sba_fac_pair(SBAArgs a, int it, int t, int G, FacPair sd) {
    const int comp = blockIdx.x / G, g = blockIdx.x - comp * G;
    if (sd.nt == 0) {
        const int* d = a.fac_pairs + 16 * ((size_t)comp * a.fac_np + t);
        const int4 d0 = *reinterpret_cast<const int4*>(d), d1 = *reinterpret_cast<const int4*>(d + 4),
                   d2 = *reinterpret_cast<const int4*>(d + 8), d3 = *reinterpret_cast<const int4*>(d + 12);
        sd.loff = (long long)(((unsigned long long)(unsigned)d0.y << 32) | (unsigned)d0.x);
        sd.l1b = d0.z;
        sd.l1e = d0.w;
        sd.l2b = d1.x;
        sd.l2e = d1.y;
        sd.rb = d1.z;
        sd.re = d1.w;
        sd.p0 = d2.x;
        sd.p1 = d2.y;
        sd.q0 = d2.z;
        sd.q1 = d2.w;
        sd.nt = d3.x;
        sd.c0 = d3.y;
    }
    if (it > 0 && !a.st->active[it]) return;
    if (!a.st->lm[(it + 1) & 1].do_solve) return;
    __shared__ __attribute__((aligned(32))) double lds[3 * kPanelStride];
    const int nt = sd.nt, np = 16 * nt, c0 = sd.c0;
    if (c0 >= nt) return;
    double* L = a.L + sd.loff;
    double* Linv = a.Linv + sd.loff;
    const int* tl = a.tl;
    const int s0 = c0 - 2;
    if (g == 0) {
        masked_tiles(L, np, tl, s0, sd.l1b, sd.l1e, 1, kSolveWaves);
        if (G == 1) masked_tiles(L, np, tl, s0, sd.rb, sd.re, 1, kSolveWaves);
        __syncthreads();
        factor_column(a, it, L, Linv, np, tl, sd.p0, sd.p1, c0, lds + kPanelStride, lds);
        if (c0 + 1 < nt) {
            __syncthreads();
            trail_tiles(L, np, tl, c0, sd.l2b, sd.l2e, 1, kSolveWaves);
            __syncthreads();
            factor_column(a, it, L, Linv, np, tl, sd.q0, sd.q1, c0 + 1, lds + kPanelStride, lds);
        }
    } else {
        masked_tiles(L, np, tl, s0, sd.rb + (g - 1), sd.re, G - 1, kSolveWaves);
    }
}

// ------------------------------------------------------------------------- blocked factor
// The same right-looking tiled Cholesky in blocks of up to kFbW tile columns, one launch per block
// (round 5: the one-launch-per-column form spent ~13 us per column on workgroup 0's chain, most of it
// global round trips and the launch).  Launch t: workgroup 0 loads every tile of block t's columns
// (at most kFbCap tiles), which k_sba_fac_upd's launch just before brought up to date with block
// t - 1's steps (the look-ahead), and factors the block in LDS — per column POTRF + L^-1 of the
// diagonal tile, the panel
// L_ic = A_ic L_cc^-T (written to the factor in global memory as well), then the column's steps on the
// block's later columns — while G - 1 workgroups apply block t - 1's steps to the tiles beyond block t.
// Every tile receives its steps in ascending order with the same operations (MFMA operands read in
// operand order from LDS instead of global memory: the same values), so the factor is bitwise the
// one-column forms' and the single workgroup's.  Launch 0 also takes the LM decision and the damping.
constexpr int kFbThreads = 512;
constexpr int kFbWaves = kFbThreads / 64;
constexpr int kFbW = 4;       // tile columns per block (4-bit step masks)
constexpr int kFbCap = 60;    // LDS tiles of a block (operand order, 2 KB each; 72 measured no faster: 19 blocks of 19.3 µs against 24 of 14.8)

__device__ __forceinline__ d4 load_acc_opo(const double* S) {
    const int lane = threadIdx.x & 63, r0 = lane >> 4, c = lane & 15;
    d4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = S[opo(r0 + 4 * r, c)];
    return v;
}

// Tiles of launch t: entries i << 16 | j << 4 | mask, steps k0 + s for the mask's bits s in ascending
// order (entries beg, beg + stride, ...), two tiles per wave at a time with every operand of their
// steps requested together (one memory round trip per pair of tiles, not one per step)
__device__ __forceinline__ void blk_tiles_pf(double* L, int np, const int* tl, int k0, int beg, int end, int stride,
                                             int waves) {
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, r0 = lane >> 4, cl = lane & 15;
    const int cnt = end > beg ? (end - beg + stride - 1) / stride : 0;
    for (int m0 = wv * 2; m0 < cnt; m0 += waves * 2) {
        d4 c[2];
        int ti[2], tj[2], mk[2];
        double4 A[2][kFbW], B[2][kFbW];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            mk[q] = 0;
            ti[q] = tj[q] = 0;
            if (m0 + q < cnt) {
                const int e = tl[beg + (m0 + q) * stride];
                ti[q] = e >> 16;
                tj[q] = (e >> 4) & 0xfff;
                mk[q] = e & 15;
                c[q] = load_acc(L + (long long)(16 * ti[q]) * np + 16 * tj[q], np);
#pragma unroll
                for (int s = 0; s < kFbW; ++s)
                    if ((mk[q] >> s) & 1) {
                        A[q][s] = *reinterpret_cast<const double4*>(L + (long long)(16 * ti[q] + cl) * np + 16 * (k0 + s) + 4 * r0);
                        B[q][s] = *reinterpret_cast<const double4*>(L + (long long)(16 * tj[q] + cl) * np + 16 * (k0 + s) + 4 * r0);
                    }
            }
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            if (m0 + q >= cnt) continue;
#pragma unroll
            for (int s = 0; s < kFbW; ++s)
                if ((mk[q] >> s) & 1) {  // (the order of mfma_abt_g)
                    c[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(-A[q][s].x, B[q][s].x, c[q], 0, 0, 0);
                    c[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(-A[q][s].y, B[q][s].y, c[q], 0, 0, 0);
                    c[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(-A[q][s].z, B[q][s].z, c[q], 0, 0, 0);
                    c[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(-A[q][s].w, B[q][s].w, c[q], 0, 0, 0);
                }
            store_acc(L + (long long)(16 * ti[q]) * np + 16 * tj[q], np, c[q]);
        }
    }
}

// The look-ahead as a launch of its own (before k_sba_fac_blk's launch t >= 1): block t - 1's steps
// applied to block t's tiles by G workgroups, so workgroup 0 of the factor launch loads block t
// finished instead of running ~2 MFLOP of updates on its one CU (round 5: 711 -> 617 µs per LM
// iteration at the connected C5; workgroup 0's own row-wise look-ahead has been removed since).
__global__ __launch_bounds__(kFbThreads) void k_sba_fac_upd(SBAArgs a, int it, int t, int G, FacBlk sd) {
    const int comp = blockIdx.x / G, g = blockIdx.x - comp * G;
    if (sd.nt == 0) {
        const int* d = a.fac_blks + 16 * ((size_t)comp * a.fac_nb + t);
        const int4 d0 = *reinterpret_cast<const int4*>(d), d2 = *reinterpret_cast<const int4*>(d + 8),
                   d3 = *reinterpret_cast<const int4*>(d + 12);
        sd.loff = (long long)(((unsigned long long)(unsigned)d0.y << 32) | (unsigned)d0.x);
        sd.K0p = d2.x;
        sd.nt = d3.x;
        sd.la_beg = d3.y;
        sd.la_end = d3.z;
    }
    if (it > 0 && !a.st->active[it]) return;
    if (sd.nt == 0 || t == 0) return;
    if (!a.st->lm[(it + 1) & 1].do_solve) return;  // (launch 0's decision)
    blk_tiles_pf(a.L + sd.loff, 16 * sd.nt, a.tl, sd.K0p, sd.la_beg + g, sd.la_end, G, kFbWaves);
}

__global__ __launch_bounds__(kFbThreads) void k_sba_fac_blk(SBAArgs a, int it, int t, int G, int cap, FacBlk sd) {
    const int comp = blockIdx.x / G, g = blockIdx.x - comp * G;
    if (sd.nt == 0) {
        const int* d = a.fac_blks + 16 * ((size_t)comp * a.fac_nb + t);
        const int4 d0 = *reinterpret_cast<const int4*>(d), d1 = *reinterpret_cast<const int4*>(d + 4),
                   d2 = *reinterpret_cast<const int4*>(d + 8), d3 = *reinterpret_cast<const int4*>(d + 12);
        sd.loff = (long long)(((unsigned long long)(unsigned)d0.y << 32) | (unsigned)d0.x);
        sd.K0 = d0.z;
        sd.W = d0.w;
        sd.bt_beg = d1.x;
        sd.bt_end = d1.y;
        sd.pb_beg = d1.z;
        sd.pb_end = d1.w;
        sd.K0p = d2.x;
        sd.Wp = d2.y;
        sd.tr_beg = d2.z;
        sd.tr_end = d2.w;
        sd.nt = d3.x;
        sd.la_beg = d3.y;
        sd.la_end = d3.z;
    }
    if (it > 0 && !a.st->active[it]) return;
    const int nt = sd.nt, np = 16 * nt;
    if (nt == 0) return;  // (this component has no block t)
    // trace build: launch nt / 8 (workgroup 0: 10 entry, 11 tables, 14 B operands staged, 0-7 each
    // wave's look-ahead rows, 12 look-ahead, 13 column 0's POTRF, 15 block done; 7 of another
    // workgroup: its trailing tiles)
    const bool kt = t == nt / 8;
    double* L = a.L + sd.loff;
    double* Linv = a.Linv + sd.loff;
    const int* tl = a.tl;
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    if (t == 0) {
        if (g != 0) return;
        __shared__ int s_solve;
        __shared__ double s_lambda;
        solve_decide(a, it, comp == 0, &s_solve, &s_lambda);
        if (!s_solve) return;
        solve_damp(a, comp, s_lambda, L, np, kFbThreads);
        __syncthreads();
    } else {
        if (!a.st->lm[(it + 1) & 1].do_solve) return;  // (launch 0's decision)
        if (kt) VX_KT(10);
        if (g > 0 || G == 1) {
            const int gg = G == 1 ? 0 : g - 1, GG = G == 1 ? 1 : G - 1;
            blk_tiles_pf(L, np, tl, sd.K0p, sd.tr_beg + gg, sd.tr_end, GG, kFbWaves);
            if (kt && g > 0) VX_KT(7);
            if (g > 0) return;
        }
    }
    extern __shared__ __attribute__((aligned(32))) double sm[];
    const int K0 = sd.K0, W = sd.W, n = sd.bt_end - sd.bt_beg, n1 = nt + 1;
    double* T = sm;                                   // cap tiles, operand order
    double* dlds = sm + (size_t)cap * kPanelStride;   // L_cc^-1 of the current column
    double* dl2 = dlds + kPanelStride;                // ... and of the next (the two alternate)
    int* ent = reinterpret_cast<int*>(dl2 + kPanelStride);  // cap entries i << 16 | c
    int* rs = ent + cap;                              // kFbW x n1: slot of (i, K0 + cc), -1: none
    int* cb = rs + kFbW * n1;                         // kFbW + 1: first slot of column cc (its diagonal)
    for (int x = tid; x < kFbW * n1; x += kFbThreads) rs[x] = -1;
    __syncthreads();
    for (int s = tid; s < n; s += kFbThreads) {
        const int e = tl[sd.bt_beg + s];
        ent[s] = e;
        rs[((e & 0xffff) - K0) * n1 + (e >> 16)] = s;
    }
    __syncthreads();
    if (tid <= W) cb[tid] = tid < W ? rs[tid * n1 + K0 + tid] : n;
    if (kt) VX_KT(11);
    // block t's tiles into LDS (block t - 1's steps: k_sba_fac_upd, the launch before) by LDS-DMA
    // (global_load_lds, 16 B a lane, no registers): two loads a tile, every tile of the wave requested
    // back to back.  Lane l of a load writes LDS doubles 2l, 2l + 1 = operand-order positions of (row
    // (l >> 1) & 15, columns 4 g + 2 (l & 1) .. + 1), g = 2 h + (l >> 5): a 16-byte piece of one tile row
    // in global memory, so the opo image is built by the source addresses.
    {
        const int row = (lane >> 1) & 15, cc = 2 * (lane & 1);
        for (int m = wv; m < n; m += kFbWaves) {
            const int e = ent[m];
            const double* src = L + (long long)(16 * (e >> 16) + row) * np + 16 * (e & 0xffff) + cc;
#pragma unroll
            for (int h = 0; h < 2; ++h)
                __builtin_amdgcn_global_load_lds(
                    (const __attribute__((address_space(1))) void*)(src + 4 * (2 * h + (lane >> 5))),
                    (__attribute__((address_space(3))) void*)(T + (size_t)m * kPanelStride + 128 * h), 16, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the LDS-DMA writes, before the barrier below)
    }
    __syncthreads();
    if (kt) VX_KT(12);
    // Per column c: the panel (all waves), a barrier, step c on the block's later columns (waves 1..),
    // a barrier.  The next column's POTRF + inverse runs on wave 0 beside step c's updates: its
    // diagonal tile's last step is the product of the panel tile L_(c+1)c with itself, which wave 0
    // forms first in the panel phase and applies at once — so the column chain is panel + max(POTRF,
    // updates), not POTRF + panel + updates.  (Two L_cc^-1 buffers alternate, dlds and dl2.  Every tile
    // sees the same operations in the same order.)
    bool ok = true;
    double* dl[2] = {dlds, dl2};
    if (wv == 0) {
        const double* D = T + (size_t)cb[0] * kPanelStride;
        ok = potrf_inv16_quad([&](int r, int q) { return D[opo(r, q)]; }, dl[0], Linv + 256 * K0);
    }
    __syncthreads();
    if (kt) VX_KT(13);
    for (int cc = 0; cc < W; ++cc) {
        const int c = K0 + cc, s0 = cb[cc], s1 = cb[cc + 1];
        const double* dc = dl[cc & 1];
        const int sn = cc + 1 < W ? rs[cc * n1 + c + 1] : -1;  // slot of L_(c+1)c (wave 0's)
        // the panel L_ic = A_ic L_cc^-T (rows below the diagonal, the rhs row last): in place and to
        // the factor
        auto panel = [&](int s) {
            double* S = T + (size_t)s * kPanelStride;
            const double4 av = *reinterpret_cast<const double4*>(S + 4 * lane);
            const double4 bv = *reinterpret_cast<const double4*>(dc + 4 * lane);
            d4 r = {0.0, 0.0, 0.0, 0.0};
            r = __builtin_amdgcn_mfma_f64_16x16x4f64(av.x, bv.x, r, 0, 0, 0);
            r = __builtin_amdgcn_mfma_f64_16x16x4f64(av.y, bv.y, r, 0, 0, 0);
            r = __builtin_amdgcn_mfma_f64_16x16x4f64(av.z, bv.z, r, 0, 0, 0);
            r = __builtin_amdgcn_mfma_f64_16x16x4f64(av.w, bv.w, r, 0, 0, 0);
            store_acc_opo(S, r);
            store_acc(L + (long long)(16 * (ent[s] >> 16)) * np + 16 * c, np, r);
        };
        if (wv == 0 && sn >= 0) {
            panel(sn);
            double* Dt = T + (size_t)cb[cc + 1] * kPanelStride;  // step c on the diagonal tile of c + 1
            d4 acc = load_acc_opo(Dt);
            acc = mfma_abt(T + (size_t)sn * kPanelStride, T + (size_t)sn * kPanelStride, acc, true);
            store_acc_opo(Dt, acc);
        }
        for (int s = s0 + 1 + wv; s < s1; s += kFbWaves)
            if (s != sn) panel(s);
        __syncthreads();
        if (cc + 1 == W) break;
        if (wv == 0) {
            const double* D = T + (size_t)cb[cc + 1] * kPanelStride;
            ok = potrf_inv16_quad([&](int r, int q) { return D[opo(r, q)]; }, dl[(cc + 1) & 1], Linv + 256 * (c + 1)) && ok;
        } else {
            // step c on the block's later columns c2: tiles (i, c2), i >= c2, for NZ(c2, c) — rows of
            // column c from the slot of (c2, c) on (the diagonal tile of c + 1: wave 0's, above)
            int tot = 0;
            for (int c2 = c + 1; c2 < K0 + W; ++c2) {
                const int sc = rs[cc * n1 + c2];
                tot += sc >= 0 ? s1 - sc : 0;
            }
            for (int p = wv - 1; p < tot; p += kFbWaves - 1) {
                int q = p, c2 = c + 1, sc = -1;
                for (; c2 < K0 + W; ++c2) {
                    sc = rs[cc * n1 + c2];
                    const int len = sc >= 0 ? s1 - sc : 0;
                    if (q < len) break;
                    q -= len;
                }
                if (c2 == c + 1 && q == 0) continue;
                const int s = sc + q;  // L_ic, with L_c2c at sc
                const int dst = rs[(c2 - K0) * n1 + (ent[s] >> 16)];
                double* Dt = T + (size_t)dst * kPanelStride;
                d4 acc = load_acc_opo(Dt);
                acc = mfma_abt(T + (size_t)s * kPanelStride, T + (size_t)sc * kPanelStride, acc, true);
                store_acc_opo(Dt, acc);
            }
        }
        __syncthreads();
    }
    if (kt) VX_KT(15);
    if (wv == 0 && lane == 0 && !ok) atomicOr(&a.st->fail[it], 1);
}

template <int kBsD>
__global__ __launch_bounds__(kSolveThreads) void k_sba_backsub(SBAArgs a, int it) {
    if (it > 0 && !a.st->active[it]) return;
    if (!a.st->lm[(it + 1) & 1].do_solve) return;
    extern __shared__ __attribute__((aligned(32))) double ys[];  // np: y, then x | back lists
    const int tid = threadIdx.x, wv = tid >> 6;
    const int comp = blockIdx.x;
    const int* hdr = a.comp_hdr + kHdrN * comp;
    const int nt = hdr[kHdrNt], np = 16 * nt;
    const int kq0 = a.comp_kf_ptr[comp], nc = 6 * (a.comp_kf_ptr[comp + 1] - kq0);
    double* L = a.L + a.comp_loff[comp];
    const double* Linv = a.Linv + a.comp_loff[comp];
    const int* tl = a.tl;
    const int* bptr = tl + hdr[kHdrBack];
    VX_KT(8);
    int* sbp = reinterpret_cast<int*>(ys + a.bs_np);
    back_substitute<kBsD>(L, Linv, np, nt, tl, bptr, ys, sbp, sbp + a.bs_nt + 1);
    VX_KT(9);
    for (int c = tid; c < nc; c += kSolveThreads) a.dx[6 * a.comp_kf[kq0 + c / 6] + c % 6] = ys[c];
    (void)wv;
    // (the clearing of the touched tiles: k_sba_update, over all its workgroups)
}

// ------------------------------------------------------------------------- k_sba_update
__global__ __launch_bounds__(kUpdThreads) void k_sba_update(SBAArgs a, int it) {
    if (it > 0 && !a.st->active[it]) return;
    // every component's factor tiles back to zero for the next assembly (k_sba_blocks writes only
    // the nonzero blocks) when this iteration factored: the copy lists spread over the launch's waves
    // — in k_sba_backsub's one workgroup per component these were ~2 MB of stores from one CU.  (A
    // failed factor counts: workgroup 0 below clears do_solve then, so the others go by the flag.)
    const LMVars v0 = a.st->lm[(it + 1) & 1];
    if (v0.do_solve || a.st->fail[it]) {
        const int gw = (blockIdx.x * kUpdThreads + threadIdx.x) >> 6, nw = gridDim.x * (kUpdThreads / 64);
        const d4 z = {0.0, 0.0, 0.0, 0.0};
        for (int comp = 0; comp < a.n_comp; ++comp) {
            const int* hdr = a.comp_hdr + kHdrN * comp;
            const int np = 16 * hdr[kHdrNt], ncp = hdr[kHdrNCopy];
            const int* cp = a.tl + hdr[kHdrCopy];
            double* L = a.L + a.comp_loff[comp];
            for (int t = gw; t < ncp; t += nw)
                store_acc(L + (long long)(16 * (cp[t] >> 16)) * np + 16 * (cp[t] & 0xffff), np, z);
        }
    }
    const LMVars v = v0;
    if (!v.do_solve) return;
    const int t = blockIdx.x * kUpdThreads + threadIdx.x;
    if (a.st->fail[it]) {  // a component's Cholesky failed: discard the step, damp harder
        if (t == 0) {
            LMVars& w = a.st->lm[(it + 1) & 1];
            w.lambda *= 10.0;
            w.eval_trial = 0;
            w.do_solve = 0;
        }
        return;
    }
    const int best = v.sel, trial = trial_idx(v.sel);
    if (t < a.nk) {
        const double* Tb = best < 0 ? a.pose0 : a.pose + (long long)best * a.nk * 8;
        double* Tt = a.pose + (long long)trial * a.nk * 8;
        double T[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) T[j] = Tb[8 * t + j];
        if (!(a.kf_flags[t] & 2)) {
            double d[6];
            bool fin = true, any = false;
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                d[j] = a.dx[6 * t + j];
                fin = fin && isfinite(d[j]);
                any = any || d[j] != 0.0;
            }
            // a zero step (a keyframe whose every observation is gated: rhs 0) is the identity: the pose
            // keeps its bits — se3_left_update would renormalise the quaternion, an ulp per accepted step
            if (fin && any) se3_left_update(d, T);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) Tt[8 * t + j] = T[j];
    }
    if (t < a.n_opt) {
        const double* Pb = (best < 0 ? a.lm0 : a.lm + (long long)best * a.n_opt * 4) + 4 * (long long)t;
        double* Pt = a.lm + (long long)trial * a.n_opt * 4 + 4 * (long long)t;
        const double* sys = a.lm_sys + (long long)t * kLmSys;
        double q[3] = {sys[6], sys[7], sys[8]};
        for (int o = a.lm_ptr[t]; o < a.lm_ptr[t + 1]; ++o) {
            const int k = a.obs_kf[o];
            if (a.kf_flags[k] & 2) continue;
            double W[18];
            load18(a.wy + (long long)o * kWy, W);
            const double* d = a.dx + 6 * k;
            double dd[6];
#pragma unroll
            for (int r = 0; r < 6; ++r) dd[r] = d[r];
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int r = 0; r < 6; ++r) q[c] -= W[3 * r + c] * dd[r];
        }
        const double dp0 = sys[0] * q[0] + sys[1] * q[1] + sys[2] * q[2];
        const double dp1 = sys[1] * q[0] + sys[3] * q[1] + sys[4] * q[2];
        const double dp2 = sys[2] * q[0] + sys[4] * q[1] + sys[5] * q[2];
        const bool fin = isfinite(dp0) && isfinite(dp1) && isfinite(dp2);
        Pt[0] = Pb[0] + (fin ? dp0 : 0.0);
        Pt[1] = Pb[1] + (fin ? dp1 : 0.0);
        Pt[2] = Pb[2] + (fin ? dp2 : 0.0);
        Pt[3] = 0.0;
    }
}

template <class T>
int upload(vx_ctx* c, DevBuf& d, const std::vector<T>& h) {
    VX_HIP(c, d.ensure(std::max<size_t>(1, h.size()) * sizeof(T)));
    if (!h.empty()) VX_HIP(c, hipMemcpy(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return VX_OK;
}

}  // namespace
}  // namespace vx

// (struct vx_sba_plan: sba_plan.hpp)

namespace vx {
namespace {

int solve_panel_slots(int np, int max_panel);

SBAArgs make_args(vx_sba_plan* p) {
    SBAArgs a{};
    a.nk = p->nk;
    a.n_opt = p->n_opt;
    a.n_lm = p->n_lm;
    a.n_oo = p->n_oo;
    a.n_obs = p->n_obs;
    a.max_iter = p->opt.max_iterations;
    a.min_point_obs = p->opt.min_point_observations;
    a.huber = p->opt.huber_delta;
    a.max_err = p->opt.max_reproj_error;
    a.lambda0 = p->opt.lambda_init;
    a.rel_tol = p->opt.rel_tol;
    {
        const double d = p->opt.huber_delta, me = p->opt.max_reproj_error;
        a.rho_gate = me <= d ? me * me : 2.0 * d * me - d * d;
    }
    a.pose0 = p->pose0.as<double>();
    a.pose = p->pose.as<double>();
    a.intr = p->intr.as<double>();
    a.kf_flags = p->kf_flags.as<int>();
    a.kf_comp = p->kf_comp.as<int>();
    a.kf_local = p->kf_local.as<int>();
    a.lm0 = p->lm0.as<double>();
    a.lm = p->lm.as<double>();
    a.obs_uv = p->obs_uv.as<double2>();
    a.obs_kf = p->obs_kf.as<int>();
    a.obs_lm = p->obs_lm.as<int>();
    a.lm_ptr = p->lm_ptr.as<int>();
    a.lm_blk = p->lm_blk.as<int>();
    a.kf_ptr = p->kf_ptr.as<int>();
    a.kf_obs = p->kf_obs.as<int>();
    a.blk_ij = p->blk_ij.as<int2>();
    a.blk_ptr = p->blk_ptr.as<int>();
    a.pairs = p->pairs.as<int2>();
    a.comp_kf_ptr = p->comp_kf_ptr.as<int>();
    a.comp_kf = p->comp_kf.as<int>();
    a.comp_off = p->comp_off.as<long long>();
    a.comp_loff = p->comp_loff.as<long long>();
    a.comp_np = p->comp_np.as<int>();
    a.comp_hdr = p->comp_hdr.as<int>();
    a.n_comp = p->n_comp;
    a.tl = p->tl.as<int>();
    a.wy = p->wy.as<double>();
    a.lm_sys = p->lm_sys.as<double>();
    a.diag_split = p->diag_split;
    a.bpart = p->bpart.as<double>();
    a.red = p->red.as<double>();
    a.red_sum = p->shard_count > 1 ? p->red_sum.as<double>() : p->red.as<double>();
    a.s_total = p->l_total;
    a.L = const_cast<double*>(a.red_sum);  // component matrices are factored in place
    a.Linv = p->Linv.as<double>();
    a.dx = p->dx.as<double>();
    a.st = p->state.as<SBAState>();
    a.panel_slots = solve_panel_slots(p->max_np, p->max_panel);
    a.fac_steps = p->fac_steps.as<int>();
    a.fac_nk = std::max(p->max_nt - 1, 1);
    a.fac_pairs = p->fac_pairs.as<int>();
    a.fac_np = std::max(p->max_pairs, 1);
    a.fac_blks = p->fac_blks.as<int>();
    a.fac_nb = std::max(p->max_blks, 1);
    a.bs_np = p->max_np;
    a.bs_nt = std::max(p->max_nt, 1);
    return a;
}

int find_root(std::vector<int>& par, int x) {
    while (par[x] != x) {
        par[x] = par[par[x]];
        x = par[x];
    }
    return x;
}

// Host threads of the plan build: at most 16 (the CPU share of one GPU on the target node),
// $VX_SBA_PLAN_THREADS overrides (1: serial).
int plan_threads() {
    static const int t = [] {
        if (const char* e = std::getenv("VX_SBA_PLAN_THREADS")) return std::max(1, std::atoi(e));
        return (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    }();
    return t;
}
// fn(t) for t in [0, T) on T threads (fn(0) on the caller); every t writes disjoint data
template <class F>
void run_threads(int T, F&& fn) {
    if (T <= 1) {
        fn(0);
        return;
    }
    std::vector<std::thread> th;
    th.reserve(T - 1);
    for (int t = 1; t < T; ++t) th.emplace_back([&fn, t] { fn(t); });
    fn(0);
    for (auto& x : th) x.join();
}

// select_window (ba_common.hpp, SelectKeyFrames + the optimised landmark set) keeping its landmark
// lookups for the observation pass: feat_l[fbase[r] + i] = map index of window keyframe r's feature i
// (features with has_landmark set and a landmark in the map; -1 otherwise), kept for the
// observation pass.  Same window, same opt_all.
void select_window_lookup(const vx_map_view* m, uint64_t ref_kf_id, int has_ref, int window_size,
                          int min_point_observations, Window& w, std::vector<int64_t>& fbase,
                          std::vector<int>& feat_l) {
    w = Window{};
    if (!m || m->n_kf <= 0) return;
    std::vector<int> order(m->n_kf);
    for (int i = 0; i < m->n_kf; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](int x, int y) { return m->kf_id[x] < m->kf_id[y]; });
    const int window = std::max(1, window_size);
    const uint64_t max_id = has_ref ? ref_kf_id : m->kf_id[order.back()];
    for (int i = m->n_kf - 1; i >= 0 && (int)w.win.size() < window; --i) {
        if (m->kf_id[order[i]] > max_id) continue;
        w.win.push_back(order[i]);
    }
    std::reverse(w.win.begin(), w.win.end());
    if (w.win.size() < 2) return;
    w.lm_by_id.build(m->lm_id, m->n_lm);
    const int nk = (int)w.win.size();
    fbase.assign(nk + 1, 0);
    for (int r = 0; r < nk; ++r) fbase[r + 1] = fbase[r] + (m->kf_feat_ptr[w.win[r] + 1] - m->kf_feat_ptr[w.win[r]]);
    feat_l.assign((size_t)fbase[nk], -1);
    // (serial: on 16 threads this pass measured no faster at C5 — the hash build, the sort and the
    // filter dominate the stage — and thread start-up made C3 slower)
    for (int r = 0; r < nk; ++r) {
        const int64_t f0 = m->kf_feat_ptr[w.win[r]], f1 = m->kf_feat_ptr[w.win[r] + 1];
        for (int64_t f = f0; f < f1; ++f)
            if (m->feat_flags[f] & 1) feat_l[(size_t)(fbase[r] + (f - f0))] = w.lm_by_id.get(m->feat_lm_id[f]);
    }
    // landmarks referenced by a window feature, then the filter, in map-index order
    std::vector<uint8_t> ref((size_t)std::max(m->n_lm, 1), 0);
    for (const int l : feat_l)
        if (l >= 0) ref[l] = 1;
    for (int l = 0; l < m->n_lm; ++l) {
        if (!ref[l] || m->lm_bad[l]) continue;
        if (m->lm_obs_ptr[l + 1] - m->lm_obs_ptr[l] < (int64_t)min_point_observations) continue;
        w.opt_all.push_back(l);
    }
    if (!w.opt_all.empty()) w.status = 0;
}

int build_sba_plan(vx_ctx* c, const vx_map_view* m, uint64_t ref_kf_id, int has_ref, vx_sba_plan* p) {
    const vx_sba_options& o = p->opt;
    static const bool timing = std::getenv("VX_SBA_PLAN_TIMING") != nullptr;
    auto t_last = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!timing) return;
        const auto t = std::chrono::steady_clock::now();
        std::fprintf(stderr, "sba plan %-12s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t - t_last).count());
        t_last = t;
    };
    p->status = 1;
    Window W;
    std::vector<int64_t> wfbase;  // window feature ranges and their landmark lookups
    std::vector<int> wfeat_l;
    select_window_lookup(m, ref_kf_id, has_ref, o.window_size, o.min_point_observations, W, wfbase, wfeat_l);
    p->n_window_kf = (int)W.win.size();
    p->n_landmarks_global = (int)W.opt_all.size();
    if (W.status != 0) return VX_OK;
    lap("window");
    p->status = 0;
    const std::vector<int>& win = W.win;
    const int nk = (int)win.size();
    p->nk = nk;
    p->kf_map_idx = win;
    auto owned = [&](int l) {
        return p->shard_count <= 1 ||
               (int)(splitmix64(m->lm_id[l]) % (uint64_t)p->shard_count) == p->shard_rank;
    };
    std::vector<int> slot_of(m->n_lm, -1);
    p->lm_map_idx.clear();
    for (int l : W.opt_all)
        if (owned(l)) {
            slot_of[l] = (int)p->lm_map_idx.size();
            p->lm_map_idx.push_back(l);
        }
    const int n_opt = (int)p->lm_map_idx.size();
    p->n_opt = n_opt;

    // ---- keyframes and observations (the pose stage's set, local_ba.cpp:126-138)
    std::vector<double> pose0((size_t)nk * 8, 0.0), intr((size_t)nk * 4, 0.0);
    std::vector<int> flags(nk, 0);
    // pass 1: the pose-stage observations in keyframe-major order, slots assigned as met
    struct HObs { int kf, slot; double u, v; };
    std::vector<HObs> all;
    all.reserve(4096);
    // the window features' landmark of each pose-stage observation (or -1): the hash probes, in
    // parallel over keyframes; then one sequential pass numbers the fixed landmarks as met
    std::vector<int64_t> fbase(nk + 1, 0);
    for (int r = 0; r < nk; ++r) {
        const int k = win[r];
        for (int j = 0; j < 7; ++j) pose0[8 * r + j] = m->kf_pose[7 * k + j];
        for (int j = 0; j < 4; ++j) intr[4 * r + j] = m->kf_intr[4 * k + j];
        const bool cam = m->kf_has_cam[k] != 0;
        flags[r] = (cam ? 1 : 0) | ((r < o.fixed_keyframes || !cam) ? 2 : 0);
        fbase[r + 1] = fbase[r] + (cam ? m->kf_feat_ptr[k + 1] - m->kf_feat_ptr[k] : 0);
    }
    std::vector<int> feat_l((size_t)fbase[nk]);
    for (int r = 0; r < nk; ++r) {  // (the lookups from select_window_lookup; the pose-stage checks)
        if (!(flags[r] & 1)) continue;
        const int64_t f0 = m->kf_feat_ptr[win[r]];
        for (int64_t i = 0; i < fbase[r + 1] - fbase[r]; ++i) {
            const uint8_t fl = m->feat_flags[f0 + i];
            int l = (fl & 2) ? -1 : wfeat_l[(size_t)(wfbase[r] + i)];
            if (l >= 0 && (m->lm_bad[l] || !owned(l))) l = -1;
            feat_l[(size_t)(fbase[r] + i)] = l;
        }
    }
    lap("obs lookups");
    for (int r = 0; r < nk; ++r) {
        if (!(flags[r] & 1)) continue;
        const int64_t f0 = m->kf_feat_ptr[win[r]];
        for (int64_t i = fbase[r]; i < fbase[r + 1]; ++i) {
            const int l = feat_l[(size_t)i];
            if (l < 0) continue;
            if (slot_of[l] < 0) {  // a landmark the pose stage sees but BA does not optimise
                slot_of[l] = (int)p->lm_map_idx.size();
                p->lm_map_idx.push_back(l);
            }
            const int64_t f = f0 + (i - fbase[r]);
            all.push_back(HObs{r, slot_of[l], m->feat_uv[2 * f], m->feat_uv[2 * f + 1]});
        }
    }
    p->n_lm = (int)p->lm_map_idx.size();
    lap("obs slots");
    // pass 2: stable counting sort into landmark-major order for the optimised slots (keyframe
    // order within a landmark), then the fixed landmarks' observations in keyframe-major order
    std::vector<int> lptr(n_opt + 1, 0);
    for (const HObs& ob : all)
        if (ob.slot < n_opt) ++lptr[ob.slot + 1];
    for (int sl = 0; sl < n_opt; ++sl) {
        if (lptr[sl + 1] > kLmThreads)
            return set_error(c, VX_ERR_INVALID, "landmark with %d observations in the window (max %d)", lptr[sl + 1],
                             kLmThreads);
        lptr[sl + 1] += lptr[sl];
    }
    const int n_oo = lptr[n_opt];
    std::vector<double2> ouv(all.size());
    std::vector<int> okf(all.size()), olm(all.size());
    {
        std::vector<int> fill(lptr.begin(), lptr.end() - 1);
        int fo = n_oo;
        for (const HObs& ob : all) {
            const int at = ob.slot < n_opt ? fill[ob.slot]++ : fo++;
            ouv[at] = make_double2(ob.u, ob.v);
            okf[at] = ob.kf;
            olm[at] = ob.slot;
        }
    }
    p->n_oo = n_oo;
    p->n_obs = (int)okf.size();
    lap("obs sort");
    std::vector<double> lm0((size_t)std::max(p->n_lm, 1) * 4, 0.0);
    for (int s = 0; s < p->n_lm; ++s)
        for (int j = 0; j < 3; ++j) lm0[4 * s + j] = m->lm_pos[3 * p->lm_map_idx[s] + j];
    // k_sba_lm workgroups: whole landmarks, <= kLmThreads observations and landmarks each
    std::vector<int> blk{0};
    {
        int n_o = 0, n_l = 0;
        for (int s = 0; s < n_opt; ++s) {
            const int cnt = lptr[s + 1] - lptr[s];
            if (n_l + 1 > kLmThreads || n_o + cnt > kLmThreads) {
                blk.push_back(s);
                n_o = n_l = 0;
            }
            n_o += cnt;
            ++n_l;
        }
        blk.push_back(n_opt);
    }
    p->n_lm_blocks = (int)blk.size() - 1;
    // keyframe-major observation lists
    std::vector<int> kptr(nk + 1, 0), kobs(p->n_obs);
    for (int ob = 0; ob < p->n_obs; ++ob) kptr[okf[ob] + 1]++;
    for (int r = 0; r < nk; ++r) kptr[r + 1] += kptr[r];
    {
        std::vector<int> fill(kptr.begin(), kptr.end() - 1);
        for (int ob = 0; ob < p->n_obs; ++ob) kobs[fill[okf[ob]]++] = ob;
    }

    lap("observations");
    // ---- blocks of the reduced system: every keyframe's diagonal block, then the off-diagonal
    // (i > j) blocks of co-observing free keyframes, each with its co-observation pairs
    // Every (i >= j) pair of free keyframes co-observing a landmark contributes the pair of its two
    // observations to block (i, j).  Blocks: the nk diagonal blocks in keyframe order, then the
    // non-empty off-diagonal blocks by (i, j); pairs inside a block by (o1, o2).  The pairs are
    // generated in (o1, o2) order, so a two-pass counting sort by block key keeps that order; the
    // passes run on T threads over contiguous slot ranges, thread t's pairs of a block placed after
    // those of threads < t (the serial order exactly).
    const int64_t nkey = (int64_t)nk * nk;
    // (threads: one per 8192 slots — thread start-up costs tens of us — and at most 64 MB of
    // per-thread key counts)
    const int T = std::max(1, std::min({plan_threads(), n_opt / 8192,
                                        (int)std::max<int64_t>(1, ((int64_t)1 << 24) / std::max<int64_t>(nkey, 1))}));
    auto for_pairs = [&](int s0, int s1, auto&& emit) {
        for (int sl = s0; sl < s1; ++sl)
            for (int a1 = lptr[sl]; a1 < lptr[sl + 1]; ++a1) {
                const int i = okf[a1];
                if (flags[i] & 2) continue;
                for (int a2 = lptr[sl]; a2 < lptr[sl + 1]; ++a2) {
                    const int j = okf[a2];
                    if ((flags[j] & 2) || j > i) continue;
                    emit((int64_t)i * nk + j, a1, a2);
                }
            }
    };
    std::vector<int> sb(T + 1);  // thread t: slots [sb[t], sb[t + 1]), balanced by observations
    for (int t = 0; t <= T; ++t)
        sb[t] = (int)(std::lower_bound(lptr.begin(), lptr.end(), (int)((int64_t)n_oo * t / T)) - lptr.begin());
    sb[0] = 0;
    sb[T] = n_opt;
    for (int t = 1; t < T; ++t) sb[t] = std::min(std::max(sb[t], sb[t - 1]), n_opt);
    std::vector<std::vector<int>> kc(T, std::vector<int>((size_t)nkey, 0));
    run_threads(T, [&](int t) { for_pairs(sb[t], sb[t + 1], [&](int64_t key, int, int) { ++kc[t][key]; }); });
    std::vector<int> kcnt((size_t)nkey, 0);
    for (int t = 0; t < T; ++t)
        for (int64_t key = 0; key < nkey; ++key) kcnt[key] += kc[t][key];
    // Sharded: the block structure is the whole window's, the same on every rank (the all-reduce
    // sums the ranks' component matrices element by element, and the symbolic factorisation must
    // cover every block any rank fills); a rank's own pairs fill part of it, the rest of its blocks
    // stay empty.  The off-diagonal blocks of the co-observations of every optimised landmark.
    std::vector<char> gblk;
    if (p->shard_count > 1) {
        gblk.assign((size_t)nkey, 0);
        std::vector<char> is_opt(m->n_lm, 0);
        for (int l : W.opt_all) is_opt[l] = 1;
        std::vector<int> head(m->n_lm, -1), nxt, row;  // per landmark: its observations' keyframe rows
        for (int r = 0; r < nk; ++r) {
            if (!(flags[r] & 1) || (flags[r] & 2)) continue;  // (free keyframes only form blocks)
            const int64_t f0 = m->kf_feat_ptr[win[r]];
            for (int64_t i = 0; i < fbase[r + 1] - fbase[r]; ++i) {
                if (m->feat_flags[f0 + i] & 2) continue;
                const int l = wfeat_l[(size_t)(wfbase[r] + i)];
                if (l < 0 || m->lm_bad[l] || !is_opt[l]) continue;
                nxt.push_back(head[l]);
                row.push_back(r);
                head[l] = (int)row.size() - 1;
            }
        }
        for (int l : W.opt_all)
            for (int e1 = head[l]; e1 >= 0; e1 = nxt[e1])
                for (int e2 = nxt[e1]; e2 >= 0; e2 = nxt[e2]) {
                    const int i = std::max(row[e1], row[e2]), j = std::min(row[e1], row[e2]);
                    if (i != j) gblk[(size_t)i * nk + j] = 1;
                }
    }
    std::vector<int2> bij;
    std::vector<int> bptr{0};
    std::vector<int> kpos((size_t)nkey, -1);  // output offset of each block key
    int64_t total = 0;
    for (int r = 0; r < nk; ++r) {
        const int64_t key = (int64_t)r * nk + r;
        bij.push_back(make_int2(r, r));
        kpos[key] = (int)total;
        total += kcnt[key];
        bptr.push_back((int)total);
    }
    for (int64_t key = 0; key < nkey; ++key) {
        const int i = (int)(key / nk), j = (int)(key % nk);
        if (i == j || (kcnt[key] == 0 && (gblk.empty() || !gblk[key]))) continue;
        bij.push_back(make_int2(i, j));
        kpos[key] = (int)total;
        total += kcnt[key];
        bptr.push_back((int)total);
    }
    for (int64_t key = 0; key < nkey; ++key) {  // kc[t][key] := thread t's first output position
        int run = kpos[key];
        for (int t = 0; t < T; ++t) {
            const int c = kc[t][key];
            kc[t][key] = run;
            run += c;
        }
    }
    std::vector<int2> prs((size_t)total);
    run_threads(T, [&](int t) {
        for_pairs(sb[t], sb[t + 1], [&](int64_t key, int a1, int a2) { prs[kc[t][key]++] = make_int2(a1, a2); });
    });
    p->n_blocks = (int)bij.size();
    p->n_pairs = (int64_t)prs.size();
    lap("blocks");
    VX_HIP(c, hipSetDevice(c->device));
    int rc;
    if ((rc = upload(c, p->pose0, pose0))) return rc;
    if ((rc = upload(c, p->intr, intr))) return rc;
    if ((rc = upload(c, p->lm0, lm0))) return rc;
    if ((rc = upload(c, p->obs_uv, ouv))) return rc;
    if ((rc = upload(c, p->obs_kf, okf))) return rc;
    if ((rc = upload(c, p->obs_lm, olm))) return rc;
    if ((rc = upload(c, p->lm_ptr, lptr))) return rc;
    if ((rc = upload(c, p->lm_blk, blk))) return rc;
    if ((rc = upload(c, p->kf_ptr, kptr))) return rc;
    if ((rc = upload(c, p->kf_obs, kobs))) return rc;
    if ((rc = upload(c, p->blk_ij, bij))) return rc;
    if ((rc = upload(c, p->blk_ptr, bptr))) return rc;
    if ((rc = upload(c, p->pairs, prs))) return rc;
    rc = sba_plan_finish(c, p, flags, bij);
    lap("finish");
    return rc;
}

}  // namespace

int sba_plan_finish(vx_ctx* c, vx_sba_plan* p, const std::vector<int>& flags, const std::vector<int2>& bij,
                    const PlanClock* clk) {
    const int nk = p->nk, n_opt = p->n_opt;
    auto mark = [clk](const char* w) {
        if (clk) clk->mark(w);
    };

    // ---- connected components of the free keyframes' covisibility graph
    // (over the off-diagonal blocks: two free keyframes share a block exactly when a landmark's
    // observations join them, so the components are those of the landmark walk; numbered below
    // by their first keyframe, whatever the union order)
    std::vector<int> par(nk);
    std::iota(par.begin(), par.end(), 0);
    for (size_t b = (size_t)nk; b < bij.size(); ++b) par[find_root(par, bij[b].x)] = find_root(par, bij[b].y);
    std::vector<int> kcomp(nk, -1), klocal(nk, 0), root_comp(nk, -1);
    p->comp_kf_ptr_h.assign(1, 0);
    p->comp_kf_h.clear();
    std::vector<std::vector<int>> comps;
    for (int r = 0; r < nk; ++r) {
        if (flags[r] & 2) continue;
        const int rt = find_root(par, r);
        if (root_comp[rt] < 0) {
            root_comp[rt] = (int)comps.size();
            comps.emplace_back();
        }
        kcomp[r] = root_comp[rt];
        klocal[r] = (int)comps[kcomp[r]].size();
        comps[kcomp[r]].push_back(r);
    }
    p->n_comp = (int)comps.size();
    p->comp_np_h.clear();
    p->comp_off_h.clear();
    std::vector<long long> loff;
    long long soff = 0, lo = 0;
    p->max_np = 16;
    for (const auto& cc : comps) {
        if ((int)cc.size() > kMaxCompKf)
            return set_error(c, VX_ERR_INVALID, "covisibility component of %d keyframes (dense solve max %d)",
                             (int)cc.size(), kMaxCompKf);
        const int np = std::max(16, (6 * (int)cc.size() + 15) / 16 * 16);
        p->comp_np_h.push_back(np);
        p->comp_off_h.push_back(soff);
        loff.push_back(lo);
        soff += (long long)np * np;
        lo += (long long)(np + 16) * np;
        p->max_np = std::max(p->max_np, np);
        for (int r : cc) p->comp_kf_h.push_back(r);
        p->comp_kf_ptr_h.push_back((int)p->comp_kf_h.size());
    }
    p->s_total = soff;
    p->l_total = lo;
    p->comp_loff_h = loff;
    mark("sba components");

    // ---- symbolic tile factorisation per component: which 16 x 16 tiles of L are nonzero (the
    // pattern of S's blocks plus Cholesky fill), and per step the panel / trailing-update / back-
    // substitution tile lists k_sba_solve walks.  A sliding window's covisibility is banded, so
    // most tiles of the dense matrix are never touched.
    std::vector<int> hdr((size_t)kHdrN * std::max(p->n_comp, 1), 0), tlist;
    p->n_lfactor_tiles = p->n_trail_updates = p->n_trail_rhs = 0;
    p->max_panel = 1;
    p->max_nt = p->max_trail_rest = 0;
    p->max_pairs = 0;
    p->max_blks = p->max_blk_trail = p->max_blk_la = 0;
    p->blk_ok = p->n_comp > 0;
    p->max_back = 0;
    std::vector<std::vector<int>> pair_desc(std::max(p->n_comp, 1)), blk_desc(std::max(p->n_comp, 1));
    {
        std::vector<std::vector<std::pair<int, int>>> cblk(p->n_comp);
        for (const int2& b : bij) {
            const int cc = kcomp[b.x];
            if (cc >= 0 && kcomp[b.y] == cc) cblk[cc].push_back({klocal[b.x], klocal[b.y]});
        }
        for (int cc = 0; cc < p->n_comp; ++cc) {
            const int nt = p->comp_np_h[cc] / 16;
            std::vector<char> nz((size_t)nt * nt, 0);
            auto NZ = [&](int i, int j) -> char& { return nz[(size_t)i * nt + j]; };
            for (int t = 0; t < nt; ++t) NZ(t, t) = 1;
            for (auto& b : cblk[cc])
                for (int r = 6 * b.first; r < 6 * b.first + 6; r += 5)
                    for (int q = 6 * b.second; q < 6 * b.second + 6; q += 5) {
                        const int ti = std::max(r, q) / 16, tj = std::min(r, q) / 16;
                        NZ(ti, tj) = 1;
                    }
            for (int k = 0; k < nt; ++k)
                for (int i = k + 1; i < nt; ++i)
                    if (NZ(i, k))
                        for (int j = k + 1; j <= i; ++j)
                            if (NZ(j, k)) NZ(i, j) = 1;
            int* h = hdr.data() + (size_t)kHdrN * cc;
            h[kHdrNt] = nt;
            h[kHdrCopy] = (int)tlist.size();
            for (int i = 0; i < nt; ++i)
                for (int j = 0; j <= i; ++j)
                    if (NZ(i, j)) tlist.push_back(i << 16 | j);
            for (int j = 0; j < nt; ++j) tlist.push_back(nt << 16 | j);
            h[kHdrNCopy] = (int)tlist.size() - h[kHdrCopy];
            p->n_lfactor_tiles += h[kHdrNCopy];
            // panel lists
            h[kHdrPanel] = (int)tlist.size();
            const int pp = (int)tlist.size();
            tlist.resize(tlist.size() + nt + 1);
            for (int k = 0; k < nt; ++k) {
                tlist[pp + k] = (int)tlist.size();
                for (int i = k + 1; i < nt; ++i)
                    if (NZ(i, k)) tlist.push_back(i);
                tlist.push_back(nt);
                p->max_panel = std::max(p->max_panel, (int)tlist.size() - tlist[pp + k]);
            }
            tlist[pp + nt] = (int)tlist.size();
            // trailing-update lists; per step k the tiles of column k + 1 first (the look-ahead
            // column the multi-workgroup factorisation updates and factors in the same launch), then
            // the rest; every tile is updated once per step, so the order inside a step is free
            h[kHdrTrail] = (int)tlist.size();
            const int tp = (int)tlist.size();
            tlist.resize(tlist.size() + nt + 1);
            std::vector<int> split(nt, 0);
            for (int k = 0; k < nt; ++k) {
                tlist[tp + k] = (int)tlist.size();
                if (k + 1 < nt && NZ(k + 1, k)) {
                    for (int i = k + 1; i < nt; ++i)
                        if (NZ(i, k)) tlist.push_back(i << 16 | (k + 1));
                    tlist.push_back(nt << 16 | (k + 1));
                    ++p->n_trail_rhs;
                }
                split[k] = (int)tlist.size();
                for (int i = k + 1; i < nt; ++i)
                    if (NZ(i, k))
                        for (int j = k + 2; j <= i; ++j)
                            if (NZ(j, k)) tlist.push_back(i << 16 | j);
                for (int j = k + 2; j < nt; ++j)
                    if (NZ(j, k)) {
                        tlist.push_back(nt << 16 | j);
                        ++p->n_trail_rhs;
                    }
                p->n_trail_updates += (int)tlist.size() - tlist[tp + k];
                p->max_trail_rest = std::max(p->max_trail_rest, (int)tlist.size() - split[k]);
            }
            tlist[tp + nt] = (int)tlist.size();
            h[kHdrTrailSplit] = (int)tlist.size();
            tlist.insert(tlist.end(), split.begin(), split.end());
            p->max_nt = std::max(p->max_nt, nt);
            // back-substitution lists: tile columns m < k of row k
            h[kHdrBack] = (int)tlist.size();
            const int bp = (int)tlist.size();
            tlist.resize(tlist.size() + nt + 1);
            for (int k = 0; k < nt; ++k) {
                tlist[bp + k] = (int)tlist.size();
                for (int m2 = 0; m2 < k; ++m2)
                    if (NZ(k, m2)) tlist.push_back(m2);
            }
            tlist[bp + nt] = (int)tlist.size();
            p->max_back = std::max(p->max_back, tlist[bp + nt] - tlist[bp]);
            // the two-column schedule's lists (k_sba_fac_pair): launch t applies steps s0 = 2t and
            // s0 + 1 (entries i << 16 | c << 2 | mask) — phase 1: columns c0 = 2t + 2, c0 + 1; phase 2:
            // step c0 on column c0 + 1 (one-step entries); rest: the columns beyond
            auto mask_of = [&](int i, int c, int s0) {
                const bool a0 = (i == nt || NZ(i, s0)) && NZ(c, s0);
                const bool a1 = (i == nt || NZ(i, s0 + 1)) && NZ(c, s0 + 1);
                return (a0 ? 1 : 0) | (a1 ? 2 : 0);
            };
            auto& pd = pair_desc[cc];
            for (int c0 = 2; c0 < nt; c0 += 2) {
                const int s0 = c0 - 2, c1 = c0 + 1;
                int d[16] = {0};
                const unsigned long long lo = (unsigned long long)loff[cc];
                d[0] = (int)(unsigned)(lo & 0xffffffffull);
                d[1] = (int)(unsigned)(lo >> 32);
                d[2] = (int)tlist.size();
                for (int c = c0; c <= std::min(c1, nt - 1); ++c)
                    for (int i = c; i <= nt; ++i) {
                        const int mk = mask_of(i, c, s0);
                        if (mk) tlist.push_back(i << 16 | c << 2 | mk);
                    }
                d[3] = (int)tlist.size();
                d[4] = (int)tlist.size();
                if (c1 < nt && NZ(c1, c0)) {
                    for (int i = c1; i < nt; ++i)
                        if (NZ(i, c0)) tlist.push_back(i << 16 | c1);
                    tlist.push_back(nt << 16 | c1);
                }
                d[5] = (int)tlist.size();
                d[6] = (int)tlist.size();
                for (int j = c1 + 1; j < nt; ++j)
                    for (int i = j; i <= nt; ++i) {
                        const int mk = mask_of(i, j, s0);
                        if (mk) tlist.push_back(i << 16 | j << 2 | mk);
                    }
                d[7] = (int)tlist.size();
                d[8] = tlist[h[kHdrPanel] + c0];
                d[9] = tlist[h[kHdrPanel] + c0 + 1];
                d[10] = c1 < nt ? tlist[h[kHdrPanel] + c1] : 0;
                d[11] = c1 < nt ? tlist[h[kHdrPanel] + c1 + 1] : 0;
                d[12] = nt;
                d[13] = c0;
                pd.insert(pd.end(), d, d + 16);
            }
            p->max_pairs = std::max(p->max_pairs, (int)(pd.size() / 16));
            // the blocked factor (k_sba_fac_blk): blocks of up to kFbW columns whose tiles (the
            // diagonal, the panel rows, the rhs row) fit kFbCap LDS tiles; per block its tile list
            // (column-major, rows ascending), then per launch t >= 1 the tiles beyond block t that block
            // t - 1's steps update (step mask bit s: NZ(i, K0p + s) and NZ(j, K0p + s), the rhs row
            // always nonzero)
            {
                auto col_tiles = [&](int c) { return tlist[h[kHdrPanel] + c + 1] - tlist[h[kHdrPanel] + c] + 1; };
                std::vector<int> bk0, bw, bb, be;
                for (int c = 0; c < nt && p->blk_ok;) {
                    int w = 0, tiles = 0;
                    while (c + w < nt && w < kFbW && tiles + col_tiles(c + w) <= kFbCap) tiles += col_tiles(c + w++);
                    if (w == 0) {
                        p->blk_ok = false;  // one column's panel exceeds the block LDS
                        break;
                    }
                    bk0.push_back(c);
                    bw.push_back(w);
                    bb.push_back((int)tlist.size());
                    for (int q = c; q < c + w; ++q) {
                        tlist.push_back(q << 16 | q);
                        for (int x = tlist[h[kHdrPanel] + q]; x < tlist[h[kHdrPanel] + q + 1]; ++x)
                            tlist.push_back(tlist[x] << 16 | q);
                    }
                    be.push_back((int)tlist.size());
                    c += w;
                }
                auto& bd = blk_desc[cc];
                const unsigned long long lo = (unsigned long long)loff[cc];
                for (size_t b = 0; p->blk_ok && b < bk0.size(); ++b) {
                    int d[16] = {0};
                    d[0] = (int)(unsigned)(lo & 0xffffffffull);
                    d[1] = (int)(unsigned)(lo >> 32);
                    d[2] = bk0[b];
                    d[3] = bw[b];
                    d[4] = bb[b];
                    d[5] = be[b];
                    d[12] = nt;
                    if (b > 0) {
                        const int k0 = bk0[b - 1], wp = bw[b - 1];
                        d[6] = bb[b - 1];
                        d[7] = be[b - 1];
                        d[8] = k0;
                        d[9] = wp;
                        d[10] = (int)tlist.size();
                        for (int j = bk0[b] + bw[b]; j < nt; ++j)
                            for (int i = j; i <= nt; ++i) {
                                int mk = 0;
                                for (int sx = 0; sx < wp; ++sx)
                                    if ((i == nt || NZ(i, k0 + sx)) && NZ(j, k0 + sx)) mk |= 1 << sx;
                                if (mk) tlist.push_back(i << 16 | j << 4 | mk);
                            }
                        d[11] = (int)tlist.size();
                        p->max_blk_trail = std::max(p->max_blk_trail, d[11] - d[10]);
                        // block t's own tiles with block t - 1's steps (the look-ahead when it runs as
                        // a launch of its own, k_sba_fac_upd)
                        d[13] = (int)tlist.size();
                        for (int x = bb[b]; x < be[b]; ++x) {
                            const int i = tlist[x] >> 16, j = tlist[x] & 0xffff;
                            int mk = 0;
                            for (int sx = 0; sx < wp; ++sx)
                                if ((i == nt || NZ(i, k0 + sx)) && NZ(j, k0 + sx)) mk |= 1 << sx;
                            if (mk) tlist.push_back(i << 16 | j << 4 | mk);
                        }
                        d[14] = (int)tlist.size();
                        p->max_blk_la = std::max(p->max_blk_la, d[14] - d[13]);
                    }
                    bd.insert(bd.end(), d, d + 16);
                }
                p->max_blks = std::max(p->max_blks, (int)(bd.size() / 16));
            }
        }
    }

    mark("sba symbolic factorisation");
    // the multi-workgroup factor's per-launch descriptors (FacStep: 8 ints per component and step)
    {
        const int fk = std::max(p->max_nt - 1, 1);
        p->fac_steps_h.assign((size_t)8 * fk * std::max(p->n_comp, 1), 0);
        for (int cc = 0; cc < p->n_comp; ++cc) {
            const int* h = hdr.data() + (size_t)kHdrN * cc;
            const int nt = h[kHdrNt];
            for (int k = 0; k + 1 < nt; ++k) {
                int* d = p->fac_steps_h.data() + 8 * ((size_t)cc * fk + k);
                const unsigned long long lo = (unsigned long long)loff[cc];
                d[0] = (int)(unsigned)(lo & 0xffffffffull);
                d[1] = (int)(unsigned)(lo >> 32);
                d[2] = tlist[h[kHdrTrail] + k];
                d[3] = tlist[h[kHdrTrailSplit] + k];
                d[4] = tlist[h[kHdrTrail] + k + 1];
                d[5] = tlist[h[kHdrPanel] + k + 1];
                d[6] = tlist[h[kHdrPanel] + k + 2];
                d[7] = nt;
            }
        }
    }
    {
        const int fp = std::max(p->max_pairs, 1);
        p->fac_pairs_h.assign((size_t)16 * fp * std::max(p->n_comp, 1), 0);
        for (int cc = 0; cc < p->n_comp; ++cc)
            std::copy(pair_desc[cc].begin(), pair_desc[cc].end(), p->fac_pairs_h.begin() + (size_t)16 * fp * cc);
    }
    {
        const int fb = std::max(p->max_blks, 1);
        p->fac_blks_h.assign((size_t)16 * fb * std::max(p->n_comp, 1), 0);
        for (int cc = 0; p->blk_ok && cc < p->n_comp; ++cc)
            std::copy(blk_desc[cc].begin(), blk_desc[cc].end(), p->fac_blks_h.begin() + (size_t)16 * fb * cc);
    }
    VX_HIP(c, hipSetDevice(c->device));
    // the tables through one pinned staging block: one copy to the device, one launch scattering it
    // into the plan's buffers (a rebuild synchronises before it rewrites the block)
    {
        auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
        size_t tot = 0;
        auto add = [&](const auto& v) { tot += pad(std::max<size_t>(1, v.size()) * sizeof(v[0])); };
        add(p->fac_steps_h), add(p->fac_pairs_h), add(p->fac_blks_h), add(flags), add(kcomp), add(klocal), add(p->comp_kf_ptr_h);
        add(p->comp_kf_h), add(p->comp_off_h), add(loff), add(p->comp_np_h), add(hdr), add(tlist);
        VX_HIP(c, p->stage.ensure(tot, true));
        VX_HIP(c, p->stage_dev.ensure(tot));
        unsigned char* st = static_cast<unsigned char*>(p->stage.p);
        unsigned char* sd = static_cast<unsigned char*>(p->stage_dev.p);
        size_t off = 0;
        hipError_t e = hipSuccess;
        MultiCopy mc;
        bool ok = true;
        auto put = [&](DevBuf& d, const auto& v) {
            const size_t n = v.size() * sizeof(v[0]);
            if (e == hipSuccess) e = d.ensure(std::max<size_t>(1, n));
            if (e == hipSuccess && n) {
                std::memcpy(st + off, v.data(), n);
                ok = ok && mc.add(d.p, sd + off, n);
            }
            off += pad(std::max<size_t>(1, n));
        };
        put(p->fac_steps, p->fac_steps_h);
        put(p->fac_pairs, p->fac_pairs_h);
        put(p->fac_blks, p->fac_blks_h);
        put(p->kf_flags, flags);
        put(p->kf_comp, kcomp);
        put(p->kf_local, klocal);
        put(p->comp_kf_ptr, p->comp_kf_ptr_h);
        put(p->comp_kf, p->comp_kf_h);
        put(p->comp_off, p->comp_off_h);
        put(p->comp_loff, loff);
        put(p->comp_np, p->comp_np_h);
        put(p->comp_hdr, hdr);
        put(p->tl, tlist);
        VX_HIP(c, e);
        if (!ok) return set_error(c, VX_ERR_STATE, "sba plan: table staging");
        VX_HIP(c, hipMemcpyAsync(sd, st, off, hipMemcpyHostToDevice, c->stream));
        VX_HIP(c, mc.launch(c->stream));
    }
    mark("sba uploads");
    VX_HIP(c, p->pose.ensure((size_t)nk * 2 * 8 * sizeof(double)));
    VX_HIP(c, p->lm.ensure((size_t)std::max(n_opt, 1) * 2 * 4 * sizeof(double)));
    VX_HIP(c, p->wy.ensure((size_t)std::max(p->n_oo, 1) * kWy * sizeof(double)));
    VX_HIP(c, p->lm_sys.ensure((size_t)std::max(n_opt, 1) * kLmSys * sizeof(double)));
    // reduction buffer = [component matrices in the factor layout ((np + 16) x np each) | rhs |
    // D | kf_cost]; unsharded, k_sba_solve factors it in place, sharded it factors the all-reduced copy
    const size_t red_n = (size_t)p->l_total + (size_t)nk * 14;
    VX_HIP(c, p->red.ensure(red_n * sizeof(double)));
    VX_HIP(c, hipMemsetAsync(p->red.p, 0, red_n * sizeof(double), c->stream));
    if (p->shard_count > 1) {
        VX_HIP(c, p->red_sum.ensure(red_n * sizeof(double)));
        VX_HIP(c, hipMemsetAsync(p->red_sum.p, 0, red_n * sizeof(double), c->stream));
    }
    // k_sba_blocks: D workgroups per diagonal block, ~512 of its keyframe's observations each, where
    // the diagonal blocks are the launch's long pole — few off-diagonal blocks (measured, r04z: C3
    // 40.9 -> 34.2 us per launch, C5 97.6 -> 92.1; the connected C5's 2318 off-diagonal blocks
    // 96.7 -> 101.3, so it keeps D = 1).  $VX_SBA_DIAG_SPLIT overrides; 1 = the round-3 form.
    p->diag_split = p->n_blocks <= 8 * nk ? std::max(1, std::min(8, (int)((p->n_obs / std::max(nk, 1) + 511) / 512))) : 1;
    if (const char* e = std::getenv("VX_SBA_DIAG_SPLIT")) p->diag_split = std::max(1, std::min(8, std::atoi(e)));
    VX_HIP(c, p->bpart.ensure((size_t)nk * p->diag_split * kBlkTerms * sizeof(double)));
    VX_HIP(c, p->Linv.ensure((size_t)std::max<long long>(p->l_total, 1) * sizeof(double)));
    VX_HIP(c, p->dx.ensure((size_t)nk * 6 * sizeof(double)));
    VX_HIP(c, hipMemsetAsync(p->dx.p, 0, (size_t)nk * 6 * sizeof(double), c->stream));
    VX_HIP(c, p->state.ensure(sizeof(SBAState)));
    VX_HIP(c, hipMemsetAsync(p->state.p, 0, sizeof(SBAState), c->stream));
    mark("sba solve buffers");
    return VX_OK;
}

namespace {
// k_sba_solve's LDS for ps panel slots: panel | L_kk^-1 | POTRF columns (2 tiles) | y | slot map
size_t solve_lds_bytes(int np, int ps) {
    return ((size_t)(ps + 3) * kPanelStride + (size_t)np) * sizeof(double) + (size_t)(np / 16 + 1) * sizeof(int);
}
// panel slots: the largest column panel of any component, as many as fit gfx950's 160 KB
int solve_panel_slots(int np, int max_panel) {
    int ps = std::max(max_panel, 1);
    // $VX_SBA_PANEL_SLOTS caps the slots (tests: the global-operand steps on small windows)
    if (const char* e = std::getenv("VX_SBA_PANEL_SLOTS")) ps = std::max(1, std::min(ps, std::atoi(e)));
    while (ps > 1 && solve_lds_bytes(np, ps) > 160 * 1024) --ps;
    return ps;
}

// Measured per LM iteration (r04e, profiles/r04/sba_bench_*_r04e.jsonl): one component of 75 tile
// columns (connected C5) 2004 -> 1004 us multi; 19 columns (C3) 153 vs 165 us and eight components of
// 10 (C5) 86 vs 99 us favour the single workgroup, whose steps need no launch.  $VX_SBA_FACTOR=single
// | multi forces one (read per run: a plan captured into a graph keeps the form it was captured with).
// LDS of k_sba_fac_step's look-ahead: 4 tiles (diagonal, L^-1, POTRF columns) + ps panel images +
// the tile row -> slot map and the updated flags
size_t lookahead_lds_bytes(int max_nt, int ps) {
    return (size_t)(4 + ps) * kPanelStride * sizeof(double) + (size_t)(max_nt + 1 + ps) * sizeof(int);
}

bool factor_blocked(const vx_sba_plan* p);
// Round 5: with one look-ahead tile per workgroup the blocked form is ahead at every size measured —
// C3 (19 tile columns) 144 -> 94 us per LM iteration, C5 (eight components of 10) 83 -> 55
// (`profiles/r05/sba_factor_block_small_r05az.txt`) — so it is the default wherever its LDS holds a
// block; otherwise one column per launch above 32 tile columns, the single workgroup below.
bool factor_multi(const vx_sba_plan* p) {
    const char* e = std::getenv("VX_SBA_FACTOR");
    if (e && std::strcmp(e, "single") == 0) return false;
    if (e && (std::strcmp(e, "multi") == 0 || std::strcmp(e, "block") == 0)) return true;
    return factor_blocked(p) || p->max_nt > 32;
}
// the multi-workgroup factor in blocks of up to kFbW columns (k_sba_fac_blk, the default where every
// column fits its LDS: connected C5 786 against 937 us per LM iteration) or one column
// per launch ($VX_SBA_FACTOR=multi)
// k_sba_fac_blk's LDS: the block's tiles, the two L_cc^-1, the entries and the slot table
size_t blk_lds_bytes(int max_nt) {
    return ((size_t)kFbCap + 2) * kPanelStride * sizeof(double) +
           ((size_t)kFbCap + kFbW * ((size_t)max_nt + 1) + kFbW + 1) * sizeof(int);
}
constexpr int kLdsMax = 160 * 1024 - 256;  // (dynamic LDS: the kernel's static variables take the rest)
bool factor_blocked(const vx_sba_plan* p) {
    const char* e = std::getenv("VX_SBA_FACTOR");
    if (e && std::strcmp(e, "multi") == 0) return false;
    return p->blk_ok && blk_lds_bytes(p->max_nt) <= (size_t)kLdsMax;  // (larger components: one column per launch)
}
// workgroups per component and step: workgroup 0 takes the look-ahead column, the others about 8
// trailing tiles each (two per wave); $VX_SBA_FACTOR_GROUPS overrides
int factor_groups(int max_trail_rest) {
    int g = 1 + (max_trail_rest + 7) / 8;
    if (const char* e = std::getenv("VX_SBA_FACTOR_GROUPS")) g = std::atoi(e);
    return std::max(1, std::min(g, 128));
}

// The launch configuration of a plan's run (the factor form, LDS sizes), fixed per run.
struct SbaRunCfg {
    SBAArgs a;
    size_t lds = 0, bs_lds = 0, la_lds = 0, red_n = 0, blk_lds = 0;
    int upd_blocks = 1, G = 1, la_ps = 0, Gb = 1, bs_depth = 3, Gu = 1;
    bool multi = false, pair = false, blk = false;
};

int sba_prepare(vx_ctx* c, vx_sba_plan* p, SbaRunCfg& r) {
    r.a = make_args(p);
    const SBAArgs& a = r.a;
    r.lds = solve_lds_bytes(p->max_np, a.panel_slots);
    if (r.lds > 64 * 1024)
        VX_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sba_solve),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)r.lds));
    r.upd_blocks = (std::max(p->n_opt, p->nk) + kUpdThreads - 1) / kUpdThreads;
    // the factorisation: one launch per tile step over G workgroups per component (components of
    // more than 32 tile columns), or the whole factor in one workgroup per component (the round-3 form)
    r.bs_lds = (size_t)p->max_np * sizeof(double) + ((size_t)a.bs_nt + 1 + p->max_back) * sizeof(int);
    r.bs_depth = std::getenv("VX_SBA_BS_DEPTH") && std::atoi(std::getenv("VX_SBA_BS_DEPTH")) == 6 ? 6 : kBsDepth;
    if (r.bs_lds > 64 * 1024) {
        VX_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sba_backsub<kBsDepth>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)r.bs_lds));
        VX_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sba_backsub<6>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)r.bs_lds));
    }
    r.multi = factor_multi(p);
    r.G = factor_groups(p->max_trail_rest);
    // one tile column per launch (default) or two ($VX_SBA_FACTOR_COLS=2: half the launches, but
    // workgroup 0's chain per launch doubles — measured slower on the connected C5, 1137 against 1030
    // us per LM iteration, profiles/r04/sba_cols*_r04j.jsonl)
    r.pair = std::getenv("VX_SBA_FACTOR_COLS") && std::atoi(std::getenv("VX_SBA_FACTOR_COLS")) == 2;
    // workgroup 0's look-ahead column in LDS when its panel fits ($VX_SBA_LOOKAHEAD_LDS=0: global)
    r.la_ps = std::max(p->max_panel, 1);
    r.la_lds = lookahead_lds_bytes(p->max_nt, r.la_ps);
    if (r.la_lds > 160 * 1024 || (std::getenv("VX_SBA_LOOKAHEAD_LDS") && std::atoi(std::getenv("VX_SBA_LOOKAHEAD_LDS")) == 0)) {
        r.la_ps = 0;
        r.la_lds = 4 * kPanelStride * sizeof(double);
    }
    if (r.multi && r.la_lds > 64 * 1024)
        VX_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sba_fac_step),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)r.la_lds));
    r.blk = r.multi && !r.pair && factor_blocked(p);
    if (r.blk) {
        r.blk_lds = blk_lds_bytes(p->max_nt);
        static std::atomic<uint64_t> blk_attr{0};
        // (the attribute at the most any plan launches with: it is set once per device)
        VX_HIP(c, lds_attr_once(c->device, reinterpret_cast<const void*>(&k_sba_fac_blk), kLdsMax, blk_attr));
        // workgroup 0 factors the block, the others take ~32 trailing tiles each (4 per wave in flight)
        // the look-ahead launch: one tile per workgroup (its wave 0), the launch spread over as many
        // CUs as block t has look-ahead tiles — each tile is a chain of up to 16 dependent MFMAs, so
        // tiles sharing a wave or a CU wait on each other (connected C5: 5.78 -> 5.17 ms per
        // optimisation against 16 tiles per workgroup; 64-thread workgroups measured the same,
        // DESIGN.md §22).  $VX_SBA_UPD_TILES / $VX_SBA_BLK_TILES: tiles per look-ahead / helper
        // workgroup, for sweeps.
        const int bt = std::getenv("VX_SBA_BLK_TILES") ? std::max(1, std::atoi(std::getenv("VX_SBA_BLK_TILES"))) : 32;
        const int ut = std::getenv("VX_SBA_UPD_TILES") ? std::max(1, std::atoi(std::getenv("VX_SBA_UPD_TILES"))) : 1;
        r.Gb = 1 + (p->max_blk_trail + bt - 1) / bt;
        if (const char* e = std::getenv("VX_SBA_FACTOR_GROUPS")) r.Gb = std::atoi(e);
        r.Gb = std::max(1, std::min(r.Gb, 128));
        r.Gu = std::max(1, std::min(1024, (p->max_blk_la + ut - 1) / ut));
    }
    r.red_n = (size_t)p->l_total + (size_t)p->nk * 14;
    return VX_OK;
}

// iteration it, part 1: the landmark stage and the reduced system's blocks (this shard's share)
int sba_assemble(vx_ctx* c, vx_sba_plan* p, const SbaRunCfg& r, int it) {
    const SBAArgs& a = r.a;
    if (p->n_lm_blocks > 0)
        VX_HIP(c, launch(c, kStSbaLandmark, k_sba_lm, dim3(p->n_lm_blocks), dim3(kLmThreads), 0, c->stream, a, it));
    VX_HIP(c, launch(c, kStSbaBlocks, k_sba_blocks, dim3(p->n_blocks + p->nk * (p->diag_split - 1)),
                     dim3(kBlkThreads), 0, c->stream, a, it));
    if (p->diag_split > 1)
        VX_HIP(c, launch(c, kStSbaBlocks, k_sba_blocks_diag, dim3(p->nk), dim3(64), 0, c->stream, a, it));
    return VX_OK;
}

// iteration it, part 2 (on the summed system, sharded: identical on every rank): the LM decision,
// the factorisation, back-substitution and the update
int sba_solve_step(vx_ctx* c, vx_sba_plan* p, const SbaRunCfg& r, int it) {
    const SBAArgs& a = r.a;
    const int G = r.G;
    if (r.blk) {
        for (int t = 0; t < p->max_blks; ++t) {
            FacBlk sd{};  // (one component: the launch's bounds as arguments)
            if (p->n_comp == 1) {
                const int* d = p->fac_blks_h.data() + 16 * (size_t)t;
                sd.loff = (long long)(((unsigned long long)(unsigned)d[1] << 32) | (unsigned)d[0]);
                sd.K0 = d[2], sd.W = d[3], sd.bt_beg = d[4], sd.bt_end = d[5], sd.pb_beg = d[6], sd.pb_end = d[7];
                sd.K0p = d[8], sd.Wp = d[9], sd.tr_beg = d[10], sd.tr_end = d[11], sd.nt = d[12];
                sd.la_beg = d[13], sd.la_end = d[14];
            }
            if (t > 0)
                VX_HIP(c, launch(c, kStSbaSolve, k_sba_fac_upd, dim3(std::max(p->n_comp, 1) * r.Gu), dim3(kFbThreads), 0,
                                 c->stream, a, it, t, r.Gu, sd));
            VX_HIP(c, launch(c, kStSbaSolve, k_sba_fac_blk, dim3(std::max(p->n_comp, 1) * r.Gb), dim3(kFbThreads),
                             (uint32_t)r.blk_lds, c->stream, a, it, t, r.Gb, kFbCap, sd));
        }
    } else if (r.multi) {
        VX_HIP(c, launch(c, kStSbaSolve, k_sba_fac_begin, dim3(std::max(p->n_comp, 1)), dim3(kSolveThreads), 0,
                         c->stream, a, it, r.pair ? 1 : 0));
        for (int t = 0; r.pair && t < p->max_pairs; ++t) {
            FacPair sd{};  // (one component: the launch's bounds as arguments)
            if (p->n_comp == 1) {
                const int* d = p->fac_pairs_h.data() + 16 * (size_t)t;
                sd.loff = (long long)(((unsigned long long)(unsigned)d[1] << 32) | (unsigned)d[0]);
                sd.l1b = d[2], sd.l1e = d[3], sd.l2b = d[4], sd.l2e = d[5], sd.rb = d[6], sd.re = d[7];
                sd.p0 = d[8], sd.p1 = d[9], sd.q0 = d[10], sd.q1 = d[11], sd.nt = d[12], sd.c0 = d[13];
            }
            VX_HIP(c, launch(c, kStSbaSolve, k_sba_fac_pair, dim3(std::max(p->n_comp, 1) * G), dim3(kSolveThreads), 0,
                             c->stream, a, it, t, G, sd));
        }
        for (int k = 0; !r.pair && k + 1 < p->max_nt; ++k) {
            FacStep sd{};  // (one component: the step's bounds as launch arguments)
            if (p->n_comp == 1) {
                const int* d = p->fac_steps_h.data() + 8 * (size_t)k;
                sd.loff = (long long)(((unsigned long long)(unsigned)d[1] << 32) | (unsigned)d[0]);
                sd.la_beg = d[2];
                sd.split = d[3];
                sd.t_end = d[4];
                sd.p0 = d[5];
                sd.p1 = d[6];
                sd.nt = d[7];
            }
            VX_HIP(c, launch(c, kStSbaSolve, k_sba_fac_step, dim3(std::max(p->n_comp, 1) * G), dim3(kSolveThreads),
                             (uint32_t)r.la_lds, c->stream, a, it, k, G, r.la_ps, sd));
        }
    } else {
        VX_HIP(c, launch(c, kStSbaSolve, k_sba_solve, dim3(std::max(p->n_comp, 1)), dim3(kSolveThreads),
                         (uint32_t)r.lds, c->stream, a, it));
    }
    VX_HIP(c, launch(c, kStSbaSolve, r.bs_depth == 6 ? k_sba_backsub<6> : k_sba_backsub<kBsDepth>, dim3(std::max(p->n_comp, 1)), dim3(kSolveThreads),
                     (uint32_t)r.bs_lds, c->stream, a, it));
    VX_HIP(c, launch(c, kStSbaUpdate, k_sba_update, dim3(std::max(r.upd_blocks, 1)), dim3(kUpdThreads), 0,
                     c->stream, a, it));
    return VX_OK;
}

int sba_run(vx_ctx* c, vx_sba_plan* p) {
    if (p->status != 0) {
        p->ran = true;
        return VX_OK;
    }
    const bool sharded = p->shard_count > 1;
    if (sharded) {
#ifndef VX_NO_RCCL
        if (!c->comm || c->nranks != p->shard_count || c->rank != p->shard_rank)
            return set_error(c, VX_ERR_STATE, "sharded plan needs vx_comm_init(%d ranks)", p->shard_count);
#else
        return set_error(c, VX_ERR_COMM, "built without RCCL");
#endif
    }
    SbaRunCfg r;
    int rc;
    if ((rc = sba_prepare(c, p, r))) return rc;
    for (int it = 0; it < p->opt.max_iterations; ++it) {
        if ((rc = sba_assemble(c, p, r, it))) return rc;
#ifndef VX_NO_RCCL
        if (sharded) {
            ProfScope ps(c, kStSbaAllreduce);
            ncclResult_t nr = ncclAllReduce(p->red.p, p->red_sum.p, r.red_n, ncclDouble, ncclSum, c->comm, c->stream);
            if (nr != ncclSuccess) return set_error(c, VX_ERR_COMM, "ncclAllReduce: %s", ncclGetErrorString(nr));
        }
#endif
        if ((rc = sba_solve_step(c, p, r, it))) return rc;
    }
    p->ran = true;
    return VX_OK;
}

// the shards' reduced systems summed in rank order into every shard's all-reduce target (the
// emulated ncclAllReduce of vx_sba_shard_emulate_run)
constexpr int kMaxSbaEmuShards = 8;
struct RedPtrs {
    const double* src[kMaxSbaEmuShards];
    double* dst[kMaxSbaEmuShards];
};
__global__ void k_sba_sum_shards(RedPtrs p, int n, long long len) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len) return;
    double s = p.src[0][i];
    for (int r = 1; r < n; ++r) s += p.src[r][i];
    for (int r = 0; r < n; ++r) p.dst[r][i] = s;
}

// the best state of a finished run (LM selection of the last iteration) into the resident rows
__global__ void k_sba_apply_dmap(const SBAState* st, int nk, int n_opt, const double* pose0, const double* pose,
                                 const double* lm0, const double* lm, const int* kf_map, const int* lm_map,
                                 double* map_pose, double* map_pos) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const LMVars& v = st->lm[st->iterations & 1];
    if (i < nk) {
        const double* src = (v.sel < 0 ? pose0 : pose + (size_t)v.sel * nk * 8) + 8 * (size_t)i;
        for (int j = 0; j < 7; ++j) map_pose[7 * (size_t)kf_map[i] + j] = src[j];
    }
    if (i < n_opt) {
        const double* src = (v.sel < 0 ? lm0 : lm + (size_t)v.sel * n_opt * 4) + 4 * (size_t)i;
        for (int j = 0; j < 3; ++j) map_pos[3 * (size_t)lm_map[i] + j] = src[j];
    }
}

}  // namespace

int build_sba_plan_dmap(vx_ctx* c, vx_dmap* m, uint64_t ref, int has_ref, vx_sba_plan* p);  // ba_lean.hip
}  // namespace vx

using namespace vx;

VX_KT_EXPORT(vx_ktrace_read_sba);

extern "C" {

void vx_sba_default_options(vx_sba_options* o) {
    if (!o) return;
    o->window_size = 5;
    o->max_iterations = 10;
    o->min_point_observations = 2;
    o->fixed_keyframes = 2;
    o->huber_delta = 5.0;
    o->max_reproj_error = 5.0;
    o->lambda_init = 1e-4;
    o->rel_tol = 1e-6;
}

int vx_sba_plan_create(vx_ctx* c, const vx_map_view* m, uint64_t ref, int has_ref, const vx_sba_options* opt,
                       int shard_rank, int shard_count, vx_sba_plan** out) {
    if (!c || !out || !opt) return VX_ERR_INVALID;
    *out = nullptr;
    if (opt->max_iterations < 0 || opt->max_iterations > kSbaMaxIter)
        return set_error(c, VX_ERR_INVALID, "max_iterations must be in [0, %d]", kSbaMaxIter);
    if (opt->fixed_keyframes < 0 || !(opt->lambda_init >= 0.0))
        return set_error(c, VX_ERR_INVALID, "fixed_keyframes >= 0 and lambda_init >= 0 required");
    if (shard_count < 1 || shard_rank < 0 || shard_rank >= shard_count)
        return set_error(c, VX_ERR_INVALID, "bad shard %d/%d", shard_rank, shard_count);
    auto* p = new vx_sba_plan();
    p->c = c;
    p->opt = *opt;
    p->shard_rank = shard_rank;
    p->shard_count = shard_count;
    const int rc = build_sba_plan(c, m, ref, has_ref, p);
    if (rc) {
        delete p;
        return rc;
    }
    *out = p;
    return VX_OK;
}

int vx_sba_plan_create_dmap(vx_ctx* c, vx_dmap* m, uint64_t ref, int has_ref, const vx_sba_options* opt,
                            vx_sba_plan** out) {
    if (!c || !out || !opt || !m || m->c != c)
        return c ? set_error(c, VX_ERR_INVALID, "vx_sba_plan_create_dmap: bad arguments") : VX_ERR_INVALID;
    *out = nullptr;
    if (opt->max_iterations < 0 || opt->max_iterations > kSbaMaxIter)
        return set_error(c, VX_ERR_INVALID, "max_iterations must be in [0, %d]", kSbaMaxIter);
    if (opt->fixed_keyframes < 0 || !(opt->lambda_init >= 0.0))
        return set_error(c, VX_ERR_INVALID, "fixed_keyframes >= 0 and lambda_init >= 0 required");
    auto* p = new vx_sba_plan();
    p->c = c;
    p->opt = *opt;
    const int rc = build_sba_plan_dmap(c, m, ref, has_ref, p);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);
        delete p;
        return rc;
    }
    *out = p;
    return VX_OK;
}

int vx_sba_shard_emulate_run(vx_ctx* c, vx_sba_plan* const* plans, int n) {
    if (!c || !plans || n < 1 || n > kMaxSbaEmuShards)
        return c ? set_error(c, VX_ERR_INVALID, "vx_sba_shard_emulate_run: bad arguments") : VX_ERR_INVALID;
    vx_sba_plan* p0 = plans[0];
    for (int r = 0; r < n; ++r) {
        const vx_sba_plan* p = plans[r];
        if (!p || p->c != c || p->shard_count != n || p->shard_rank != r)
            return set_error(c, VX_ERR_INVALID, "shard %d: plan of another context or shard layout", r);
        if (p->status != p0->status || p->nk != p0->nk || p->l_total != p0->l_total || p->n_blocks != p0->n_blocks ||
            p->opt.max_iterations != p0->opt.max_iterations)
            return set_error(c, VX_ERR_INVALID, "shard %d: plan built from another window", r);
    }
    if (p0->status != 0) {
        for (int r = 0; r < n; ++r) plans[r]->ran = true;
        return VX_OK;
    }
    std::vector<SbaRunCfg> cfg(n);
    RedPtrs rp{};
    int rc;
    for (int r = 0; r < n; ++r) {
        if ((rc = sba_prepare(c, plans[r], cfg[r]))) return rc;
        rp.src[r] = plans[r]->red.as<double>();
        rp.dst[r] = plans[r]->red_sum.as<double>();
    }
    const long long len = (long long)cfg[0].red_n;
    for (int it = 0; it < p0->opt.max_iterations; ++it) {
        for (int r = 0; r < n; ++r)
            if ((rc = sba_assemble(c, plans[r], cfg[r], it))) return rc;
        hipLaunchKernelGGL(k_sba_sum_shards, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, c->stream, rp, n, len);
        VX_LAUNCH_CHECK(c, "k_sba_sum_shards");
        for (int r = 0; r < n; ++r)
            if ((rc = sba_solve_step(c, plans[r], cfg[r], it))) return rc;
    }
    for (int r = 0; r < n; ++r) plans[r]->ran = true;
    return VX_OK;
}

int vx_sba_plan_rebuild_dmap(vx_ctx* c, vx_dmap* m, uint64_t ref, int has_ref, vx_sba_plan* p) {
    if (!c || !p || !m || p->c != c || m->c != c)
        return c ? set_error(c, VX_ERR_INVALID, "vx_sba_plan_rebuild_dmap: bad arguments") : VX_ERR_INVALID;
    if (!p->from_dmap) return set_error(c, VX_ERR_STATE, "plan was not built from a vx_dmap");
    // the previous build's staged uploads and any run of the plan are complete before its buffers
    // and staging are rewritten (a no-op after the fetch that normally precedes a rebuild)
    VX_HIP(c, hipStreamSynchronize(c->stream));
    p->graph.reset();
    p->ran = false;
    const int rc = build_sba_plan_dmap(c, m, ref, has_ref, p);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);
        p->status = 1;
        return rc;
    }
    return VX_OK;
}

int vx_sba_plan_apply_dmap(vx_ctx* c, vx_sba_plan* p, vx_dmap* m) {
    if (!c || !p || !m || p->c != c || m->c != c)
        return c ? set_error(c, VX_ERR_INVALID, "vx_sba_plan_apply_dmap: bad arguments") : VX_ERR_INVALID;
    if (!p->from_dmap) return set_error(c, VX_ERR_STATE, "plan was not built from a vx_dmap");
    if (!p->ran) return set_error(c, VX_ERR_STATE, "plan not run");
    if (p->status != 0 || p->opt.max_iterations == 0) return VX_OK;
    const int n = std::max(p->nk, p->n_opt);
    hipLaunchKernelGGL(k_sba_apply_dmap, dim3((n + 255) / 256), dim3(256), 0, c->stream,
                       (const SBAState*)p->state.as<SBAState>(), p->nk, p->n_opt, (const double*)p->pose0.as<double>(),
                       (const double*)p->pose.as<double>(), (const double*)p->lm0.as<double>(),
                       (const double*)p->lm.as<double>(), (const int*)p->kf_map_dev.as<int>(),
                       (const int*)p->lm_map_dev.as<int>(), m->kf_pose.as<double>(), m->lm_pos.as<double>());
    VX_LAUNCH_CHECK(c, "k_sba_apply_dmap");
    return VX_OK;
}

int vx_sba_plan_run_async(vx_ctx* c, vx_sba_plan* p) {
    if (!c || !p || p->c != c) return VX_ERR_INVALID;
    if (p->shard_count > 1 || p->status != 0) return sba_run(c, p);  // (RCCL calls stay outside graphs)
    p->ran = true;
    return graph_run_owned(c, p->graph, [](vx_ctx* cc, void* v) { return sba_run(cc, static_cast<vx_sba_plan*>(v)); }, p);
}

int vx_sba_plan_fetch(vx_ctx* c, vx_sba_plan* p, vx_map_view* m, vx_sba_stats* st) {
    if (!c || !p || p->c != c) return VX_ERR_INVALID;
    if (!p->ran) return set_error(c, VX_ERR_STATE, "plan not run");
    if (m && p->from_dmap) return set_error(c, VX_ERR_STATE, "dmap plan: scatter with vx_sba_plan_apply_dmap");
    vx_sba_stats s{};
    s.status = p->status;
    s.n_window_kf = p->n_window_kf;
    s.n_landmarks = p->n_landmarks_global;
    if (p->status == 0 && p->opt.max_iterations > 0) {
        SBAState hs;
        VX_HIP(c, hipMemcpyAsync(&hs, p->state.p, sizeof hs, hipMemcpyDeviceToHost, c->stream));
        VX_HIP(c, hipStreamSynchronize(c->stream));
        const LMVars v = hs.lm[hs.iterations & 1];
        std::vector<double> pose((size_t)p->nk * 8), lm((size_t)std::max(p->n_opt, 1) * 4);
        const double* ps = v.sel < 0 ? p->pose0.as<double>() : p->pose.as<double>() + (size_t)v.sel * p->nk * 8;
        const double* ls = v.sel < 0 ? p->lm0.as<double>() : p->lm.as<double>() + (size_t)v.sel * p->n_opt * 4;
        VX_HIP(c, hipMemcpyAsync(pose.data(), ps, pose.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (p->n_opt > 0)
            VX_HIP(c, hipMemcpyAsync(lm.data(), ls, (size_t)p->n_opt * 4 * sizeof(double), hipMemcpyDeviceToHost,
                                     c->stream));
        VX_HIP(c, hipStreamSynchronize(c->stream));
        if (c->prof) prof_collect(c);
        s.iterations = hs.iterations;
        s.accepted = v.accepted;
        s.lambda = v.lambda;
        s.initial_cost = hs.initial_cost;
        s.final_cost = v.best_cost;
        for (int i = 0; i < 16; ++i) {
            s.cost[i] = hs.cost[i];
            s.obs[i] = hs.obs[i];
            s.step[i] = hs.step[i];
        }
        if (m) {
            for (int r = 0; r < p->nk; ++r)
                for (int j = 0; j < 7; ++j) m->kf_pose[7 * p->kf_map_idx[r] + j] = pose[8 * r + j];
            for (int sl = 0; sl < p->n_opt; ++sl)
                for (int j = 0; j < 3; ++j) m->lm_pos[3 * p->lm_map_idx[sl] + j] = lm[4 * sl + j];
        }
    }
    if (st) *st = s;
    return VX_OK;
}

void vx_sba_plan_destroy(vx_sba_plan* p) {
    delete p;
}

int vx_sba_plan_info(const vx_sba_plan* p, int64_t* out8) {
    if (!p || !out8) return VX_ERR_INVALID;
    const int64_t v[8] = {p->nk, p->n_opt, p->n_obs, p->n_pairs, p->n_blocks, 6 * (int64_t)p->nk,
                          p->n_lfactor_tiles, p->n_comp};
    for (int i = 0; i < 8; ++i) out8[i] = v[i];
    return VX_OK;
}

int vx_sba_plan_factor_work(const vx_sba_plan* p, int64_t* out4) {
    if (!p || !out4) return VX_ERR_INVALID;
    int64_t diag = 0;
    for (int np : p->comp_np_h) diag += np / 16;
    // (algorithmic: the rhs row's tiles — one per column, and their updates — are left out)
    const int64_t v[4] = {p->n_lfactor_tiles - diag, p->n_trail_updates - p->n_trail_rhs, diag,
                          p->n_lfactor_tiles - diag - diag};
    for (int i = 0; i < 4; ++i) out4[i] = v[i];
    return VX_OK;
}

int vx_sba_plan_system(vx_ctx* c, vx_sba_plan* p, double* S, double* rhs, int n) {
    if (!c || !p || p->c != c || !S || !rhs) return VX_ERR_INVALID;
    if (p->status != 0) return set_error(c, VX_ERR_STATE, "empty plan");
    if (n != 6 * p->nk) return set_error(c, VX_ERR_INVALID, "n must be %d", 6 * p->nk);
    if (!p->ran) return set_error(c, VX_ERR_STATE, "plan not run");
    const size_t red_n = (size_t)p->l_total + (size_t)p->nk * 14;
    std::vector<double> h(red_n);
    const void* src = p->shard_count > 1 ? p->red_sum.p : p->red.p;
    VX_HIP(c, hipMemcpyAsync(h.data(), src, red_n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    SBAState hs;
    VX_HIP(c, hipMemcpyAsync(&hs, p->state.p, sizeof hs, hipMemcpyDeviceToHost, c->stream));
    VX_HIP(c, hipStreamSynchronize(c->stream));
    const int n6 = 6 * p->nk;
    // the damping of the last assembly: lambda of lm[(iterations - 1) & 1] (lambda0 at iteration 0)
    const double lambda = hs.iterations <= 1 ? p->opt.lambda_init : hs.lm[(hs.iterations - 1) & 1].lambda;
    const double* rh = h.data() + p->l_total;
    std::memset(S, 0, sizeof(double) * (size_t)n * n);
    std::vector<int> comp_of(p->nk, -1), local(p->nk, 0);
    for (int cc = 0; cc < p->n_comp; ++cc)
        for (int q = p->comp_kf_ptr_h[cc]; q < p->comp_kf_ptr_h[cc + 1]; ++q) {
            comp_of[p->comp_kf_h[q]] = cc;
            local[p->comp_kf_h[q]] = q - p->comp_kf_ptr_h[cc];
        }
    for (int i = 0; i < p->nk; ++i) {
        const int ci = comp_of[i];
        for (int a2 = 0; a2 < 6; ++a2) rhs[6 * i + a2] = ci < 0 ? 0.0 : rh[6 * i + a2];
        if (ci < 0) {
            for (int a2 = 0; a2 < 6; ++a2) S[(size_t)(6 * i + a2) * (n + 1)] = 1.0;
            continue;
        }
        for (int j = 0; j <= i; ++j) {
            if (comp_of[j] != ci) continue;
            const int np = p->comp_np_h[ci];
            const double* B = h.data() + p->comp_loff_h[ci] + (size_t)(6 * local[i]) * np + 6 * local[j];
            for (int r = 0; r < 6; ++r)
                for (int cc = 0; cc < 6; ++cc) {
                    double v = B[(size_t)r * np + cc];
                    if (i == j && r == cc) v += lambda * rh[n6 + 6 * i + r] + 1e-6;
                    S[(size_t)(6 * i + r) * n + 6 * j + cc] = v;
                }
        }
    }
    return VX_OK;
}

int vx_sba_plan_step(vx_ctx* c, vx_sba_plan* p, double* dx, int n, int32_t* fail) {
    if (!c || !p || p->c != c || !dx || !fail) return VX_ERR_INVALID;
    if (p->status != 0) return set_error(c, VX_ERR_STATE, "empty plan");
    if (n != 6 * p->nk) return set_error(c, VX_ERR_INVALID, "n must be %d", 6 * p->nk);
    if (!p->ran) return set_error(c, VX_ERR_STATE, "plan not run");
    SBAState hs;
    VX_HIP(c, hipMemcpyAsync(dx, p->dx.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    VX_HIP(c, hipMemcpyAsync(&hs, p->state.p, sizeof hs, hipMemcpyDeviceToHost, c->stream));
    VX_HIP(c, hipStreamSynchronize(c->stream));
    // (fail[it] is rewritten by every iteration that runs: entries past the run's last are not its own)
    int any = 0;
    for (int it = 0; it < hs.iterations && it < kSbaMaxIter; ++it) any |= hs.fail[it] != 0;
    *fail = any;
    return VX_OK;
}

int vx_sba_optimize_map(vx_ctx* c, vx_map_view* m, uint64_t ref, int has_ref, const vx_sba_options* opt,
                        vx_sba_stats* st) {
    vx_sba_plan* p = nullptr;
    int rc = vx_sba_plan_create(c, m, ref, has_ref, opt, 0, 1, &p);
    if (rc) return rc;
    rc = vx_sba_plan_run_async(c, p);
    if (!rc) rc = vx_sba_plan_fetch(c, p, m, st);
    (void)hipStreamSynchronize(c->stream);
    vx_sba_plan_destroy(p);
    return rc;
}

}  // extern "C"
