// ba_fused_kernel.hpp — device code of ba.hip, included by it alone after ba_kernels.hpp: the fused
// path's argument record FusedArgs, its LDS layout and k_ba_iter (one launch per iteration).
#pragma once
#include "ba_kernels.hpp"

namespace vx {
namespace {

using namespace vx::ba;

// ------------------------------------------------------------------ fused path: one launch per iteration
// k_ba_iter(it) = combine + pose solve of iteration it, landmark stage of it, pose stage of it + 1.
// Workgroups own whole landmarks in keyframe-locality order (plan: build_fused), so each needs the
// poses of only the few keyframes its observations touch (kent: at most kFK entries).  After its
// landmark stage a workgroup holds the iteration's poses (LDS) and its landmarks' new positions
// (LDS), which is everything the next iteration's pose stage needs for the pose observations of
// those landmarks (local_ba.cpp:131-159 at it + 1): it forms their 29 terms per keyframe (one wave
// per keyframe entry, halving butterfly) into that keyframe's partial slot.  The next launch sums a
// keyframe's slots in slot order — the same sum in every workgroup that needs the pose, so the
// redundant solves agree bitwise — and every keyframe's pose is published by exactly one owner.
// Pose observations of fixed landmarks (not optimised: positions constant) go to the owner of their
// keyframe.  The prologue launch (kPro) forms iteration 0's pose stage from the initial state.
constexpr int kFK = kBaFusedK;
// Threads per fused workgroup (= its landmark-stage observation / landmark capacity): 512, or 1024
// for windows whose 512-thread packing needs more workgroups than the device has CUs (fewer,
// larger workgroups: shorter per-keyframe slot lists; measured).
constexpr int kFTSmall = kBaFTSmall, kFTLarge = kBaFTLarge, kFTNarrow = kBaFTNarrow;

// Fused layout (ba.hip build_fused).  Per workgroup b: landmarks and landmark-stage observations at
// the fixed bases b * kFT (padded), so their loads do not wait for the workgroup table; keyframe
// entries at b * kFK; pose-stage observations in wave-major order — wave w takes entries w, w + kFW,
// ..., each entry's observations start on a 64-aligned index (lane l of round r reads wstart + 64 r
// + l), with fixed landmarks' positions stored in the observation record.
struct FusedArgs {
    const int4* blk;        // 1 + kFW / 2 per workgroup: {landmarks, landmark-stage observations,
                            // keyframe entries, 0}, then {wstart, rounds} per wave
    const int* lm_slot;     // [b * kFT + t] landmark slot (padding: slot 0)
    const int2* lm_run;     // [b * kFT + t] its landmark-stage observations [r0, r1) (workgroup-local)
    const double2* lobs_uv; // [b * kFT + t]
    const int4* lobs_rec;   // [b * kFT + t] {keyframe entry, workgroup-local landmark, slot, 0}
    const int4* kent;       // 2 per entry, kFK entries per workgroup: {row | owner << 30, or -1; slots of
                            // the row; pose observations [start, end)}, {partial slot or -1, 0, 0, 0}
    const double2* pobs_uv;
    const double4* pobs_p;  // {x, y, z, code}: code >= 0 workgroup-local landmark (position from LDS),
                            // code < 0 a fixed landmark at (x, y, z)
    double* part;           // 2 x n_kf x maxl partial blocks of 32 doubles (row-major by keyframe): the
                            // pose stage of iteration i fills buffer i & 1 (a launch reads one buffer
                            // and writes the other, so no workgroup reads what another overwrites)
    int maxl, n_part;
    const double* rowpart;  // sharded plans: per keyframe row the partial slots summed (k_row_sum) and
                            // all-reduced over the ranks; the combine and the stop rule read it instead
    double4* lpos;          // [b * kFT + t] the workgroup's landmark positions in fused order (each read
                            // and rewritten by its owning thread only; the prologue fills them)
    double2* costpart;      // 2 x n_part: each partial slot's {cost, observations} (terms 27, 28) again,
                            // compact, for the stop rule's totals (parity as part)
    int stop_b;             // the workgroup that runs the stop rule (the lightest pose stage, plan time)
    double* epose;          // [(b * kFK + j) * 16] the workgroup's copy of entry j's pose T 8 | C 4 | flags:
                            // every workgroup solving the entry computes the same pose, so each keeps
                            // its own and reads it back at a fixed address (no keyframe-row indirection)
    // Row sums by float atomics (unsharded plans; the default, $VX_BA_ATOMIC_ROWS=0 for slots):
    // launch it >= 0 adds its pose-stage partials (iteration it + 1) straight into per-row sums
    // arow[it % 3] (n_kf x kStride, float atomics executed at the memory side) instead of partial
    // slots, so the next launch combines ONE row per entry instead of re-summing the row's maxl slots
    // (sum order = arrival order: results agree to rounding, not bitwise, run to run; every workgroup
    // of a launch still reads the same row, so the redundant pose solves agree bitwise).  Launch it
    // zeroes arow[(it + 1) % 3], the buffer launch it + 1 accumulates into (last read by launch
    // it - 1).  With apro (plans of >= 2 iterations) the prologue accumulates into arow[3], which
    // launch 0 reads and the run's last launch zeroes for the next run (the plan build zeroes it
    // first); without it the prologue writes slots, which launch 0 combines.
    double* arow;
    int n_kf, apro;
    int drow;  // rows read by the entries' own threads, no combine phase ($VX_BA_DROW=0: the combine)
    int padskip;  // no loads for padding rows / lanes ($VX_BA_PADSKIP=0: every row and lane loads)
};

// the arow buffer launch `it` reads (combine), accumulates into (pose stage of it + 1) and zeroes
__device__ __forceinline__ int arow_rd(int it) { return it == 0 ? 3 : (it - 1) % 3; }
__device__ __forceinline__ int arow_wr(bool pro, int it) { return pro ? 3 : it % 3; }
__device__ __forceinline__ int arow_zero(bool pro, int it) { return pro ? 0 : (it + 1) % 3; }

// LDS layout of k_ba_iter (dynamic): kFK keyframe slots (S, then T 8 | R 9 | C 4), 9 x kFT
// observation terms, kFT counted flags, 3 x kFT landmark positions, the block-0 totals (the entry's
// loaded state stays in its solving thread's registers)
constexpr size_t fused_lds(int ft) {
    return (size_t)kFK * kLdsStride * sizeof(double) + (size_t)9 * ft * sizeof(double) +
           (size_t)ft * sizeof(int) + (size_t)3 * ft * sizeof(double) + (size_t)2 * (ft / 64) * sizeof(double);
}
static_assert(fused_lds(kFTLarge) <= 160 * 1024, "k_ba_iter LDS exceeds gfx950's 160 KB per workgroup");
// compacted pose stage (kCmp): per wave a ring of kQ accepted observations, kQRec doubles each
constexpr int kQ = 128, kQRec = 8;
constexpr size_t fused_lds_cmp(int ft) { return fused_lds(ft) + (size_t)(ft / 64) * kQ * kQRec * sizeof(double); }
static_assert(fused_lds_cmp(kFTSmall) <= 160 * 1024, "k_ba_iter (compacted) LDS exceeds 160 KB");

// The Jacobian / normal-equation half of pose_obs_accum for one accepted observation given its
// camera-frame point (xx, yy, zz), 1 / z, residual and weight (the gate already passed): the same
// FMA chains as the branch-free form (terms 0-26; cost and count are added at the gate).
__device__ __forceinline__ void pose_obs_terms(const double* C, double xx, double yy, double zz, double inv_z,
                                               double e0, double e1, double w, double* v) {
    const double fx = C[0], fy = C[1];
    const double x = xx * inv_z, y = yy * inv_z;
    const double jp0 = fx * inv_z, jp2 = -jp0 * x, jp4 = fy * inv_z, jp5 = -jp4 * y;
    const double J0[6] = {jp0, 0.0, jp2, jp2 * yy, fma(jp0, zz, -jp2 * xx), -jp0 * yy};
    const double J1[6] = {0.0, jp4, jp5, fma(jp5, yy, -jp4 * zz), -jp5 * xx, jp4 * xx};
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
            const bool u0 = r != 1 && c != 1, u1 = r != 0 && c != 0;
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
}

// trace build: phases of the it == 1 launch only (the last launch of a run has no pose stage)
#define FKT(slot)                              \
    do {                                       \
        if (!kPro && it == 1) VX_KT(slot);     \
    } while (0)

typedef int si4 __attribute__((ext_vector_type(4)));  // (an SGPR quad for the scalar loads below)

template <bool kPro, int kFT, bool kCmp = false>
__global__ __launch_bounds__(kFT) void k_ba_iter(BAArgs a, FusedArgs f, int it) {
    constexpr int kFW = kFT / 64;  // waves per workgroup
    // per-entry pose copies (f.epose) and fused-order landmark positions (f.lpos) in the 512-thread
    // kernel; the 1024-thread one (128 VGPRs) keeps the indirect reads of the published poses and
    // positions, whose longer live ranges it cannot afford
    constexpr bool kEcopy = kFT <= kFTSmall;
    // highest wave priority: in the pipeline, extraction waves share these SIMDs, and the launch's
    // dependent FP64 chains are what the frame waits for (instruction-issue arbitration prefers
    // higher-priority waves; the co-resident waves fill the gaps of the chains)
    __builtin_amdgcn_s_setprio(3);
    // row sums by atomics: the 256 / 512-thread layouts only (the host never enables them for the
    // 1024-thread one, whose 128 VGPRs leave no room: compiled out there)
    double* const arow = kFT <= kFTSmall ? f.arow : nullptr;
    if (!kPro && arow && f.apro && it == a.max_iter - 1) {  // (arow[3] for the next run's prologue)
        double* z = arow + (size_t)3 * f.n_kf * kStride;
        for (int i = blockIdx.x * kFT + threadIdx.x; i < f.n_kf * kStride; i += (int)gridDim.x * kFT) z[i] = 0.0;
    }
    // (an iteration after the stop returns before its first write, below: its loads are issued
    // first so the flag's latency overlaps theirs)
    if (!kEcopy && !kPro && it > 0 && !a.state->active[it]) return;
    // (a relaxed atomic load is issued here with the other loads — a plain one was sunk to its use —
    // and waited for only at its use below)
    const int act = kPro ? 1 : __hip_atomic_load(&a.state->active[it], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    extern __shared__ __attribute__((aligned(16))) double fl[];
    // the workgroup's keyframe entry records, staged once: the combine and the pose stage read them
    // from LDS instead of issuing a dependent global load at the start of each
    __shared__ int4 s_ke[kFK];
    __shared__ int s_kd[kFK];
    double* kslot = fl;                                  // [kFK][kLdsStride]
    double* terms = kslot + kFK * kLdsStride;            // [9][kFT]
    int* tcount = reinterpret_cast<int*>(terms + 9 * kFT);
    double* lpos = terms + 9 * kFT + kFT / 2;            // [kFT][3] (after kFT ints)
    double* red = lpos + 3 * kFT;                        // [2][kFW]
    double* qbuf = red + 2 * kFW;                        // (kCmp) [kFW][kQ][kQRec] accepted observations
    const int tid = threadIdx.x, b = blockIdx.x, wv = tid >> 6, lane = tid & 63;
    const size_t base = (size_t)b * kFT;
    const int4* KE = f.kent + (size_t)b * kFK * 2;
    const double* part_in = f.part + (size_t)(it & 1) * f.n_part * kStride;  // (unused by kPro)
    double* part_out = f.part + (size_t)((it + 1) & 1) * f.n_part * kStride;
    FKT(0);
    // ---- every load the launch needs, issued up front (at most two dependent levels); values
    // needed only after the first barrier are parked in LDS, not held in registers.  Issue order
    // matters: `s_waitcnt vmcnt` retires loads in issue order, so a value is waited for together with
    // every load issued before it.  Wave 0's chain is the block record and its entry records, then
    // the rows those name (drow), then the solve: the entry records and copies go right behind the
    // block record, ahead of the landmark loads, and none of their values is used (no wait) before
    // every independent load is in flight.
    // (the block records by scalar loads — plan data no kernel writes — so that waiting for them
    // (lgkmcnt, below) does not wait for the vector loads issued behind them; the compiler keeps
    // them on the vector path, whose in-order vmcnt made the landmark loads wait for the rows)
    const int wvu = __builtin_amdgcn_readfirstlane(wv);
    si4 Bv, WBv;
    asm volatile("s_load_dwordx4 %0, %1, 0x0" : "=s"(Bv) : "s"(f.blk + (size_t)b * (1 + kFW / 2)));
    asm volatile("s_load_dwordx4 %0, %1, 0x0" : "=s"(WBv) : "s"(f.blk + (size_t)b * (1 + kFW / 2) + 1 + (wvu >> 1)));
    // (c) the keyframe entry it solves: previous pose, intrinsics, flags (the prologue
    // gathers them by keyframe row into the workgroup's entry copy; later launches read the copy)
    int4 ke = make_int4(-1, 0, 0, 0);
    int kd = -1;
    double ev[13];
    if (tid < kFK) {
        ke = KE[2 * tid];
        kd = KE[2 * tid + 1].x;
        if (!kPro && kEcopy) {
            // (the copy is read whether or not the entry exists — unused entries are valid memory —
            // so the load does not wait for the entry table)
            const double4* E4 = reinterpret_cast<const double4*>(f.epose + ((size_t)b * kFK + tid) * 16);
            const double4 e0 = E4[0], e1 = E4[1], e2 = E4[2];
            ev[0] = e0.x, ev[1] = e0.y, ev[2] = e0.z, ev[3] = e0.w;
            ev[4] = e1.x, ev[5] = e1.y, ev[6] = e1.z, ev[7] = e1.w;
            ev[8] = e2.x, ev[9] = e2.y, ev[10] = e2.z, ev[11] = e2.w;
            ev[12] = reinterpret_cast<const double*>(E4 + 3)[0];
        }
    }
    // (a) this thread's landmark-stage observation (padding rows are valid memory)
    int4 orec = make_int4(0, 0, 0, 0);
    double2 ouv = make_double2(1e300, 1e300);
    if (!kPro) {
        orec = f.lobs_rec[base + tid];
        ouv = f.lobs_uv[base + tid];
    }
    // (c') with the rows summed by atomics the entry's own thread (wave 0) reads its row as soon as its
    // entry record is in and solves without the combine phase or the first barrier: the other waves
    // meet it at the barrier after the solve (round 5: the combine's LDS round trip and two barriers
    // off the launch's path)
    const bool drow = !kPro && f.drow && arow && (it > 0 || f.apro);
    double Sd[kNTerms];
    if (drow && tid < kFK && ke.x >= 0) {
        const double* rp = arow + ((size_t)arow_rd(it) * f.n_kf + (ke.x & 0x3fffffff)) * kStride;
#pragma unroll
        for (int t = 0; t < kNTerms; ++t) Sd[t] = rp[t];
    }
    // (c) the prologue / 1024-thread layout: the entry's state by keyframe row
    if ((kPro || !kEcopy) && tid < kFK && ke.x >= 0) {
        const int row = ke.x & 0x3fffffff;
        const double* Tin = (kPro ? a.kf_pose0 : pose_in(a, it)) + 8 * (size_t)row;
#pragma unroll
        for (int j = 0; j < 8; ++j) ev[j] = Tin[j];
#pragma unroll
        for (int j = 0; j < 4; ++j) ev[8 + j] = a.kf_intr[4 * row + j];
        ev[12] = (double)a.kf_flags[row];
    }
    // (b) the landmark it owns (its position goes to LDS for the observations of the landmark):
    // fused-order copy at a fixed address (the prologue reads the slot's initial position)
    // (iterations of the 512-thread layout: only the workgroup's B.x landmark threads load — the
    // padding rows of the other ~70 % were ~1.8 MB per launch of HBM traffic; the loads wait for B,
    // which the solving wave's row loads outlast anyway.  The prologue keeps them unconditional: its
    // first barrier waits for them.)
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(Bv), "+s"(WBv));  // (the block records, above)
    const int4 B = make_int4(Bv.x, Bv.y, Bv.z, Bv.w), WB = make_int4(WBv.x, WBv.y, WBv.z, WBv.w);
    const int wstart = (wvu & 1) ? WB.z : WB.x, wrounds = (wvu & 1) ? WB.w : WB.y;
    const bool lm_load = kPro || !kEcopy || !f.padskip || tid < B.x;
    int lslot = lm_load ? f.lm_slot[base + tid] : 0;
    int2 run = make_int2(0, 0);
    if (!kPro && lm_load) run = f.lm_run[base + tid];
    D3 PL{0.0, 0.0, 0.0};
    if (kPro || !kEcopy) {
        const double* P = kPro ? a.lm_pos0 + 4 * (size_t)lslot : lm_in(a, it, lslot);
        PL = {P[0], P[1], P[2]};
    } else if (lm_load) {
        const double* P = reinterpret_cast<const double*>(f.lpos + base + tid);
        PL = {P[0], P[1], P[2]};
    }
    // (d) this wave's first pose-stage round (round r + 1 is requested when round r is consumed)
    const bool pose_next = kPro || it + 1 < a.max_iter;
    double2 u0 = make_double2(0, 0);
    double4 p0 = make_double4(0, 0, 0, 0);
    if (pose_next && wrounds > 0) {
        u0 = f.pobs_uv[wstart + lane];
        p0 = f.pobs_p[wstart + lane];
    }
    // (the entry's state stays in the solving thread's registers: an LDS copy here would wait for
    // every load issued so far — the waits merge conservatively over the branches above)
    if (tid < kFK && (ke.x >= 0 || (!kPro && kEcopy))) {
        if (kPro && kEcopy) {
            double* E = f.epose + ((size_t)b * kFK + tid) * 16;
#pragma unroll
            for (int j = 0; j < 13; ++j) E[j] = ev[j];
        }
    }
    const int n_lm = B.x, n_ob = B.y, n_ent = B.z;
    const bool has_o = !kPro && tid < n_ob, own = tid < n_lm;
    if (!kPro && it > 0 && !act) return;  // iteration after the stop: no global write
    if (arow) {  // the buffer the NEXT launch accumulates into (see FusedArgs::arow)
        double* z = arow + (size_t)arow_zero(kPro, it) * f.n_kf * kStride;
        for (int i = b * kFT + tid; i < f.n_kf * kStride; i += (int)gridDim.x * kFT) z[i] = 0.0;
    }
    if (kPro && kEcopy) f.lpos[base + tid] = make_double4(PL.x, PL.y, PL.z, 0.0);
    lpos[3 * tid] = PL.x;
    lpos[3 * tid + 1] = PL.y;
    lpos[3 * tid + 2] = PL.z;
    if (tid < kFK) {
        s_ke[tid] = ke;
        s_kd[tid] = kd;
    }
    FKT(1);
    if (!drow) __syncthreads();  // s_ke / s_kd
    if (!kPro) {
        // ---- combine: S of entry j, term t = the row's partial slots summed in slot order
        for (int pr = tid; !drow && pr < n_ent * kNTerms; pr += kFT) {
            const int j = pr / kNTerms, t = pr - j * kNTerms;
            const int4 e = s_ke[j];
            if (e.x < 0) continue;  // a hole in the entry positions
            if (f.rowpart) {  // sharded: the all-reduced row (identical on every rank)
                kslot[j * kLdsStride + t] = f.rowpart[(size_t)(e.x & 0x3fffffff) * kStride + t];
                continue;
            }
            if (arow && (it > 0 || f.apro)) {  // the row summed by the previous launch's atomics
                kslot[j * kLdsStride + t] = arow[((size_t)arow_rd(it) * f.n_kf + (e.x & 0x3fffffff)) * kStride + t];
                continue;
            }
            const double* src = part_in + ((size_t)(e.x & 0x3fffffff) * f.maxl) * kStride + t;
            constexpr int kCB = kFT <= kFTSmall ? 32 : 16;  // slots per batch of loads (one round at C3)
            double acc = 0.0;
            for (int i0 = 0; i0 < e.y; i0 += kCB) {
                double v[kCB];
#pragma unroll
                for (int q = 0; q < kCB; ++q) v[q] = i0 + q < e.y ? src[(size_t)(i0 + q) * kStride] : 0.0;
#pragma unroll
                for (int q = 0; q < kCB; ++q) acc += v[q];  // (+0.0 past the end: exact)
            }
            kslot[j * kLdsStride + t] = acc;
        }
        // ---- stop rule of iteration it (workgroup 0): totals over every partial slot
        if (b == f.stop_b) {
            double tot = 0.0, cnt = 0.0;
            if (f.rowpart || (arow && (it > 0 || f.apro))) {
                const double* rows = f.rowpart ? f.rowpart : arow + (size_t)arow_rd(it) * f.n_kf * kStride;
                for (int q = tid; q < a.n_kf; q += kFT) {
                    tot += rows[(size_t)q * kStride + 27];
                    cnt += rows[(size_t)q * kStride + 28];
                }
            } else {
                const double2* cp = f.costpart + (size_t)(it & 1) * f.n_part;
                for (int q0 = 0; q0 < f.n_part; q0 += 2 * kFT) {  // (two loads in flight per thread)
                    const int q1 = q0 + tid, q2 = q0 + kFT + tid;
                    const double2 c1 = q1 < f.n_part ? cp[q1] : make_double2(0.0, 0.0);
                    const double2 c2 = q2 < f.n_part ? cp[q2] : make_double2(0.0, 0.0);
                    tot += c1.x;
                    cnt += c1.y;
                    tot += c2.x;
                    cnt += c2.y;
                }
            }
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) {
                tot += __shfl_xor(tot, m, 64);
                cnt += __shfl_xor(cnt, m, 64);
            }
            if (lane == 0) {
                red[wv] = tot;
                red[kFW + wv] = cnt;
            }
        }
    }
    if (!drow) __syncthreads();  // (kslot's combined rows, red[])
    FKT(2);
    // ---- pose solve of the entries (local_ba.cpp:163-173); owners publish
    if (ke.x >= 0) {
        double* sl = kslot + tid * kLdsStride;
        double T[8], R[9], C[4];
#pragma unroll
        for (int j = 0; j < 8; ++j) T[j] = ev[j];
#pragma unroll
        for (int j = 0; j < 4; ++j) C[j] = ev[8 + j];
        if (!kPro) {
            double S[kNTerms];
#pragma unroll
            for (int t = 0; t < kNTerms; ++t) S[t] = drow ? Sd[t] : sl[t];
            solve_pose(a, (int)ev[12], S, T, R);
            if (ke.x & (1 << 30)) {
                double* Tout = pose_out(a, it) + 8 * (size_t)(ke.x & 0x3fffffff);
#pragma unroll
                for (int j = 0; j < 8; ++j) Tout[j] = T[j];
            }
            if (kEcopy) {
                double4* E4 = reinterpret_cast<double4*>(f.epose + ((size_t)b * kFK + tid) * 16);
                E4[0] = make_double4(T[0], T[1], T[2], T[3]);
                E4[1] = make_double4(T[4], T[5], T[6], T[7]);
            }
        } else {
            rot_from_quat(T, R);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) sl[j] = T[j];
#pragma unroll
        for (int j = 0; j < 9; ++j) sl[8 + j] = R[j];
#pragma unroll
        for (int j = 0; j < 4; ++j) sl[17 + j] = C[j];
    }
    auto stop_from_red = [&] {
        double tot = 0.0, cnt = 0.0;
        for (int w2 = 0; w2 < kFW; ++w2) {
            tot += red[w2];
            cnt += red[kFW + w2];
        }
        stop_rule(a, it, tot, (int)cnt);
    };
    if (!kPro && !drow && b == f.stop_b && tid == 0) stop_from_red();
    __syncthreads();
    if (drow && b == f.stop_b && tid == 0) stop_from_red();  // (every wave's red[] is in after the barrier)
    FKT(3);
    // ---- landmark stage of iteration it (local_ba.cpp:176-238)
    if (!kPro) {
        double h[9];
        const D3 PO{lpos[3 * orec.y], lpos[3 * orec.y + 1], lpos[3 * orec.y + 2]};
        const bool ok = obs_terms<kFT <= kFTSmall>(a, PO, orec.x, ouv, kslot, kLdsStride, kslot + 8, kLdsStride,
                                                   kslot + 17, kLdsStride, h);
#pragma unroll
        for (int j = 0; j < 9; ++j) terms[j * kFT + tid] = h[j];
        tcount[tid] = (has_o && ok) ? 1 : 0;
        __syncthreads();
        if (own) {
            double hs[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            int obs = 0;
            for (int r = run.x; r < run.y; ++r) {
#pragma unroll
                for (int j = 0; j < 9; ++j) hs[j] += terms[j * kFT + r];
                obs += tcount[r];
            }
            // (lslot made opaque until here: otherwise its address arithmetic is hoisted next to its
            // load, whose wait — vmcnt, in issue order — then holds wave 0 for the rows behind it)
            asm volatile("" : "+v"(lslot));
            PL = lm_update(a, lslot, PL, hs, obs);
            if (kEcopy) f.lpos[base + tid] = make_double4(PL.x, PL.y, PL.z, 0.0);
            lpos[3 * tid] = PL.x;
            lpos[3 * tid + 1] = PL.y;
            lpos[3 * tid + 2] = PL.z;
        }
        __syncthreads();
    }
    FKT(4);
    // ---- pose stage of iteration it + 1: wave wv takes entries wv, wv + kFW, ...
    if (!pose_next) return;
    int r = 0;
    FKT(6);
    for (int j = wv; j < n_ent; j += kFW) {
        const int4 e = s_ke[j];
        const int dst = s_kd[j];
        const int nr = (e.w - e.z + 63) >> 6;
        if (nr == 0) continue;
        const double* T = kslot + j * kLdsStride;
        const double* R = T + 8;
        const double* C = T + 17;
        double v[kStride];
#pragma unroll
        for (int t = 0; t < kStride; ++t) v[t] = 0.0;
        if constexpr (kCmp) {
            // Projection and gate (local_ba.cpp:131-146) for every observation; the Jacobian and
            // normal-equation half (:148-159) only for the accepted ones, 64 at a time from a per-wave
            // ring in LDS: after the first iterations most observations fail the gate (the
            // reference's step sign grows the residuals), so most rounds skip that half.  Accepted
            // observations keep their order within a lane slot only up to the summation order of
            // the terms (the tolerance-level change documented in DESIGN.md §2).
            double* qw = qbuf + (size_t)wv * kQ * kQRec;
            int qh = 0, qn = 0;  // ring head (next write) and queued count (wave-uniform)
            auto drain = [&](int n) {  // terms of the n oldest queued observations
                const int slot = (qh - qn + lane + kQ) & (kQ - 1);
                const double4 r0 = *reinterpret_cast<const double4*>(qw + (size_t)slot * kQRec);
                const double4 r1 = *reinterpret_cast<const double4*>(qw + (size_t)slot * kQRec + 4);
                // lanes past n read stale ring entries (or never-written LDS): finite stand-ins with
                // weight 0, so their terms are exactly +-0.0
                const bool use = lane < n;
                pose_obs_terms(C, use ? r0.x : 0.0, use ? r0.y : 0.0, use ? r0.z : 1.0, use ? r0.w : 1.0,
                               use ? r1.x : 0.0, use ? r1.y : 0.0, use ? r1.z : 0.0, v);
                qn -= n;
            };
            for (int q = 0; q < nr; ++q, ++r) {
                const double2 uv = u0;
                const double4 P4 = p0;
                if (r + 1 < wrounds) {
                    u0 = f.pobs_uv[wstart + 64 * (r + 1) + lane];
                    p0 = f.pobs_p[wstart + 64 * (r + 1) + lane];
                }
                const bool valid = e.z + 64 * q + lane < e.w;
                const int code = (int)P4.w;
                const D3 P = code >= 0 ? D3{lpos[3 * code], lpos[3 * code + 1], lpos[3 * code + 2]} : D3{P4.x, P4.y, P4.z};
                const D3 pc = rt_apply(R, T + 4, P);
                const bool front = pc.z > 1e-6;
                const double inv_z = frcp(front ? pc.z : 1.0);
                const double e0 = uv.x - (C[0] * (pc.x * inv_z) + C[2]);
                const double e1 = uv.y - (C[1] * (pc.y * inv_z) + C[3]);
                const double e2 = e0 * e0 + e1 * e1;
                const bool ok = valid && front && !(e2 > a.max_err2);
                const double w = ok ? (e2 > a.huber2 ? a.huber * frsq(e2) : 1.0) : 0.0;
                v[27] = fma(w, e2, v[27]);
                v[28] += ok ? 1.0 : 0.0;
                const unsigned long long m = __ballot(ok);
                const int slot = ok ? ((qh + mbcnt_lo_hi(m)) & (kQ - 1)) : -1;
                if (ok) {
                    double4* rec = reinterpret_cast<double4*>(qw + (size_t)slot * kQRec);
                    rec[0] = make_double4(pc.x, pc.y, pc.z, inv_z);
                    rec[1] = make_double4(e0, e1, w, 0.0);
                }
                const int na = __popcll(m);
                qh = (qh + na) & (kQ - 1);
                qn += na;
                if (qn >= 64) {
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    drain(64);
                }
            }
            if (qn > 0) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                drain(qn);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // (the ring is reused by the next entry)
            __builtin_amdgcn_wave_barrier();
        } else {
        for (int q = 0; q < nr; ++q, ++r) {
            const double2 uv = u0;
            const double4 P4 = p0;
            if (r + 1 < wrounds) {
                // only the lanes of the next round that hold an observation load (the entries'
                // 64-aligned padding stays in memory): the next round is this entry's or the first
                // of the wave's next entry with rounds
                int lim = f.padskip ? e.w - (e.z + 64 * (q + 1)) : 64;
                if (f.padskip && q + 1 >= nr) {
                    int jn = j + kFW;
                    int4 en = s_ke[jn < kFK ? jn : j];
                    while (jn < n_ent && ((en.w - en.z + 63) >> 6) == 0) {
                        jn += kFW;
                        en = s_ke[jn < kFK ? jn : j];
                    }
                    lim = en.w - en.z;
                }
                if (lane < lim) {
                    u0 = f.pobs_uv[wstart + 64 * (r + 1) + lane];
                    p0 = f.pobs_p[wstart + 64 * (r + 1) + lane];
                } else {
                    u0 = make_double2(0.0, 0.0);
                    p0 = make_double4(0.0, 0.0, 0.0, 0.0);
                }
            }
            const bool valid = e.z + 64 * q + lane < e.w;
            if (kFT <= kFTSmall || valid) {  // (256 / 512: padding lanes run too, weight 0 — no branch)
                const int code = (int)P4.w;
                const D3 P = code >= 0 ? D3{lpos[3 * code], lpos[3 * code + 1], lpos[3 * code + 2]}
                                       : D3{P4.x, P4.y, P4.z};
                pose_obs_accum<kFT <= kFTSmall>(a, T, R, C, P, uv, v, valid);
            }
        }
        }
        if (j == wv) FKT(7);
        const double tot = wave_sum32(v);
        if (arow && (!kPro || f.apro)) {  // (iteration it + 1's row sums, see FusedArgs::arow)
            if ((lane & 1) == 0 && (lane >> 1) < kNTerms)
                unsafeAtomicAdd(arow + ((size_t)arow_wr(kPro, it) * f.n_kf + (e.x & 0x3fffffff)) * kStride + (lane >> 1),
                                tot);
            continue;
        }
        if ((lane & 1) == 0) part_out[(size_t)dst * kStride + (lane >> 1)] = (lane >> 1) < kNTerms ? tot : 0.0;
        if (lane == 54 || lane == 56)  // terms 27 (cost) and 28 (observations)
            reinterpret_cast<double*>(f.costpart + (size_t)((it + 1) & 1) * f.n_part + dst)[(lane - 54) >> 1] = tot;
    }
    if (!kPro && it == 1) VX_KTW(8, 8);  // (trace build: each wave's pose stage done)
    FKT(5);
}

}  // namespace
}  // namespace vx
