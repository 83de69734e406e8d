// ba_win_kernel.hpp — device code of ba.hip, included by it alone after ba_fused_kernel.hpp: the
// persistent window k_ba_win (one launch per run), its argument record WinArgs and the comment that
// specifies its hand-off protocol.  The -DVX_WIN_TRACE_LM / -DVX_WIN_TRACE_SOLVE variants of the Makefile's
// trace-lm / trace-solve targets are read here.
#pragma once
#include "ba_fused_kernel.hpp"

namespace vx {
namespace {

using namespace vx::ba;

// ------------------------------------------------------------------ persistent window (k_ba_win)
// The prologue and every iteration of one LocalBA window in ONE launch (round 6, VERDICT r5 #2a).
// k_ba_iter's workgroups already exchange nothing but the keyframe rows: a workgroup solves the poses
// of its own <= kFK keyframe entries from their rows, updates its own landmarks and produces the next
// iteration's pose-stage terms of its landmarks' observations for those rows.  So the launch
// boundary between iterations is replaced by point-to-point hand-offs, not a grid barrier, and the
// handed-off data is its own flag (cdna_hip_programming.md Guideline 16, form R2):
//   - a (workgroup, keyframe) entry with observations owns one partial slot of its row per iteration
//     (the slot k_ba_iter's partial buffer uses: kent's second record, k * maxl + rank).  After the
//     entry's wave sum the lanes that hold its 29 terms store each double as two 8-byte granules
//     {32-bit half, 32-bit tag} into part[iteration][slot] (relaxed agent-scope atomic stores: sc1,
//     write-through; one aligned 8-byte store per granule, so a granule is never torn).  No atomic
//     add, no drain, no barrier, no counter: a wave's entry is on its way as soon as it is summed;
//   - every wave of a workgroup sweeps the rows of the entries dealt to it (as in the pose stage):
//     one lane per term, the two halves of the wave on alternate slots, every slot's granules loaded
//     (sc1 loads to registers: they bypass this CU's L1) before any tag is checked, then again — only
//     the granules still missing: re-reading whole rows while the last producers are awaited made
//     each poll as slow as a full sweep, 0.0503 against 0.0489 ms, r07 — until every tag is the
//     run's; then the slots are summed in slot order from 0.0 — k_ba_iter's slot combine,
//     so every run of a plan gives the same bits — and the entry's 29 sums are staged in LDS;
//   - behind one workgroup barrier wave 0 solves every entry of the workgroup, lane p the entry
//     at position p (k_ba_iter's form).  Solved by lane i of each wave for that wave's i-th
//     entry, a C3 workgroup's 5-8 entries made up to eight waves issue the whole solve_pose
//     stream for one active lane each, two of them per SIMD; now it is issued once.  Wave 1, on
//     another SIMD, runs the stop rule beside it.  LDS between the two barriers of phase A
//     (B1: sums staged, B2: the phase's end):
//       `terms` as staging: an entry's sums are written by its sweeping wave before B1, read
//         by wave 0 between B1 and B2 and by nobody else; the landmark stage rewrites `terms`
//         only behind B2, and its own reads of `terms` end at its closing barrier, before the
//         next sweep can stage anything;
//       pose sets: wave 0 reads set (it - 1) & 1 (last written before the previous B2, or in
//         the prologue) and writes set it & 1 between B1 and B2; every wave has left pose stage
//         `it` (which reads set (it - 1) & 1) before B1, and set it & 1 is first read behind B2;
//       s_fault: set by a wave whose sweep ran out before B1, so wave 0, which reads it behind
//         B1, does not solve from incomplete sums; wave 1 may set it between B1 and B2 (the stop
//         rule's wait ran out) while wave 0 reads it — either value is fine, the run is void and
//         every wave leaves behind B2, where all of them read the same value;
//       s_act: written by wave 1 between B1 and B2, read by every wave behind B2 and not again
//         after the landmark stage's barriers, which precede the next B1;
//     every wave executes B1 and B2 once per iteration on every path (a sweep that ran out, a
//     workgroup without entries, holes, one iteration, an early stop, the test's fault): neither
//     stands under a condition, and the loop is left only behind B2 on workgroup-wide values.
//     Between B1 and B2 every thread also requests what the landmark stage reads first (its
//     observation record, its landmark's position in lpos, its run): loop-invariant or written
//     only inside the landmark stage, whose closing barrier precedes B1, and next written behind
//     B2.  (In place of B1, a generation word per wave in LDS that wave 0 polls measured slower:
//     LocalBA alone 0.0472-0.0475 against 0.0467-0.0468 ms, r15);
//   - the tag is the run's generation + 1 (w.gen, on the device: graph replays see it), never 0.
//     Granules are per iteration (no reuse inside a run) and runs of one plan are stream-ordered, so
//     a granule with this run's tag was written in this run for this iteration; whatever an earlier
//     run (or an iteration an early stop skipped) left carries a smaller tag, the build's memset 0.
//     Nothing is cleared between runs.  A plan whose generation nears 2^31 runs reports a fault
//     instead of wrapping: vx_ba_plan_fetch then keeps it on the per-iteration launches;
//   - ordering: a matching tag arrived in the same 8-byte load as its half, so the value is the
//     producer's; no other byte is handed over (poses, landmarks and plan tables are the
//     workgroup's own or written before the launch).  fence(acquire, "wavefront") after a sweep
//     emits nothing and only keeps the compiler from moving loads above the poll;
//   - the stop rule of iteration i - 1 (whether iteration i runs) needs the cost / count terms of
//     every row of iteration i - 1: the row's owner publishes them from its own sum as tagged
//     granules (stop[i - 1][row]); wave 1 sweeps them one iteration later (almost always already
//     there), sums them in a fixed order and decides — every workgroup the same, from the same
//     values; workgroup 0 writes the run's statistics;
//   - workgroup 0 bumps the generation at its end.  Every workgroup stores the tag into hello[b]
//     right after reading the generation, and workgroup 0's wave 1 sweeps hello[] in iteration 0
//     (max_iter >= 1, and a stop is decided in iteration 1 at the earliest): it cannot reach its end
//     before every workgroup has read the generation, whatever the entries' topology, M = 1 and
//     early stops included.
// Everything a workgroup loads that no iteration changes (block / entry records, landmark-stage
// observations, the landmarks' slots and runs, the first pose-stage round) is loaded once; the
// entries' poses and the landmark positions stay in registers / LDS.  Every workgroup must be
// resident at once (nb <= CUs, one 512-thread workgroup per CU); every wait is bounded
// (kWinSpinTicks): a wait that runs out sets the state's fault flag, every workgroup leaves, and
// vx_ba_plan_fetch re-runs the window with the per-iteration launches (plan->win_off) — two
// persistent windows on one device at once could otherwise hold each other's compute units.
typedef unsigned long long wgran;  // {value half (low 32 bits), tag (high 32 bits)}
struct WinArgs {
    wgran* part;         // [max_iter][n_kf * maxl + 1][kStride][2] the rows' partial slots
    wgran* stop;         // [max_iter][n_kf][4] the owners' cost | count terms of their rows
    unsigned* hello;     // [workgroups] tag once the workgroup has read the generation
    int* gen;            // run generation, bumped by workgroup 0 at the run's end
    int* fault;          // set when a wait ran out (every workgroup then leaves)
    int bias;            // $VX_BA_WIN_TEST_FAULT: row 0 waits for one more slot, which nobody fills
};
constexpr long long kWinSpinTicks = 20'000'000;  // 200 ms of the 100 MHz wall clock
constexpr int kWinGenMax = 0x7ffffff0;           // (tags stay below 2^31: no wrap-around)
// slots per lane and sweep pass (two lanes per term: 2 kWinSB slots a pass; C3's rows have ~17).
// 16 — every row in one pass — measured slower: LocalBA alone 0.0534 against 0.0503 ms, r07
constexpr int kWinSB = 8;
constexpr int kWinSStride = kStride + 1;  // staged row sums in LDS (odd: the solving lanes' reads spread)
// k_ba_win's LDS: k_ba_iter's plus a second set of pose slots
constexpr size_t win_lds(int ft) {
    return fused_lds(ft) + (size_t)kFK * kLdsStride * sizeof(double) + (size_t)ft * (16 + 16 + 12);
}
static_assert(win_lds(kFTSmall) <= 160 * 1024, "k_ba_win LDS exceeds gfx950's 160 KB per workgroup");
static_assert(kFK * kWinSStride <= 9 * kFTSmall, "k_ba_win stages the row sums in the landmark stage's terms");

__device__ __forceinline__ int ld_sc1(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned ld_sc1(const unsigned* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ wgran ld_sc1(const wgran* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// one double as its two tagged granules (each an aligned 8-byte sc1 store)
__device__ __forceinline__ void st_gran2(wgran* g, double v, unsigned tag) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v), t = (unsigned long long)tag << 32;
    __hip_atomic_store(g, t | (u & 0xffffffffull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(g + 1, t | (u >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double gran2_value(wgran lo, wgran hi) {
    return __longlong_as_double((long long)((lo & 0xffffffffull) | (hi << 32)));
}
// a sweep that found a tag missing: naps, and every 16th pass checks the fault word and the clock.
// Wave-uniform; true when the wait ran out or another workgroup reported a fault (the fault word is
// then set)
__device__ __forceinline__ bool win_spin_fail(int& k, long long t0, int* fault) {
    if ((++k & 15) == 0 && (ld_sc1(fault) || wall_clock64() - t0 > kWinSpinTicks)) {
        if ((threadIdx.x & 63) == 0) __hip_atomic_store(fault, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return true;
    }
    __builtin_amdgcn_s_sleep(1);  // (longer naps between polls measured the same: r06g)
    return false;
}

// (238 VGPRs, no scratch, two waves per SIMD.  Sized for three — 168 VGPRs, so that a third wave of
// the other streams' kernels fits beside it — it spills outside the observation rounds: LocalBA
// alone 0.067 against 0.054 ms, the C3 pipeline 0.074 against 0.063 ms/frame, r06i)
template <int kFT>
__global__ __launch_bounds__(kFT) void k_ba_win(BAArgs a, FusedArgs f, WinArgs w) {
    constexpr int kFW = kFT / 64;
    static_assert(kFW >= 2, "k_ba_win: wave 1 runs the stop rule");
    __builtin_amdgcn_s_setprio(3);
    extern __shared__ __attribute__((aligned(16))) double fl[];
    __shared__ int4 s_ke[kFK];
    __shared__ int s_kd[kFK];  // the entry's partial slot (k * maxl + rank; -1: no observations)
    __shared__ int s_act, s_fault;
    // two pose-slot sets (T 8 | R 9 | C 4 | flags per entry): iteration it solves from set (it - 1) & 1
    // into set it & 1, so a wave still in the previous pose stage (no barrier closes it) reads poses
    // the solve does not overwrite
    double* const ks0 = fl;                              // [2][kFK][kLdsStride]
    double* terms = ks0 + 2 * kFK * kLdsStride;          // [9][kFT]
    int* tcount = reinterpret_cast<int*>(terms + 9 * kFT);
    double* lpos = terms + 9 * kFT + kFT / 2;            // [kFT][3]
    // the landmark stage's per-thread records, loop-invariant: parked in LDS, not in registers
    // (k_ba_win keeps far more state live across its loop than one k_ba_iter launch)
    int4* s_orec = reinterpret_cast<int4*>(lpos + 3 * kFT);      // [kFT]
    double2* s_ouv = reinterpret_cast<double2*>(s_orec + kFT);    // [kFT]
    int* s_run = reinterpret_cast<int*>(s_ouv + kFT);             // [kFT][3]: r0, r1, slot
    const int tid = threadIdx.x, b = blockIdx.x, wv = tid >> 6, lane = tid & 63;
    const size_t base = (size_t)b * kFT;
    const int4* KE = f.kent + (size_t)b * kFK * 2;
    const int M = a.max_iter, nk = a.n_kf, nb = (int)gridDim.x;
    const int nslot = nk * f.maxl;  // (slot nslot: the one nobody fills, WinArgs::bias)
    // ---- loads: the run generation, then everything the window keeps (k_ba_iter's prologue loads
    // plus the landmark-stage records its iteration launches load again and again)
    const int gen = w.gen[0];
    const unsigned tag = (unsigned)gen + 1u;
    if (gen < 0 || gen >= kWinGenMax) {  // (every workgroup alike: the fetch falls back for good)
        if (tid == 0) __hip_atomic_store(w.fault, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    if (tid == 0) __hip_atomic_store(w.hello + b, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int wvu = __builtin_amdgcn_readfirstlane(wv);
    const int4 B = f.blk[(size_t)b * (1 + kFW / 2)];
    const int4 WB = f.blk[(size_t)b * (1 + kFW / 2) + 1 + (wvu >> 1)];
    int4 ke = make_int4(-1, 0, 0, 0);
    int kd = -1;
    if (tid < kFK) {
        ke = KE[2 * tid];
        kd = KE[2 * tid + 1].x;
    }
    const int4 orec0 = f.lobs_rec[base + tid];
    const double2 ouv0 = f.lobs_uv[base + tid];
    const int lslot0 = f.lm_slot[base + tid];
    const int2 run0 = f.lm_run[base + tid];
    D3 PL;
    {
        const double* P = a.lm_pos0 + 4 * (size_t)lslot0;
        PL = {P[0], P[1], P[2]};
    }
    const int wstart = (wvu & 1) ? WB.z : WB.x, wrounds = (wvu & 1) ? WB.w : WB.y;
    // (each wave's first pose-stage round, requested again before every pose stage: kept in
    // registers across the loop it would cost the registers the landmark stage needs)
    double2 u0 = make_double2(0, 0);
    double4 p0 = make_double4(0, 0, 0, 0);
    auto first_round = [&] {
        if (wrounds > 0) {
            u0 = f.pobs_uv[wstart + lane];
            p0 = f.pobs_p[wstart + lane];
        }
    };
    first_round();
    // the entry's state lives in its LDS slot (T 8 | R 9 | C 4 | flags), not in registers
    double ev[13];
    const int row = ke.x & 0x3fffffff;
    if (tid < kFK && ke.x >= 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) ev[j] = a.kf_pose0[8 * (size_t)row + j];
#pragma unroll
        for (int j = 0; j < 4; ++j) ev[8 + j] = a.kf_intr[4 * row + j];
        ev[12] = (double)a.kf_flags[row];
    }
    if (b == 0 && tid < 16) {  // (the statistics of this run, as stop_rule(0) starts them)
        a.state->cost[tid] = 0.0;
        a.state->obs[tid] = 0;
    }
    const int n_lm = B.x, n_ob = B.y, n_ent = B.z;
    const bool has_o = tid < n_ob, own = tid < n_lm;
    lpos[3 * tid] = PL.x;
    lpos[3 * tid + 1] = PL.y;
    lpos[3 * tid + 2] = PL.z;
    s_orec[tid] = orec0;
    s_ouv[tid] = ouv0;
    s_run[3 * tid] = run0.x;
    s_run[3 * tid + 1] = run0.y;
    s_run[3 * tid + 2] = lslot0;
    if (tid < kFK) {
        s_ke[tid] = ke;
        s_kd[tid] = kd;
    }
    if (tid == 0) s_fault = 0;
    if (tid < kFK && ke.x >= 0) {  // iteration 0's pose stage reads the initial poses (set 1)
        double Rm[9];
        rot_from_quat(ev, Rm);
        double* sl = ks0 + (kFK + tid) * kLdsStride;
        double* sl0 = ks0 + tid * kLdsStride;
#pragma unroll
        for (int j = 0; j < 8; ++j) sl[j] = ev[j];
#pragma unroll
        for (int j = 0; j < 9; ++j) sl[8 + j] = Rm[j];
#pragma unroll
        for (int j = 0; j < 4; ++j) sl[17 + j] = sl0[17 + j] = ev[8 + j];
        sl[21] = sl0[21] = ev[12];
    }
    __syncthreads();

    // ---- pose stage of iteration `itn` from the poses in set (itn - 1) & 1 and the landmarks in lpos,
    // each entry's terms into its own partial slot of iteration itn as tagged granules: that store is
    // the hand-off.  No barrier closes the stage: the LDS it reads (s_ke / s_kd: never rewritten; pose
    // set (itn - 1) & 1: the next solve writes the other set; lpos: next written behind phase A's
    // barrier) is not written before every wave has passed the next barrier, and what the next
    // phase A writes (the staged sums in `terms`, s_act) it does not read.
    auto pose_stage = [&](int itn) {
        int r = 0;
        wgran* const Pn = w.part + (size_t)itn * (nslot + 1) * (2 * kStride);
        const double* const kslot = ks0 + ((itn - 1) & 1) * kFK * kLdsStride;
        for (int j = wv; j < n_ent; j += kFW) {
            const int4 e = s_ke[j];
            const int nr = (e.w - e.z + 63) >> 6;
            if (nr == 0) continue;
            const double* T = kslot + j * kLdsStride;
            const double* Rr = T + 8;
            const double* C = T + 17;
            double v[kStride];
#pragma unroll
            for (int t = 0; t < kStride; ++t) v[t] = 0.0;
            for (int q = 0; q < nr; ++q, ++r) {
                const double2 uv = u0;
                const double4 P4 = p0;
                if (r + 1 < wrounds) {
                    int lim = e.w - (e.z + 64 * (q + 1));
                    if (q + 1 >= nr) {  // the wave's next entry with rounds
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
                const int code = (int)P4.w;
                const D3 P = code >= 0 ? D3{lpos[3 * code], lpos[3 * code + 1], lpos[3 * code + 2]} : D3{P4.x, P4.y, P4.z};
                pose_obs_accum<true>(a, T, Rr, C, P, uv, v, valid);
            }
            const double tot = wave_sum32(v);
            const int kdj = s_kd[j];
            if ((lane & 1) == 0 && (lane >> 1) < kNTerms && kdj >= 0)
                st_gran2(Pn + ((size_t)kdj * kStride + (lane >> 1)) * 2, tot, tag);
        }
    };
    // ---- workgroup 0, iteration 0: every workgroup has read the generation (see the header)
    auto hello_sweep = [&]() -> int {
        const long long t0 = wall_clock64();
        for (int spins = 0;;) {
            bool ok = true;
            for (int q = lane; q < nb; q += 64) ok &= ld_sc1(w.hello + q) == tag;
            if (__all(ok)) return 1;
            if (win_spin_fail(spins, t0, w.fault)) return -1;
        }
    };
    // ---- stop rule of iteration ip (local_ba.cpp:240-247) from the owners' cost / count terms of
    // every row of iteration ip, by wave 1 of every workgroup (the same values summed in the same
    // order: the same decision everywhere)
    double last = 1.7976931348623157e308;
    // (d: the first 64 rows' granules, requested by the caller ahead of its own sweep so that their
    // round trip is not in front of it; they are the first poll)
    auto decide_issue = [&](int ip, wgran (&d)[4]) {
        const wgran* const g = w.stop + ((size_t)ip * nk + (lane < nk ? lane : 0)) * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i] = ld_sc1(g + i);
    };
    auto decide = [&](int ip, const wgran (&d)[4]) -> int {
        const wgran* const sp = w.stop + (size_t)ip * nk * 4;
        const long long t0 = wall_clock64();
        int spins = 0;
        double tot = 0.0, cn = 0.0;
        for (int q0 = 0; q0 < nk; q0 += 64) {  // (lane-strided, as the sums of complete rows were)
            const bool live = q0 + lane < nk;
            const wgran* const g = sp + (size_t)(live ? q0 + lane : 0) * 4;
            wgran c0 = d[0], c1 = d[1], n0 = d[2], n1 = d[3];
            for (bool first = q0 == 0;; first = false) {
                if (!first) c0 = ld_sc1(g), c1 = ld_sc1(g + 1), n0 = ld_sc1(g + 2), n1 = ld_sc1(g + 3);
                const bool ok = !live || ((unsigned)(c0 >> 32) == tag && (unsigned)(c1 >> 32) == tag &&
                                          (unsigned)(n0 >> 32) == tag && (unsigned)(n1 >> 32) == tag);
                if (__all(ok)) break;
                if (win_spin_fail(spins, t0, w.fault)) return -1;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            tot += live ? gran2_value(c0, c1) : 0.0;
            cn += live ? gran2_value(n0, n1) : 0.0;
        }
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
            tot += __shfl_xor(tot, m, 64);
            cn += __shfl_xor(cn, m, 64);
        }
        const int tobs = (int)cn;
        const bool stop = tobs == 0 || fabs(last - tot) < 1e-6 * last;
        if (!stop) last = tot;
        if (b == 0 && lane == 0) {
            BAState* s = a.state;
            if (ip < 16) {
                s->cost[ip] = tot;
                s->obs[ip] = tobs;
            }
            s->iterations = ip + 1;
            s->last_cost = last;
            if (!stop && ip + 1 < M)
                s->active[ip + 1] = 1;
            else
                for (int k = ip + 1; k <= M; ++k) s->active[k] = 0;
        }
        return stop ? 0 : 1;
    };

    VX_KT(0);
    pose_stage(0);  // (iteration 0's pose stage: k_ba_iter's prologue)
    if (wv == 0) VX_KT(15);
    for (int it = 0; it < M; ++it) {
        double* const kslot = ks0 + (it & 1) * kFK * kLdsStride;
        const double* const kprev = ks0 + ((it + 1) & 1) * kFK * kLdsStride;
        // ---- A: every wave sweeps the partial slots of its entries' rows (entries dealt as in the
        // pose stage), sums them in slot order and stages the sums; behind a barrier wave 0 solves
        // every entry while wave 1 (another SIMD) decides whether iteration it runs (the stop rule of
        // it - 1: its granules have had an iteration to arrive and are requested ahead of the wave's
        // own sweep)
        wgran dgr[4] = {0, 0, 0, 0};
        if (wv == 1 && it > 0) decide_issue(it - 1, dgr);
        {
            const int h = lane >> 5, t = lane & 31;  // half h of the wave: slots s0 + 2 i + h, term t
            const wgran* const Pi = w.part + (size_t)it * (nslot + 1) * (2 * kStride);
            double* const stage = terms;  // [kFK][kWinSStride] (the landmark stage writes terms behind the barrier)
            const long long t0 = wall_clock64();
            int spins = 0;
            bool okw = true;
            __builtin_amdgcn_s_setprio(0);
            for (int j = wv; j < n_ent && okw; j += kFW) {
                const int4 e = s_ke[j];
                if (e.x < 0) continue;  // a hole in the entry positions
                const int erow = e.x & 0x3fffffff;
                const int ns = e.y + (erow == 0 ? w.bias : 0);
                double acc = 0.0;
                for (int s0 = 0; s0 < ns && okw; s0 += 2 * kWinSB) {
                    wgran g0[kWinSB], g1[kWinSB];
                    // have: bit i = the lane's slot i is in (both tags matched) or is nothing to wait for
                    unsigned have = 0;
#pragma unroll
                    for (int i = 0; i < kWinSB; ++i) {
                        g0[i] = g1[i] = 0;
                        if (!(s0 + 2 * i + h < ns && t < kNTerms)) have |= 1u << i;
                    }
                    for (;;) {
                        // every missing slot's loads go out before any tag is checked; a pass asks
                        // again only for what the pass before did not find (a matched granule is
                        // final), so the passes that wait for the last producers are a few loads
#pragma unroll
                        for (int i = 0; i < kWinSB; ++i)
                            if (!((have >> i) & 1)) {
                                const int q = s0 + 2 * i + h;
                                const int slot = q < e.y ? erow * f.maxl + q : nslot;
                                const wgran* g = Pi + ((size_t)slot * kStride + t) * 2;
                                g0[i] = ld_sc1(g);
                                g1[i] = ld_sc1(g + 1);
                            }
#pragma unroll
                        for (int i = 0; i < kWinSB; ++i)
                            if (!((have >> i) & 1) && (unsigned)(g0[i] >> 32) == tag && (unsigned)(g1[i] >> 32) == tag)
                                have |= 1u << i;
                        if (__all(have == (1u << kWinSB) - 1)) break;
                        if (win_spin_fail(spins, t0, w.fault)) {
                            okw = false;
                            break;
                        }
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // (no load moves above the poll)
                    // slot order from 0.0, as k_ba_iter's slot combine (+0.0 past the end: exact);
                    // the sum is lane t's (half 0), which gets the odd slots from lane t + 32
#pragma unroll
                    for (int i = 0; i < kWinSB; ++i) {
                        const bool live = s0 + 2 * i + h < ns && t < kNTerms;
                        const double v = live ? gran2_value(g0[i], g1[i]) : 0.0;
                        const double vo = __shfl(v, t + 32, 64);
                        acc += v;
                        acc += vo;
                    }
                }
                if (lane < kNTerms) stage[j * kWinSStride + lane] = acc;
                // the row's owner hands its cost / count terms to the stop rule
                if (okw && (e.x & (1 << 30)) && (lane == 27 || lane == 28))
                    st_gran2(w.stop + ((size_t)it * nk + erow) * 4 + (lane - 27) * 2, acc, tag);
            }
            __builtin_amdgcn_s_setprio(3);
#if !defined(VX_WIN_TRACE_LM) && !defined(VX_WIN_TRACE_SOLVE)
            if (wv == 0 && it < 5) VX_KT(1 + 3 * it);
#endif
            if (!okw && lane == 0) s_fault = 1;
        }
        // ---- every wave's sums are staged (and a sweep that ran out has set s_fault): wave 0 solves,
        // lane p the entry at position p, as k_ba_iter does — one solve_pose stream per workgroup on
        // one SIMD, not one per wave for a single lane each
        __syncthreads();
#ifdef VX_WIN_TRACE_SOLVE  // (trace variant: slot 1 + 3 it = every wave's sums staged, 3 + 3 it = solve done)
        if (wv == 0 && it < 5) VX_KT(1 + 3 * it);
#endif
        // the landmark stage's first two LDS levels do not depend on the new poses (lpos is written
        // only inside the landmark stage, behind barriers of its own): requested here, so that the
        // waves that wait for wave 0's solve have them when the barrier opens
        const int4 orec = s_orec[tid];
        const double2 ouv = s_ouv[tid];
        const D3 PO{lpos[3 * orec.y], lpos[3 * orec.y + 1], lpos[3 * orec.y + 2]};
        const int r0 = s_run[3 * tid], r1 = s_run[3 * tid + 1], lslot = s_run[3 * tid + 2];
        if (tid < kFK && ke.x >= 0 && !s_fault) {
            const double* const stage = terms;
            double S[kNTerms];
#pragma unroll
            for (int q = 0; q < kNTerms; ++q) S[q] = stage[tid * kWinSStride + q];
            double* sl = kslot + tid * kLdsStride;
            const double* sp = kprev + tid * kLdsStride;
            double T[8], Rm[9];
#pragma unroll
            for (int j = 0; j < 8; ++j) T[j] = sp[j];
            solve_pose(a, (int)sp[21], S, T, Rm);
#pragma unroll
            for (int j = 0; j < 8; ++j) sl[j] = T[j];
#pragma unroll
            for (int j = 0; j < 9; ++j) sl[8 + j] = Rm[j];
        }
#ifdef VX_WIN_TRACE_SOLVE
        if (wv == 0 && it < 4) VX_KT(3 + 3 * it);
#endif
        if (wv == 1) {
            __builtin_amdgcn_s_setprio(0);  // (a polling wave leaves the SIMD to co-resident waves)
            const int act = it == 0 ? (b == 0 ? hello_sweep() : 1) : decide(it - 1, dgr);
            __builtin_amdgcn_s_setprio(3);
            if (lane == 0) {
                s_act = act > 0;
                if (act < 0) s_fault = 1;
            }
        }
        __syncthreads();
        if (wv == 0 && it < 5) VX_KT(2 + 3 * it);
        if (s_fault || !s_act) break;
        if (tid < kFK && ke.x >= 0 && (ke.x & (1 << 30))) {  // the owner publishes the pose
            double* Tout = pose_out(a, it) + 8 * (size_t)row;
            const double* sl = kslot + tid * kLdsStride;
#pragma unroll
            for (int j = 0; j < 8; ++j) Tout[j] = sl[j];
        }
        if (it + 1 < M) first_round();
        // ---- landmark stage of iteration it (local_ba.cpp:176-238), as k_ba_iter
        {
            double h[9];
            const bool ok = obs_terms<true>(a, PO, orec.x, ouv, kslot, kLdsStride, kslot + 8, kLdsStride, kslot + 17,
                                            kLdsStride, h);
#pragma unroll
            for (int j = 0; j < 9; ++j) terms[j * kFT + tid] = h[j];
            tcount[tid] = (has_o && ok) ? 1 : 0;
            __syncthreads();
            if (own) {
                double hs[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
                int obs = 0;
                const D3 P0{lpos[3 * tid], lpos[3 * tid + 1], lpos[3 * tid + 2]};
                for (int q = r0; q < r1; ++q) {
#pragma unroll
                    for (int j = 0; j < 9; ++j) hs[j] += terms[j * kFT + q];
                    obs += tcount[q];
                }
                const D3 P1 = lm_update(a, lslot, P0, hs, obs);
                lpos[3 * tid] = P1.x;
                lpos[3 * tid + 1] = P1.y;
                lpos[3 * tid + 2] = P1.z;
            }
            __syncthreads();
        }
#ifdef VX_WIN_TRACE_LM  // (trace variant: slot 1 + 3 it = the landmark stage done instead of rows ready)
        if (wv == 0 && it < 5) VX_KT(1 + 3 * it);
#endif
        if (it + 1 < M) pose_stage(it + 1);
#ifndef VX_WIN_TRACE_SOLVE
        if (wv == 0 && it < 4) VX_KT(3 + 3 * it);
#endif
    }
    // ---- the last iteration's statistics (a stop inside the loop wrote them), then the next run's
    // generation: workgroup 0's wave 1 swept hello[] in iteration 0, so every workgroup has read
    // this run's (a faulted run keeps its generation: the plan leaves the window for good)
    if (b == 0 && wv == 1 && !s_fault && s_act) {
        wgran dgr[4];
        decide_issue(M - 1, dgr);
        const int r = decide(M - 1, dgr);
        if (r < 0 && lane == 0) s_fault = 1;
    }
    if (b == 0 && wv == 1 && lane == 0 && !s_fault) w.gen[0] = gen + 1;
}

}  // namespace
}  // namespace vx
