// ransac_common.hpp — what PnP RANSAC (ransac.hip, 4 points, one model per hypothesis) and
// essential-matrix RANSAC (essential.hip, 5 points, up to 10 models) share: the counter stream and
// the sampler, RANSACUpdateNumIters, the block inlier count, a problem's hypothesis budget, the
// 64-wide replay of RANSACPointSetRegistrator::run, and the host side of a batch call.
#pragma once

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

#include "vx_internal.hpp"

namespace vx {
namespace rs {

constexpr int kMaxHyp = 4096;  // hypotheses per problem (max_iterations above it is refused)

// splitmix64: hypothesis h's attempt a is splitmix64(seed + 64 h + a)
__host__ __device__ inline uint64_t splitmix64(uint64_t x) {
    x += 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// hypothesis h's sample: K distinct indices below n (n >= 1) in at most 64 attempts, an attempt
// that repeats an index already taken skipped.  idx is read and written by unrolled compile-time
// selects only, so it stays in registers (free slots hold -1, which no attempt draws).
template <int K>
__device__ __forceinline__ bool draw_distinct(uint64_t seed, int h, int n, int (&idx)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) idx[k] = -1;
    int got = 0;
    for (int a = 0; a < 64 && got < K; ++a) {
        const uint64_t x = splitmix64(seed + (uint64_t)h * 64u + (uint64_t)a);
        const int i = (int)(((x >> 32) * (uint64_t)n) >> 32);
        bool dup = false;
#pragma unroll
        for (int k = 0; k < K; ++k) dup |= idx[k] == i;
        if (dup) continue;
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (k == got) idx[k] = i;
        ++got;
    }
    return got == K;
}

// RANSACUpdateNumIters for modelPoints = kPts (the power in a fixed multiplication order: the
// result is compared bit for bit with the oracle's)
template <int kPts>
__device__ int update_num_iters(double p, double ep, int max_iters) {
    static_assert(kPts == 4 || kPts == 5, "the power is spelled out per model size");
    p = fmax(p, 0.0);
    p = fmin(p, 1.0);
    ep = fmax(ep, 0.0);
    ep = fmin(ep, 1.0);
    double num = fmax(1.0 - p, DBL_MIN);
    const double x = 1.0 - ep;
    double denom;
    if constexpr (kPts == 4) denom = 1.0 - (x * x) * (x * x);
    else denom = 1.0 - ((x * x) * (x * x)) * x;
    if (denom < DBL_MIN) return 0;
    num = log(num);
    denom = log(denom);
    return denom >= 0.0 || -num >= (double)max_iters * -denom ? max_iters : (int)rint(num / denom);
}

// block-wide integer sum of per-thread flags (ballot + popcount per wave, LDS atomics)
__device__ __forceinline__ void block_count(int flag, int* lds_cnt) {
    const uint64_t b = __ballot(flag);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(lds_cnt, __popcll(b));
}

// hypotheses of a problem: its max_iterations, at most kMaxHyp and at most hmax, the hypothesis
// grid's x and the stride of the hypothesis records
__device__ __forceinline__ int hyp_budget(int max_iterations, int hmax) {
    return min(min(max(max_iterations, 0), kMaxHyp), hmax);
}

// RANSACPointSetRegistrator::run replayed by one wave over the counts of the (hypothesis, model)
// slots in order, f = kModels h + m, 64 at a time.  A slot can only be kept if its count beats
// every earlier count and kPts - 1: an in-wave prefix max + ballot finds those "records", which are
// then walked in order, each shrinking the iteration budget; the budget test applies when a record
// starts a new hypothesis, as in the sequential loop, and the walk ends at the first record of a
// hypothesis at or beyond the budget.  Straddle rule: a hypothesis whose kModels slots cross a
// block boundary may shrink the budget to <= h with a record in its first block; the sequential
// loop still scores the remaining models of a sample it has started, so the block loop goes on
// while a block can hold slots of last_h, the last hypothesis started, and loads those even at
// h >= niters (last_h < min(H, hlimit): at most H kModels / 64 rounds).  With kModels == 1 a
// hypothesis is one slot, last_h always lies in the block being walked, and neither the longer bound
// nor the h == last_h load ever adds a round or a slot: the plain loop.
// count_at(h, m) is the count of slot m of hypothesis h (-1: no model), called only for
// (h < niters || h == last_h) && h < hlimit, so records beyond a problem's budget are never read.
// Returns {hypothesis, model, hypotheses run, count} (hypothesis and model -1 when nothing is
// kept); *budget, if given, is the budget left after hlimit hypotheses (0: the loop has ended).
template <int kModels, int kPts, class CountAt>
__device__ int4 replay(CountAt count_at, int H, int n, double confidence, int hlimit = kMaxHyp,
                       int* budget = nullptr) {
    const int lane = threadIdx.x & 63;
    int niters = n >= kPts ? H : 0, best = -1, good = 0, last_h = -1;
    bool stop = false;
    for (int base = 0; !stop && base < max(min(niters, hlimit), last_h + 1) * kModels; base += 64) {
        const int f = base + lane;
        const int h = f / kModels, m = f - h * kModels;
        const int c = (h < niters || h == last_h) && h < hlimit ? count_at(h, m) : -1;
        int incl = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int y = __shfl_up(incl, off);
            if (lane >= off) incl = max(incl, y);
        }
        int excl = __shfl_up(incl, 1);
        if (lane == 0) excl = -1;
        uint64_t bits = __ballot(c > max(max(excl, good), kPts - 1));
        while (bits) {
            const int k = __ffsll((unsigned long long)bits) - 1;
            const int fk = base + k, hk = fk / kModels;
            if (hk != last_h && hk >= niters) {
                stop = true;
                break;
            }
            const int ck = __builtin_amdgcn_readlane(c, k);  // (k is the same in every lane: no LDS-routed shuffle)
            best = fk;
            last_h = hk;
            good = ck;
            niters = update_num_iters<kPts>(confidence, (double)(n - ck) / (double)n, niters);
            bits &= bits - 1;
        }
    }
    const int hb = best >= 0 ? best / kModels : -1;
    if (budget) *budget = stop ? 0 : niters;
    return make_int4(hb, best >= 0 ? best - hb * kModels : -1, best >= 0 ? max(niters, hb + 1) : niters, good);
}

// ---------------------------------------------------------------- host: one batch call
// vx_pnp_ransac_batch / vx_essential_ransac_batch (`fn`) from the argument checks to the scatter:
// the packed block offsets | intr | options | ptsA | ptsB (each part on a 16-byte boundary) staged
// in c->rs_host and uploaded into c->rs_in in one copy, `enqueue(d, hmax)` with the device pointers
// (D = PnpDeviceArgs / EmDeviceArgs: both list offsets, intr, opt, ptsA, ptsB, out, mask in this
// order; hmax = the largest max_iterations, at least 1), results | mask (c->rs_out) back in one
// copy, one synchronisation.  `check(p)` holds the option checks of problem p that differ between
// the two calls (it sets the error it returns), max_n / too_many their bound on offsets[P].
template <class D, class Opt, class Res, class Check, class Enqueue>
int batch_call(vx_ctx* c, const char* fn, int P, const int32_t* offsets, const double* intr4, const Opt* opt,
               const float* ptsA, int widthA, const float* ptsB, int widthB, int64_t max_n, const char* too_many,
               uint8_t* mask, Res* out, Check check, Enqueue enqueue) {
    if (!c || P < 0 || (P > 0 && (!offsets || !intr4 || !opt || !out)))
        return c ? set_error(c, VX_ERR_INVALID, "%s: bad arguments", fn) : VX_ERR_INVALID;
    if (P == 0) return VX_OK;
    if (P > 65535) return set_error(c, VX_ERR_INVALID, "at most 65535 problems per batch");
    if (offsets[0] != 0) return set_error(c, VX_ERR_INVALID, "offsets[0] must be 0");
    int hmax = 1;
    for (int p = 0; p < P; ++p) {
        if (offsets[p + 1] < offsets[p]) return set_error(c, VX_ERR_INVALID, "offsets must be non-decreasing");
        if (opt[p].max_iterations > kMaxHyp)
            return set_error(c, VX_ERR_INVALID, "max_iterations %d > %d", opt[p].max_iterations, kMaxHyp);
        if (int rc = check(p)) return rc;
        hmax = std::max(hmax, opt[p].max_iterations);
    }
    const int64_t N = offsets[P];
    if (N > 0 && (!ptsA || !ptsB)) return set_error(c, VX_ERR_INVALID, "%s: null points", fn);
    if (N > max_n) return set_error(c, VX_ERR_INVALID, "%s", too_many);
    VX_HIP(c, hipSetDevice(c->device));
    const size_t bytesA = (size_t)N * widthA * sizeof(float), bytesB = (size_t)N * widthB * sizeof(float);
    const size_t o_off = 0, o_intr = align16(o_off + (P + 1) * sizeof(int32_t)),
                 o_opt = align16(o_intr + (size_t)P * 4 * sizeof(double)),
                 o_a = align16(o_opt + (size_t)P * sizeof(Opt)), o_b = align16(o_a + bytesA),
                 in_bytes = align16(o_b + bytesB);
    VX_HIP(c, c->rs_host.ensure(in_bytes));
    uint8_t* hs = static_cast<uint8_t*>(c->rs_host.p);
    std::memcpy(hs + o_off, offsets, (P + 1) * sizeof(int32_t));
    std::memcpy(hs + o_intr, intr4, (size_t)P * 4 * sizeof(double));
    std::memcpy(hs + o_opt, opt, (size_t)P * sizeof(Opt));
    if (N) {
        std::memcpy(hs + o_a, ptsA, bytesA);
        std::memcpy(hs + o_b, ptsB, bytesB);
    }
    VX_HIP(c, c->rs_in.ensure(in_bytes));
    VX_HIP(c, hipMemcpyAsync(c->rs_in.p, hs, in_bytes, hipMemcpyHostToDevice, c->stream));
    const size_t o_mask = align16((size_t)P * sizeof(Res)), out_bytes = o_mask + (size_t)std::max<int64_t>(N, 1);
    VX_HIP(c, c->rs_out.ensure(out_bytes));
    const uint8_t* din = c->rs_in.as<uint8_t>();
    const D d{reinterpret_cast<const int*>(din + o_off), reinterpret_cast<const double*>(din + o_intr),
              reinterpret_cast<const Opt*>(din + o_opt),  reinterpret_cast<const float*>(din + o_a),
              reinterpret_cast<const float*>(din + o_b),  c->rs_out.as<Res>(),
              c->rs_out.as<uint8_t>() + o_mask};
    if (int rc = enqueue(d, hmax)) return rc;
    VX_HIP(c, c->rs_host_out.ensure(out_bytes));
    VX_HIP(c, hipMemcpyAsync(c->rs_host_out.p, c->rs_out.p, out_bytes, hipMemcpyDeviceToHost, c->stream));
    VX_HIP(c, hipStreamSynchronize(c->stream));
    const uint8_t* ho = static_cast<const uint8_t*>(c->rs_host_out.p);
    std::memcpy(out, ho, (size_t)P * sizeof(Res));
    if (mask && N) std::memcpy(mask, ho + o_mask, (size_t)N);
    return VX_OK;
}

}  // namespace rs
}  // namespace vx
