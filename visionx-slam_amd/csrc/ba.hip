// ba.hip — sliding-window bundle adjustment on gfx950 (LocalBA::Optimize drop-in).
//
// Replaces LocalBA::Optimize (core/backend/local_ba.cpp:66-249).  The reference alternates a
// per-keyframe 6x6 Gauss-Newton step with landmarks fixed (:116-174) and a per-landmark 3x3 step
// with poses fixed (:176-238), up to max_iterations times with a relative-cost stop (:240-247).
// Both stages are embarrassingly parallel, so the device problem is two CSR views of the window:
//
//   host   plan:  SelectKeyFrames (:42-62) + landmark filtering (:93-104) + the per-observation
//                 validity checks that are static during Optimize (:131-138, :186-204) ->
//                 keyframe-major pose observations (uv, landmark slot) and landmark-major
//                 observations (uv, keyframe row); uploaded once, replayed by every run.
//   device run (per iteration it; every kernel early-exits once the stop rule has fired):
//     k_pose_kf        n_split workgroups per keyframe, each over a slice of its observations
//                      (about one per thread): project (ProjectToPixel, projection.h:11-31), gate,
//                      weight, the 21 + 6 + 2 normal-equation terms of the 2x6 PoseJacobian in
//                      registers; a halving-butterfly wave reduction + LDS tree writes the slice's
//                      29-term partial block (fixed order: deterministic)
//     [sharded only]   ncclAllReduce(sum, f64) of the partial blocks over the landmark shards
//                      (one collective per iteration, 32 doubles per keyframe slice)
//     k_landmark_solve every workgroup sums the slice partials in slice order and solves ALL window
//                      keyframes redundantly (one lane per keyframe: H += 1e-6 I, Eigen-style
//                      pivoted LDLT, finite check, T <- exp(dx) T) into LDS — bitwise identical in
//                      every workgroup — while its landmark-stage loads are in flight; then one
//                      thread per landmark OBSERVATION forms its 9 terms (Jp * R), the thread owning
//                      each landmark sums them in CSR order and solves the 3x3 (p += dp).
//                      Workgroup 0 publishes the poses and evaluates the stop rule.
//                      Windows beyond kMaxKfLds keyframes use k_pose_solve_g + k_landmark instead.
// Iterations alternate two pose buffers (no launch reads what another workgroup of it writes);
// iteration 0 reads the initial poses / positions directly, so a run needs no reset launch.
// The step keeps the reference's sign (b = -J^T e, :156 and :224): this is a drop-in, not a fix.
//
// This file is the host side and one translation unit with the kernels, whose text lives in
// ba_kernels.hpp (the two-kernel path above), ba_fused_kernel.hpp (k_ba_iter: one launch per
// iteration) and ba_win_kernel.hpp (k_ba_win: one launch per run); the small reduction kernels
// (k_row_sum, k_peer_*, k_sum_parts) stay here beside their launches.  The records the kernels take
// (BAState, BAArgs) are declared in ba_plan.hpp.  Host side, top to bottom: make_args, the plan's
// buffers and pool, the fused layout (build_fused, fused_finish), build_plan, then the run —
// choose_kernels, the stage launches, reduce_rows and run_window, which is the ONLY statement of a
// run's order (reset, prologue, per iteration the row reduction and the iteration's kernels) for an
// unsharded plan, a real rank's shard and the one-device emulation of every shard alike — and the
// C entry points.
#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <chrono>
#include <cmath>
#include <type_traits>
#include <cstring>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "vx_internal.hpp"
#include "vx_ktrace.hpp"
#include "ba_common.hpp"
#include "ba_plan.hpp"
#include "dmap.hpp"

// the kernels, in this order
#include "ba_kernels.hpp"
#include "ba_fused_kernel.hpp"
#include "ba_win_kernel.hpp"

namespace vx {
namespace {

using namespace vx::ba;

// sharded plans: each keyframe row's partial slots summed in slot order (the slots of a row no group
// fills are 0) -> rowpart, which the per-iteration all-reduce then sums over the ranks
__global__ void k_row_sum(const double* part, int n_kf, int maxl, double* rowpart) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_kf * kStride) return;
    const int row = i / kStride, t = i - row * kStride;
    const double* src = part + (size_t)row * maxl * kStride + t;
    double s = 0.0;
    for (int q = 0; q < maxl; ++q) s += src[(size_t)q * kStride];
    rowpart[i] = s;
}

// ---- one-shot peer reduction of a sharded window's row sums ($VX_BA_PEER=1, opt-in)
// In place of the per-iteration ncclAllReduce (a ring of 2 (N - 1) dependent steps, latency-bound at
// 100 KB: DESIGN.md §6): every rank publishes its row sums into a block of its own device memory that
// every other rank has mapped (IPC over xGMI) and sets the block's flag to the iteration's
// generation; every rank waits for all N flags and sums the ranks' rows in rank order — the same
// values on every rank, and bitwise what the one-GPU emulation's k_sum_parts gives.  The rows are
// double-buffered by generation parity: a rank rewrites parity p at generation g + 2 only after its
// own wait for every flag >= g + 1, which each rank sets after it has read generation g.  Bounded
// waits: a flag that does not come sets the state's fault (vx_ba_plan_fetch reports VX_ERR_COMM).
constexpr int kMaxPeers = 16;
constexpr long long kPeerSpinTicks = 20'000'000;  // 200 ms of the 100 MHz wall clock
struct PeerPtrs {
    const double* rows[kMaxPeers];
    const unsigned long long* flag[kMaxPeers];
};
// this rank's row sums (k_row_sum's arithmetic: slots in slot order) -> its block (parity), then the flag
__global__ __launch_bounds__(1024) void k_peer_publish(const double* part, int n_kf, int maxl, double* out,
                                                      unsigned long long* flag, unsigned long long gen) {
    const int n = n_kf * kStride;
    for (int i = threadIdx.x; i < n; i += 1024) {
        const int row = i / kStride, t = i - row * kStride;
        const double* src = part + (size_t)row * maxl * kStride + t;
        double s = 0.0;
        for (int q = 0; q < maxl; ++q) s += src[(size_t)q * kStride];
        out[i] = s;
    }
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(flag, gen, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// every rank's flag >= gen, then the ranks' rows (parity offset off) summed in rank order -> out
__global__ __launch_bounds__(1024) void k_peer_gather(PeerPtrs pp, int n_ranks, int len, int off, unsigned long long gen,
                                                     double* out, int* fault) {
    __shared__ int s_bad;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    if (threadIdx.x < n_ranks) {
        const long long t0 = wall_clock64();
        while (__hip_atomic_load(pp.flag[threadIdx.x], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < gen) {
            if (wall_clock64() - t0 > kPeerSpinTicks) {
                s_bad = 1;
                break;
            }
            __builtin_amdgcn_s_sleep(2);
        }
    }
    __syncthreads();
    if (s_bad) {
        if (threadIdx.x == 0) __hip_atomic_store(fault, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    __threadfence_system();
    for (int i = threadIdx.x; i < len; i += 1024) {
        double s = __hip_atomic_load(pp.rows[0] + off + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        for (int r = 1; r < n_ranks; ++r) s += __hip_atomic_load(pp.rows[r] + off + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        out[i] = s;
    }
}

// fused-order observation payloads: uv by plan index (-1: padding), pose records with the fixed
// landmarks' positions
__global__ void k_fused_gather(const int* lsrc, int nl, const double2* luv, double2* out_luv, const int* psrc,
                               const int* pcode, int np, const double2* puv, const double* lm_pos0, double2* out_puv,
                               double4* out_pp) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nl) out_luv[i] = lsrc[i] >= 0 ? luv[lsrc[i]] : make_double2(1e300, 1e300);
    if (i < np) {
        const int sidx = psrc[i], c = pcode[i];
        out_puv[i] = sidx >= 0 ? puv[sidx] : make_double2(0.0, 0.0);
        double4 P = make_double4(0.0, 0.0, 0.0, (double)c);
        if (c < 0) {
            const double* q = lm_pos0 + 4 * (size_t)(-1 - c);
            P.x = q[0];
            P.y = q[1];
            P.z = q[2];
        }
        out_pp[i] = P;
    }
}


}  // namespace
}  // namespace vx


namespace vx {
namespace {

BAArgs make_args(vx_ba_plan* p) {
    BAArgs a{};
    a.n_kf = p->n_kf;
    a.n_opt = p->n_opt;
    a.n_lm = p->n_lm;
    ba_set_options(a, p->opt);
    a.kf_pose0 = p->kf_pose0.as<double>();
    a.kf_pose = p->kf_pose.as<double>();
    a.kf_intr = p->kf_intr.as<double>();
    a.kf_rot = p->kf_rot.as<double>();
    a.kf_flags = p->kf_flags.as<int>();
    a.kf_obs_ptr = p->kf_obs_ptr.as<int>();
    a.kf_part = p->kf_part.as<double>();
    a.n_split = p->n_split;
    a.kf_cost = p->kf_cost.as<double>();
    a.lm_pos0 = p->lm_pos0.as<double>();
    a.lm_pos = p->lm_pos.as<double>();
    a.pobs_uv = p->pobs_uv.as<double2>();
    a.pobs_lm = p->pobs_lm.as<int>();
    a.lobs_ptr = p->lobs_ptr.as<int>();
    a.lobs_kf = p->lobs_kf.as<int>();
    a.lobs_lm = p->lobs_lm.as<int>();
    a.lm_blk = p->lm_blk.as<int>();
    a.lobs_uv = p->lobs_uv.as<double2>();
    a.state = p->state.as<BAState>();
    return a;
}

template <class T>
int upload(vx_ctx* c, DevBuf& d, const std::vector<T>& h) {
    VX_HIP(c, d.ensure(std::max<size_t>(1, h.size()) * sizeof(T)));
    if (!h.empty()) VX_HIP(c, hipMemcpy(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return VX_OK;
}

}  // namespace

// k_landmark_solve workgroups: whole landmarks, at most kLmBlock landmarks and observations each
// (a window of <= kMaxKfLds keyframes gives a landmark <= kMaxKfLds < kLmBlock of them)
// Returned as {first landmark, its first observation} per workgroup (n_blocks + 1 pairs), so a
// workgroup reads both in one load instead of a dependent lobs_ptr load after lm_blk.
// A landmark with more than kLmBlock observations (possible only if a snapshot lists one keyframe
// twice for it) gets a workgroup of its own and *max_cnt reports it: plan_run then takes the
// one-thread-per-landmark kernels, which have no such limit.
std::vector<int> pack_lm_blocks(const std::vector<int>& lptr, int n_opt, int* max_cnt) {
    std::vector<int> blk{0, lptr[0]};
    int n_o = 0, n_l = 0, mx = 0;
    for (int s = 0; s < n_opt; ++s) {
        const int cnt = lptr[s + 1] - lptr[s];
        mx = std::max(mx, cnt);
        if (n_l + 1 > kLmBlock || n_o + cnt > kLmBlock) {
            blk.push_back(s);
            blk.push_back(lptr[s]);
            n_o = n_l = 0;
        }
        n_o += cnt;
        ++n_l;
    }
    blk.push_back(n_opt);
    blk.push_back(lptr[n_opt]);
    if (max_cnt) *max_cnt = mx;
    return blk;
}

// Work buffers of a run (both plan builders end here): ping-pong poses, rotations, pose-stage
// partial blocks, costs, landmark positions and the iteration state.
namespace {
// a finished run's window poses (ping-pong buffer of the last iteration) and optimised landmark
// positions into the resident map's rows
__global__ void k_apply_dmap(const BAState* st, const double* kf_pose, int n_kf, const double* lm_pos, int n_opt,
                             const int* kf_map, const int* lm_map, double* map_pose, double* map_pos) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_kf) {
        const double* src = kf_pose + (size_t)(st->iterations & 1) * n_kf * 8 + (size_t)8 * i;
        for (int j = 0; j < 7; ++j) map_pose[(size_t)7 * kf_map[i] + j] = src[j];
    }
    if (i < n_opt)
        for (int j = 0; j < 3; ++j) map_pos[(size_t)3 * lm_map[i] + j] = lm_pos[(size_t)4 * i + j];
}
}  // namespace

int alloc_run_buffers(vx_ctx* c, vx_ba_plan* p) {
    const size_t nk = (size_t)p->n_kf;
    VX_HIP(c, p->kf_pose.ensure(nk * 2 * 8 * sizeof(double)));
    VX_HIP(c, p->kf_rot.ensure(nk * 9 * sizeof(double)));
    VX_HIP(c, p->kf_part.ensure(nk * p->n_split * kStride * sizeof(double)));
    VX_HIP(c, p->kf_cost.ensure(nk * 2 * sizeof(double)));
    VX_HIP(c, p->lm_pos.ensure((size_t)std::max(p->n_lm, 1) * 4 * sizeof(double)));
    VX_HIP(c, p->state.ensure(sizeof(BAState)));
    // (the fault word is read by every fetch; a recycled state block may hold anything)
    VX_HIP(c, hipMemsetAsync(p->state.p, 0, sizeof(BAState), c->stream));
    return VX_OK;
}

namespace {
template <class B>
void swap_buf(B& a, B& b) {
    std::swap(a.p, b.p);
    std::swap(a.bytes, b.bytes);
}
// dst takes src's buffers (and src dst's); nothing else of either plan moves
void adopt_buffers(vx_ba_plan* dst, vx_ba_plan* src) {
#define VX_SWAP_BUF(b) swap_buf(dst->b, src->b);
    VX_PLAN_BUFFERS(VX_SWAP_BUF)
#undef VX_SWAP_BUF
}
constexpr size_t kMaxPlanHusks = 4;  // parked buffer sets per context
}  // namespace

vx_ba_plan* plan_new(vx_ctx* c) {
    auto* p = new vx_ba_plan();
    p->c = c;
    if (!c) return p;
    if (!c->plan_husks.empty()) {
        vx_ba_plan* h = c->plan_husks.back();
        c->plan_husks.pop_back();
        adopt_buffers(p, h);
        delete h;
    }
    c->plan_live.push_back(p);
    return p;
}

// Test hook: $VX_TEST_FAIL_PLAN=1 makes every plan build fail after the plan was registered with
// its context (tests/test_gpu_parity.py::test_failed_plan_build_then_destroy).
int plan_fault_injected(vx_ctx* c) {
    const char* e = getenv("VX_TEST_FAIL_PLAN");
    return (e && e[0] == '1') ? set_error(c, VX_ERR_STATE, "plan build failed ($VX_TEST_FAIL_PLAN)") : VX_OK;
}

void plan_pool_release(vx_ctx* c) {
    for (vx_ba_plan* h : c->plan_husks) delete h;
    c->plan_husks.clear();
    for (vx_ba_plan* p : c->plan_live) p->c = nullptr;  // their destroy then just frees
    c->plan_live.clear();
}

bool fused_eligible(const vx_ba_plan* p) {
    if (p->status != 0 || p->global_poses || p->n_kf > kMaxKfLds || p->n_opt <= 0) return false;
    // a keyframe with one or two observations may step: its pose system needs the LDL^T branch that
    // only k_landmark_solve / k_pose_solve_g carry (solve_pose<true>)
    if (p->opt.min_pose_observations < 3) return false;
    if (const char* e = getenv("VX_BA_FUSED"))
        if (e[0] == '0') return false;
    return true;
}

// $VX_BA_PERSIST=0: the fused LocalBA as one launch per iteration (k_ba_iter) instead of the
// persistent window (k_ba_win; read at plan build)
bool ba_persist() {
    const char* e = getenv("VX_BA_PERSIST");
    return !(e && e[0] == '0');
}

// $VX_BA_ATOMIC_ROWS=0: the fused LocalBA's per-keyframe partial slots (every run bitwise the
// same) instead of row sums by float atomics (FusedArgs::arow; read at plan build)
bool ba_atomic_rows() {
    const char* e = getenv("VX_BA_ATOMIC_ROWS");
    return !(e && e[0] == '0');
}

// 1024 threads when 512-thread workgroups would outnumber the compute units (their count is within a
// few percent of the landmark-stage observations / 512: whole landmarks of <= 5 observations);
// VX_BA_FUSED_THREADS / VX_BA_FUSED_CAP override for sweeps
int fused_threads(vx_ctx* c, int64_t n_lobs, int* cap) {
    if (!c->n_cus) c->n_cus = std::max(vx_device_cus(c->device), 1);
    int ft = n_lobs > (int64_t)c->n_cus * (kFTSmall - 16) ? kFTLarge : kFTSmall;
    if (const char* e = getenv("VX_BA_FUSED_THREADS")) {
        const int v = atoi(e);
        ft = v == kFTLarge ? kFTLarge : v == kFTNarrow ? kFTNarrow : kFTSmall;
    }
    *cap = ft;
    if (const char* e = getenv("VX_BA_FUSED_CAP")) *cap = std::min(ft, std::max(64, atoi(e)));
    return ft;
}

size_t fused_offsets(int nb, int ft, size_t n_pp, FusedOffsets& F) {
    const size_t n_lp = (size_t)nb * ft;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t o = at;
        at += (bytes + 255) & ~(size_t)255;
        return o;
    };
    F.blk = take((size_t)nb * fused_blk_ints(ft) * 4);
    F.lm_slot = take(n_lp * 4);
    F.lm_run = take(n_lp * 8);
    F.lobs_rec = take(n_lp * 16);
    F.kent = take((size_t)nb * kFK * 32);
    F.lobs_src = take(n_lp * 4);
    F.pobs_src = take(std::max<size_t>(n_pp, 1) * 4);
    F.pobs_code = take(std::max<size_t>(n_pp, 1) * 4);
    return at;
}

int fused_finish(vx_ctx* c, vx_ba_plan* p, int nb, int ft, int maxl, size_t n_pp, int stop_b) {
    const FusedOffsets& F = p->f_off;
    const size_t n_lp = (size_t)nb * ft;
    const uint8_t* T = p->f_tab.as<uint8_t>();
    VX_HIP(c, p->f_lobs_uv.ensure(n_lp * sizeof(double2)));
    VX_HIP(c, p->f_pobs_uv.ensure(std::max<size_t>(n_pp, 1) * sizeof(double2)));
    VX_HIP(c, p->f_pobs_p.ensure(std::max<size_t>(n_pp, 1) * sizeof(double4)));
    hipLaunchKernelGGL(k_fused_gather, dim3((unsigned)((std::max(n_lp, n_pp) + 255) / 256)), dim3(256), 0, c->stream,
                       reinterpret_cast<const int*>(T + F.lobs_src), (int)n_lp, (const double2*)p->lobs_uv.as<double2>(),
                       p->f_lobs_uv.as<double2>(), reinterpret_cast<const int*>(T + F.pobs_src),
                       reinterpret_cast<const int*>(T + F.pobs_code), (int)n_pp, (const double2*)p->pobs_uv.as<double2>(),
                       (const double*)p->lm_pos0.as<double>(), p->f_pobs_uv.as<double2>(), p->f_pobs_p.as<double4>());
    VX_LAUNCH_CHECK(c, "k_fused_gather");
    VX_HIP(c, p->f_lpos.ensure(n_lp * sizeof(double4)));
    VX_HIP(c, p->f_epose.ensure((size_t)nb * kFK * 16 * sizeof(double)));
    const size_t part_bytes = 2 * (size_t)p->n_kf * maxl * kStride * sizeof(double);
    VX_HIP(c, p->f_part.ensure(part_bytes));
    if (p->shard_count > 1) VX_HIP(c, p->f_rowpart.ensure((size_t)p->n_kf * kStride * sizeof(double)));
    VX_HIP(c, hipMemsetAsync(p->f_part.p, 0, part_bytes, c->stream));  // slots no group writes stay 0
    const size_t cost_bytes = 2 * (size_t)p->n_kf * maxl * sizeof(double2);
    VX_HIP(c, p->f_costpart.ensure(cost_bytes));
    VX_HIP(c, hipMemsetAsync(p->f_costpart.p, 0, cost_bytes, c->stream));
    // row sums by float atomics (FusedArgs::arow): unsharded plans, unless $VX_BA_ATOMIC_ROWS=0
    // (partial slots: every run bitwise the same)
    p->f_atomic = p->shard_count <= 1 && ft <= kFTSmall && ba_atomic_rows();
    if (p->f_atomic) {
        const size_t ab = 4 * (size_t)p->n_kf * kStride * sizeof(double);
        VX_HIP(c, p->f_arow.ensure(ab));
        VX_HIP(c, hipMemsetAsync(p->f_arow.p, 0, ab, c->stream));
    }
    // persistent window (k_ba_win): unsharded atomic-row plans of 512-thread workgroups that are all
    // resident at once (one per CU); $VX_BA_PERSIST=0 keeps the per-iteration launches
    p->f_persist = false;
    p->win_off = false;
    if (!c->n_cus) c->n_cus = std::max(vx_device_cus(c->device), 1);
    if (p->f_atomic && ft == kFTSmall && nb <= c->n_cus && p->opt.max_iterations >= 1 &&
        p->opt.max_iterations <= kMaxIter && ba_persist()) {
        const size_t M = (size_t)p->opt.max_iterations, nk = (size_t)p->n_kf;
        size_t at = 0;
        auto take = [&](size_t bytes) {
            const size_t o = at;
            at += (bytes + 255) & ~(size_t)255;
            return o;
        };
        // per iteration every partial slot of every row plus one slot that nobody fills (what
        // $VX_BA_WIN_TEST_FAULT makes row 0 wait for: the test of the fault path,
        // tests/test_gpu_parity.py); zeroed once here (tag 0 is no run's), never between runs
        p->win_part_off = take(M * (nk * (size_t)maxl + 1) * kStride * 2 * sizeof(wgran));
        p->win_stop_off = take(M * nk * 4 * sizeof(wgran));
        p->win_hello_off = take((size_t)nb * sizeof(unsigned));
        p->win_gen_off = take(sizeof(int));
        p->win_bias = getenv("VX_BA_WIN_TEST_FAULT") ? 1 : 0;
        VX_HIP(c, p->f_win.ensure(at));
        VX_HIP(c, hipMemsetAsync(p->f_win.p, 0, at, c->stream));
        p->f_persist = true;
    }
    p->f_stop_b = stop_b;
    p->f_blocks = nb;
    p->f_maxl = maxl;
    p->f_threads = ft;
    p->f_npp = n_pp;
    p->fused = true;
    return VX_OK;
}

// The fused layout (k_ba_iter) from the plan's CSRs, on the host: both plan builders end here with
// the same arrays, so the layout — and every run — is the same for both.
//   1. optimised landmarks ordered by the first window keyframe that observes them (stable), so a
//      workgroup's landmarks share few keyframes;
//   2. greedy workgroups: at most ft landmarks, ft landmark-stage observations and kFK
//      keyframes (those of its landmark-stage and pose-stage observations);
//   3. each window keyframe owned by the first workgroup that touches it (untouched ones by
//      workgroup 0): the owner publishes its pose and takes the pose observations of fixed
//      landmarks in it;
//   4. a workgroup's pose observations grouped by keyframe (ascending observation index inside,
//      i.e. the plan's keyframe-major order), one partial slot per non-empty (workgroup, keyframe)
//      group, numbered per keyframe in workgroup order.
int build_fused(vx_ctx* c, vx_ba_plan* p, const std::vector<int>& kptr, const std::vector<int>& plm,
                const std::vector<int>& lptr, const std::vector<int>& lkf) {
    p->fused = false;
    if (!fused_eligible(p)) return VX_OK;
    const int nk = p->n_kf, n_opt = p->n_opt, n_pose = kptr[nk];
    // $VX_PLAN_TIMING=1: phase times of this build on stderr (scripts/plan_build_time.py)
    static const bool timing = getenv("VX_PLAN_TIMING") != nullptr;
    using clk = std::chrono::steady_clock;
    const auto t_start = clk::now();
    double t_ph[16] = {0};
    auto lap = [&](int i) { t_ph[i] = std::chrono::duration<double, std::milli>(clk::now() - t_start).count(); };
    std::vector<int> pkf(n_pose);
    for (int k = 0; k < nk; ++k)
        for (int o = kptr[k]; o < kptr[k + 1]; ++o) pkf[o] = k;
    // pose observations per optimised slot (ascending)
    std::vector<int> pp(n_opt + 1, 0), pidx;
    for (int o = 0; o < n_pose; ++o)
        if (plm[o] < n_opt) ++pp[plm[o] + 1];
    for (int q = 0; q < n_opt; ++q) pp[q + 1] += pp[q];
    pidx.resize(pp[n_opt]);
    {
        std::vector<int> w(pp.begin(), pp.end() - 1);
        for (int o = 0; o < n_pose; ++o)
            if (plm[o] < n_opt) pidx[w[plm[o]]++] = o;
    }
    lap(3);
    // 1. keyframe-locality order (counting sort by first keyframe, stable)
    std::vector<int> key(n_opt, nk), order(n_opt);
    for (int q = 0; q < n_opt; ++q) {
        int k0 = nk;
        for (int o = lptr[q]; o < lptr[q + 1]; ++o) k0 = std::min(k0, lkf[o]);
        for (int i = pp[q]; i < pp[q + 1]; ++i) k0 = std::min(k0, pkf[pidx[i]]);
        key[q] = k0;
    }
    {
        std::vector<int> kc(nk + 2, 0);
        for (int q = 0; q < n_opt; ++q) ++kc[key[q] + 1];
        for (int k = 0; k <= nk; ++k) kc[k + 1] += kc[k];
        for (int q = 0; q < n_opt; ++q) order[kc[key[q]]++] = q;
    }
    lap(4);
    // each optimised landmark's distinct keyframes (landmark-stage and pose-stage observations)
    std::vector<int> uk_ptr(n_opt + 1, 0), uk;
    uk.reserve((size_t)lptr[n_opt] + pidx.size());
    {
        std::vector<int> seen(nk, -1);
        for (int q = 0; q < n_opt; ++q) {
            for (int o = lptr[q]; o < lptr[q + 1]; ++o)
                if (seen[lkf[o]] != q) {
                    seen[lkf[o]] = q;
                    uk.push_back(lkf[o]);
                }
            for (int i = pp[q]; i < pp[q + 1]; ++i)
                if (seen[pkf[pidx[i]]] != q) {
                    seen[pkf[pidx[i]]] = q;
                    uk.push_back(pkf[pidx[i]]);
                }
            uk_ptr[q + 1] = (int)uk.size();
        }
    }
    lap(5);
    // 2. greedy workgroups of ft threads (cap: landmark-stage observations and landmarks per
    // workgroup; VX_BA_FUSED_THREADS / VX_BA_FUSED_CAP override for sweeps).  1024
    // threads when 512-thread workgroups would outnumber the compute units (their count is within a
    // few percent of the landmark-stage observations / 512: whole landmarks of <= 5 observations)
    int cap = 0;
    const int ft = fused_threads(c, lptr[n_opt], &cap);
    std::vector<std::vector<int>> K(1), LM(1);
    std::vector<int> stamp(nk, -1);
    int n_l = 0, n_o = 0;
    for (int idx = 0; idx < n_opt; ++idx) {
        const int q = order[idx], cnt = lptr[q + 1] - lptr[q];
        if (cnt > ft) return VX_OK;
        int cur = (int)K.size() - 1;
        int nn = 0;
        for (int u = uk_ptr[q]; u < uk_ptr[q + 1]; ++u) nn += stamp[uk[u]] != cur;
        if (n_l > 0 && (n_l + 1 > cap || n_o + cnt > cap || (int)K[cur].size() + nn > kFK)) {
            K.emplace_back();
            LM.emplace_back();
            ++cur;
            n_l = n_o = 0;
            nn = uk_ptr[q + 1] - uk_ptr[q];
        }
        if (nn > kFK) return VX_OK;
        for (int u = uk_ptr[q]; u < uk_ptr[q + 1]; ++u)
            if (stamp[uk[u]] != cur) {
                stamp[uk[u]] = cur;
                K[cur].push_back(uk[u]);
            }
        LM[cur].push_back(q);
        ++n_l;
        n_o += cnt;
    }
    const int nb = (int)K.size();
    // the device build's workgroup limit (k_fb_pose_rank's LDS counters, ba_fused_build.hip): beyond
    // it both builds give the plan no fused layout, so host- and device-built plans stay identical
    if (nb > kFusedMaxGroups) return VX_OK;
    const int fw = ft / 64;
    lap(0);
    // 3. owners
    std::vector<int> owner(nk, -1);
    for (int b = 0; b < nb; ++b)
        for (int k : K[b])
            if (owner[k] < 0) owner[k] = b;
    for (int k = 0; k < nk; ++k)
        if (owner[k] < 0) {
            owner[k] = 0;
            K[0].push_back(k);
        }
    if ((int)K[0].size() > kFK) return VX_OK;
    for (auto& v : K) std::sort(v.begin(), v.end());
    lap(6);
    // 4. pose observations per workgroup (ascending observation index = keyframe-major)
    std::vector<int> lm_blk(n_opt), lm_loc(n_opt);
    for (int b = 0; b < nb; ++b)
        for (int i = 0; i < (int)LM[b].size(); ++i) {
            lm_blk[LM[b][i]] = b;
            lm_loc[LM[b][i]] = i;
        }
    // (CSR by workgroup, ascending observation index inside)
    std::vector<int> po_ptr(nb + 1, 0), po(n_pose), po_blk(n_pose);
    for (int o = 0; o < n_pose; ++o) {
        po_blk[o] = plm[o] < n_opt ? lm_blk[plm[o]] : owner[pkf[o]];
        ++po_ptr[po_blk[o] + 1];
    }
    for (int b = 0; b < nb; ++b) po_ptr[b + 1] += po_ptr[b];
    {
        std::vector<int> w(po_ptr.begin(), po_ptr.end() - 1);
        for (int o = 0; o < n_pose; ++o) po[w[po_blk[o]]++] = o;
    }
    // tables: landmarks / landmark-stage observations at b * ft, keyframe entries at b * kFK,
    // pose observations wave-major with 64-aligned entries.  Written straight into one pinned
    // staging block and uploaded with one copy (the build is paid per LocalBA::Optimize call).
    const int kBlkInts = fused_blk_ints(ft);
    lap(7);
    // pass 1: each entry's pose observations, the waves' rounds
    std::vector<int> ent_beg((size_t)nb * kFK, 0), ent_end((size_t)nb * kFK, 0);
    size_t n_pp = 0;
    for (int b = 0; b < nb; ++b) {
        int i = po_ptr[b];
        for (int j = 0; j < (int)K[b].size(); ++j) {
            ent_beg[(size_t)b * kFK + j] = i;
            while (i < po_ptr[b + 1] && pkf[po[i]] == K[b][j]) ++i;
            ent_end[(size_t)b * kFK + j] = i;
            n_pp += (size_t)(i - ent_beg[(size_t)b * kFK + j] + 63) / 64 * 64;
        }
        if (i != po_ptr[b + 1]) return set_error(c, VX_ERR_STATE, "fused layout: pose observations out of keyframe order");
    }
    // entry positions: SIMD-aware LPT over the entries' pose-stage rounds (fused_place_entries)
    std::vector<int> epos((size_t)nb * kFK, -1), n_pos(nb, 0);
    for (int b = 0; b < nb; ++b) {
        int rounds[kFK];
        const int ne = (int)K[b].size();
        for (int j = 0; j < ne; ++j)
            rounds[j] = (ent_end[(size_t)b * kFK + j] - ent_beg[(size_t)b * kFK + j] + 63) / 64;
        n_pos[b] = fused_place_entries(rounds, ne, &epos[(size_t)b * kFK]);
    }
    FusedOffsets& F = p->f_off;
    const size_t at = fused_offsets(nb, ft, n_pp, F);
    lap(8);
    VX_HIP(c, p->f_stage.ensure(at, true));
    lap(9);
    uint8_t* S = static_cast<uint8_t*>(p->f_stage.p);
    int* blk = reinterpret_cast<int*>(S + F.blk);
    int* lm_slot = reinterpret_cast<int*>(S + F.lm_slot);
    int2* lm_run = reinterpret_cast<int2*>(S + F.lm_run);
    int4* lobs_rec = reinterpret_cast<int4*>(S + F.lobs_rec);
    int* kent = reinterpret_cast<int*>(S + F.kent);
    int* lobs_src = reinterpret_cast<int*>(S + F.lobs_src);
    int* pobs_src = reinterpret_cast<int*>(S + F.pobs_src);
    int* pobs_code = reinterpret_cast<int*>(S + F.pobs_code);
    std::memset(blk, 0, (size_t)nb * kBlkInts * 4);
    std::vector<int> loc(nk, -1), rank(nk, 0), ent_rank((size_t)nb * kFK, -1), at_pos(kFK);
    size_t pw = 0;
    long long stop_key = -1;
    for (int b = 0; b < nb; ++b) {
        int max_rounds = 0;
        const int* EP = &epos[(size_t)b * kFK];
        for (int j = 0; j < (int)K[b].size(); ++j) loc[K[b][j]] = EP[j];
        std::fill(at_pos.begin(), at_pos.end(), -1);
        for (int j = 0; j < (int)K[b].size(); ++j) at_pos[EP[j]] = j;
        int* B = blk + (size_t)b * kBlkInts;
        const size_t base = (size_t)b * ft;
        int ob = 0;
        for (int t = 0; t < (int)LM[b].size(); ++t) {
            const int q = LM[b][t];
            lm_slot[base + t] = q;
            lm_run[base + t].x = ob;
            for (int o = lptr[q]; o < lptr[q + 1]; ++o, ++ob) {
                lobs_src[base + ob] = o;
                lobs_rec[base + ob] = make_int4(loc[lkf[o]], t, q, 0);
            }
            lm_run[base + t].y = ob;
        }
        // padding rows (valid loads: slot 0, empty runs, no observation)
        for (int t = (int)LM[b].size(); t < ft; ++t) {
            lm_slot[base + t] = 0;
            lm_run[base + t] = make_int2(0, 0);
        }
        for (int t = ob; t < ft; ++t) {
            lobs_src[base + t] = -1;
            lobs_rec[base + t] = make_int4(0, 0, 0, 0);
        }
        B[0] = (int)LM[b].size();
        B[1] = ob;
        B[2] = n_pos[b];  // (positions: entries and holes)
        int* E = kent + (size_t)b * kFK * 8;
        for (int j = 0; j < kFK; ++j)
            for (int x = 0; x < 8; ++x) E[8 * j + x] = (x == 0 || x == 4) ? -1 : 0;
        for (int w = 0; w < fw; ++w) {
            const size_t wstart = pw;
            for (int P = w; P < n_pos[b]; P += fw) {
                const int j = at_pos[P];
                if (j < 0) continue;  // a hole
                const int k = K[b][j];
                const int e0 = ent_beg[(size_t)b * kFK + j], e1 = ent_end[(size_t)b * kFK + j], n = e1 - e0;
                E[8 * P] = k | (owner[k] == b ? (1 << 30) : 0);
                E[8 * P + 2] = (int)pw;
                E[8 * P + 3] = (int)pw + n;
                for (int x = e0; x < e1; ++x) {
                    const int o = po[x];
                    pobs_src[pw + (x - e0)] = o;
                    pobs_code[pw + (x - e0)] = plm[o] < n_opt ? lm_loc[plm[o]] : -1 - plm[o];
                }
                const size_t padded = (size_t)(n + 63) / 64 * 64;  // pad to the next round
                for (size_t x = n; x < padded; ++x) {
                    pobs_src[pw + x] = -1;
                    pobs_code[pw + x] = 0;
                }
                pw += padded;
                if (n > 0) ent_rank[(size_t)b * kFK + j] = rank[k]++;
            }
            B[4 + 2 * w] = (int)wstart;
            B[4 + 2 * w + 1] = (int)((pw - wstart) / 64);
            max_rounds = std::max(max_rounds, B[4 + 2 * w + 1]);
        }
        const long long key = fused_stop_key(max_rounds, n_pos[b], b);
        if (stop_key < 0 || key < stop_key) stop_key = key;
        for (int k : K[b]) loc[k] = -1;
    }
    lap(10);
    int maxl = 1;
    for (int k = 0; k < nk; ++k) maxl = std::max(maxl, rank[k]);
    for (int b = 0; b < nb; ++b)
        for (int j = 0; j < (int)K[b].size(); ++j) {
            int* E = kent + ((size_t)b * kFK + epos[(size_t)b * kFK + j]) * 8;
            const int k = K[b][j];
            E[1] = rank[k];
            const int r = ent_rank[(size_t)b * kFK + j];
            E[4] = r >= 0 ? k * maxl + r : -1;
        }
    lap(1);
    // one upload, then the observation payloads gathered into the fused order
    VX_HIP(c, p->f_tab.ensure(at));
    VX_HIP(c, hipMemcpyAsync(p->f_tab.p, S, at, hipMemcpyHostToDevice, c->stream));
    int rc;
    if ((rc = fused_finish(c, p, nb, ft, maxl, n_pp, (int)(stop_key & 0xffffffff)))) return rc;
    VX_HIP(c, hipStreamSynchronize(c->stream));  // (the staging block is reused by the next build)
    lap(2);
    if (timing)
    {
        fprintf(stderr, "[vx plan] fused layout: pack %.3f ms, tables %.3f ms, upload + gather %.3f ms (%d workgroups x %d)\n",
                t_ph[0], t_ph[1] - t_ph[0], t_ph[2] - t_ph[1], nb, ft);
        fprintf(stderr, "[vx plan]   laps: pp %.3f order %.3f uk %.3f greedy %.3f owners %.3f po %.3f pass1 %.3f pinned %.3f tables %.3f ranks %.3f\n",
                t_ph[3], t_ph[4] - t_ph[3], t_ph[5] - t_ph[4], t_ph[0] - t_ph[5], t_ph[6] - t_ph[0], t_ph[7] - t_ph[6],
                t_ph[8] - t_ph[7], t_ph[9] - t_ph[8], t_ph[10] - t_ph[9], t_ph[1] - t_ph[10]);
    }
    return VX_OK;
}

namespace {

int build_plan(vx_ctx* c, const vx_map_view* m, uint64_t ref_kf_id, int has_ref, vx_ba_plan* p,
               bool device = true) {
    const vx_ba_options& o = p->opt;
    p->status = 1;
    if (!m || m->n_kf <= 0) return VX_OK;
    // ---- SelectKeyFrames (local_ba.cpp:42-62) + landmark set (local_ba.cpp:83-108)
    Window W;
    select_window(m, ref_kf_id, has_ref, o.window_size, o.min_point_observations, W);
    const std::vector<int>& win = W.win;
    const auto& win_row = W.win_row;
    const auto& lm_by_id = W.lm_by_id;
    const std::vector<int>& opt_all = W.opt_all;
    p->n_window_kf = (int)win.size();
    p->n_landmarks_global = (int)opt_all.size();
    if (W.status != 0) return VX_OK;
    p->status = 0;

    auto owned = [&](int l) {
        return p->shard_count <= 1 ||
               (int)(splitmix64(m->lm_id[l]) % (uint64_t)p->shard_count) == p->shard_rank;
    };
    // local landmark slots: owned optimisable first, then owned fixed ones met in the pose stage
    std::vector<int> slot_of(m->n_lm, -1);
    p->lm_map_idx.clear();
    for (int l : opt_all)
        if (owned(l)) {
            slot_of[l] = (int)p->lm_map_idx.size();
            p->lm_map_idx.push_back(l);
        }
    p->n_opt = (int)p->lm_map_idx.size();

    // ---- keyframe table + pose-stage CSR (local_ba.cpp:116-161)
    const int nk = (int)win.size();
    p->n_kf = nk;
    p->kf_map_idx = win;
    std::vector<double> pose0((size_t)nk * 8, 0.0), intr((size_t)nk * 4, 0.0);
    std::vector<double2> puv;
    std::vector<int> plm, kf_obs_ptr(nk + 1, 0), kf_flags(nk, 0);
    for (int r = 0; r < nk; ++r) {
        const int k = win[r];
        for (int j = 0; j < 7; ++j) pose0[8 * r + j] = m->kf_pose[7 * k + j];
        for (int j = 0; j < 4; ++j) intr[4 * r + j] = m->kf_intr[4 * k + j];
        kf_flags[r] = m->kf_has_cam[k] ? 1 : 0;
        kf_obs_ptr[r] = (int)puv.size();
        if (!m->kf_has_cam[k]) continue;
        for (int64_t f = m->kf_feat_ptr[k]; f < m->kf_feat_ptr[k + 1]; ++f) {
            const uint8_t fl = m->feat_flags[f];
            if (!(fl & 1) || (fl & 2)) continue;
            const int l_found = lm_by_id.get(m->feat_lm_id[f]);
            if (l_found < 0) continue;
            const int l = l_found;
            if (m->lm_bad[l] || !owned(l)) continue;
            if (slot_of[l] < 0) {
                slot_of[l] = (int)p->lm_map_idx.size();
                p->lm_map_idx.push_back(l);
            }
            puv.push_back(make_double2(m->feat_uv[2 * f], m->feat_uv[2 * f + 1]));
            plm.push_back(slot_of[l]);
        }
    }
    kf_obs_ptr[nk] = (int)puv.size();
    // workgroups per keyframe: about one observation per thread, from counts every shard sees
    // alike (the window's landmark features before sharding), so the all-reduced partial layout
    // is the same on every rank
    {
        int64_t mx = 0;
        for (int k : win)
            if (m->kf_has_cam[k]) {
                int64_t n = 0;
                for (int64_t f = m->kf_feat_ptr[k]; f < m->kf_feat_ptr[k + 1]; ++f) n += m->feat_flags[f] & 1;
                mx = std::max(mx, n);
            }
        p->n_split = ba_split(mx, p->shard_count);
    }
    p->n_lm = (int)p->lm_map_idx.size();
    p->n_pose_obs = (int64_t)puv.size();
    std::vector<double> lm0((size_t)std::max(p->n_lm, 1) * 4, 0.0);
    for (int s = 0; s < p->n_lm; ++s)
        for (int j = 0; j < 3; ++j) lm0[4 * s + j] = m->lm_pos[3 * p->lm_map_idx[s] + j];

    // ---- landmark-stage CSR (local_ba.cpp:186-204)
    std::vector<int> lptr(p->n_opt + 1, 0), lkf, llm;
    std::vector<double2> luv;
    for (int s = 0; s < p->n_opt; ++s) {
        const int l = p->lm_map_idx[s];
        for (int64_t ob = m->lm_obs_ptr[l]; ob < m->lm_obs_ptr[l + 1]; ++ob) {
            auto it = win_row.find(m->obs_kf_id[ob]);
            if (it == win_row.end()) continue;
            const int r = it->second;
            const int k = win[r];
            if (!m->kf_has_cam[k]) continue;
            const uint64_t fi = m->obs_feat_idx[ob];
            const int64_t nf = m->kf_feat_ptr[k + 1] - m->kf_feat_ptr[k];
            if (fi >= (uint64_t)nf) continue;
            const int64_t f = m->kf_feat_ptr[k] + (int64_t)fi;
            const uint8_t fl = m->feat_flags[f];
            if (!(fl & 1) || (fl & 2) || m->feat_lm_id[f] != m->lm_id[l]) continue;
            lkf.push_back(r);
            llm.push_back(s);
            luv.push_back(make_double2(m->feat_uv[2 * f], m->feat_uv[2 * f + 1]));
        }
        lptr[s + 1] = (int)lkf.size();
    }
    p->n_lm_obs = (int64_t)lkf.size();
    const std::vector<int> blk = pack_lm_blocks(lptr, p->n_opt, &p->max_lm_obs);
    p->n_lm_blocks = (int)blk.size() / 2 - 1;
    if (!device) return VX_OK;

    VX_HIP(c, hipSetDevice(c->device));
    int rc;
    if ((rc = upload(c, p->kf_pose0, pose0))) return rc;
    if ((rc = upload(c, p->kf_intr, intr))) return rc;
    if ((rc = upload(c, p->kf_flags, kf_flags))) return rc;
    if ((rc = upload(c, p->kf_obs_ptr, kf_obs_ptr))) return rc;
    if ((rc = upload(c, p->lm_pos0, lm0))) return rc;
    if ((rc = upload(c, p->pobs_uv, puv))) return rc;
    if ((rc = upload(c, p->pobs_lm, plm))) return rc;
    if ((rc = upload(c, p->lobs_ptr, lptr))) return rc;
    if ((rc = upload(c, p->lobs_kf, lkf))) return rc;
    if ((rc = upload(c, p->lobs_lm, llm))) return rc;
    if ((rc = upload(c, p->lm_blk, blk))) return rc;
    if ((rc = upload(c, p->lobs_uv, luv))) return rc;
    if ((rc = alloc_run_buffers(c, p))) return rc;
    return build_fused(c, p, kf_obs_ptr, plm, lptr, lkf);
}

// Kernel set of a run.  Every k_landmark_solve workgroup re-solves all window poses, so that
// redundancy grows as n_kf x workgroups: beyond the measured crossover (scripts/ba_window_sweep.py,
// DESIGN.md §6) the large-window kernels (poses solved once, one extra launch per iteration) are
// faster; they are also the only ones for windows beyond kMaxKfLds keyframes and for a landmark
// with more than kLmBlock observations.  `blocks` / `max_obs` are maxima over every shard of the
// window (all-reduced once for a sharded plan), so all ranks take the same kernels.
bool choose_lds_poses(const vx_ba_plan* p, int blocks, int max_obs) {
    return p->n_kf <= kMaxKfLds && !p->global_poses && (int64_t)p->n_kf * blocks <= 80000 && blocks <= 480 &&
           max_obs <= kLmBlock;
}

// The two-kernel path's stages, from the record's own counts (a plan's, or a lean plan's through
// ba_run_dyn).  lm_blocks: k_landmark_solve workgroups (a lean plan: the capacity grid).
int pose_stage(vx_ctx* c, const BAArgs& a, int it) {
    VX_HIP(c, launch(c, kStBaPose, k_pose_kf, dim3(a.n_kf * a.n_split), dim3(kPoseBlock), 0, c->stream, a, it));
    return VX_OK;
}

int landmark_stage(vx_ctx* c, const BAArgs& a, int it, int lm_blocks, bool lds_poses) {
    if (lds_poses) {
        const size_t lds = (size_t)a.n_kf * kLdsStride * sizeof(double) + (size_t)kLmBlock * (9 * sizeof(double) + sizeof(int));
        if (lds > 64 * 1024) {  // up to ~154 KB at kMaxKfLds keyframes (gfx950: 160 KB per workgroup)
            static std::atomic<uint64_t> done{0};
            VX_HIP(c, lds_attr_once(c->device, reinterpret_cast<const void*>(&k_landmark_solve), 160 * 1024, done));
        }
        VX_HIP(c, launch(c, kStBaLandmark, k_landmark_solve, dim3(lm_blocks), dim3(kLmBlock), (uint32_t)lds, c->stream,
                         a, it));
    } else {
        ProfScope ps(c, kStBaLandmark);
        hipLaunchKernelGGL(k_pose_solve_g, dim3((a.n_kf + 255) / 256), dim3(256), 0, c->stream, a, it);
        VX_LAUNCH_CHECK(c, "k_pose_solve_g");
        hipLaunchKernelGGL(k_landmark, dim3(std::max(1, (a.n_opt + 255) / 256)), dim3(256), 0, c->stream, a, it);
        VX_LAUNCH_CHECK(c, "k_landmark");
    }
    return VX_OK;
}

int reset_if_no_iterations(vx_ctx* c, const BAArgs& a) {
    if (a.max_iter != 0) return VX_OK;
    ProfScope ps(c, kStBaReset);
    const int n = std::max(a.n_kf * 8, std::max(a.n_lm, 1) * 4);
    hipLaunchKernelGGL(k_ba_reset, dim3((n + 255) / 256), dim3(256), 0, c->stream, a);
    VX_LAUNCH_CHECK(c, "k_ba_reset");
    return VX_OK;
}

// Whether this process holds one rank's shard of a window whose other shards are on other devices
// (a real sharded run); otherwise every shard of the window is among the n plans (n = 1: an unsharded
// plan; n > 1: the one-device emulation, vx_ba_shard_emulate_run).
bool one_of_many_ranks(const vx_ba_plan* p, int n) { return n == 1 && p->shard_count > 1; }

// The kernel set of a run from the maxima over every shard of the window — {landmark workgroups, most
// observations of one landmark, 1 if a shard has no fused layout} — so all shards take the same
// kernels, and the fused form only when every shard has the layout (their reductions must match).
// The n plans' own maxima when they are all of the window; a real rank all-reduces its own with the
// other ranks', once per plan (one small collective and a host synchronisation at its first run).
int choose_kernels(vx_ctx* c, vx_ba_plan* const* plans, int n) {
    int32_t mx[3] = {0, 0, 0};
    for (int r = 0; r < n; ++r) {
        mx[0] = std::max(mx[0], (int32_t)plans[r]->n_lm_blocks);
        mx[1] = std::max(mx[1], (int32_t)plans[r]->max_lm_obs);
        mx[2] = std::max(mx[2], plans[r]->fused ? 0 : 1);
    }
    if (one_of_many_ranks(plans[0], n)) {
        if (plans[0]->choice_made) return VX_OK;
#ifndef VX_NO_RCCL
        DevBuf d;
        VX_HIP(c, d.ensure(sizeof mx));
        VX_HIP(c, hipMemcpyAsync(d.p, mx, sizeof mx, hipMemcpyHostToDevice, c->stream));
        ncclResult_t r = ncclAllReduce(d.p, d.p, 3, ncclInt32, ncclMax, c->comm, c->stream);
        if (r != ncclSuccess) return set_error(c, VX_ERR_COMM, "ncclAllReduce: %s", ncclGetErrorString(r));
        int32_t all[3];
        VX_HIP(c, hipMemcpyAsync(all, d.p, sizeof all, hipMemcpyDeviceToHost, c->stream));
        VX_HIP(c, hipStreamSynchronize(c->stream));
        std::copy(all, all + 3, mx);
#else
        return set_error(c, VX_ERR_COMM, "built without RCCL");
#endif
    }
    for (int r = 0; r < n; ++r) {
        plans[r]->lds_poses = choose_lds_poses(plans[r], mx[0], mx[1]);
        plans[r]->fused_all = mx[2] == 0;
        plans[r]->choice_made = true;
    }
    return VX_OK;
}

FusedArgs make_fused_args(vx_ba_plan* p) {
    FusedArgs f{};
    const uint8_t* T = p->f_tab.as<uint8_t>();
    f.blk = reinterpret_cast<const int4*>(T + p->f_off.blk);
    f.lm_slot = reinterpret_cast<const int*>(T + p->f_off.lm_slot);
    f.lm_run = reinterpret_cast<const int2*>(T + p->f_off.lm_run);
    f.lobs_uv = p->f_lobs_uv.as<double2>();
    f.lobs_rec = reinterpret_cast<const int4*>(T + p->f_off.lobs_rec);
    f.kent = reinterpret_cast<const int4*>(T + p->f_off.kent);
    f.pobs_uv = p->f_pobs_uv.as<double2>();
    f.pobs_p = p->f_pobs_p.as<double4>();
    f.part = p->f_part.as<double>();
    f.maxl = p->f_maxl;
    f.n_part = p->n_kf * p->f_maxl;
    f.rowpart = p->shard_count > 1 ? p->f_rowpart.as<double>() : nullptr;
    f.costpart = p->f_costpart.as<double2>();
    f.stop_b = p->f_stop_b;
    f.lpos = p->f_lpos.as<double4>();
    f.epose = p->f_epose.as<double>();
    f.arow = p->f_atomic && p->shard_count <= 1 ? p->f_arow.as<double>() : nullptr;
    f.n_kf = p->n_kf;
    f.apro = p->opt.max_iterations >= 2;
    static const int drow_env = [] {
        const char* e = getenv("VX_BA_DROW");
        return e && e[0] == '0' ? 0 : 1;
    }();
    f.drow = drow_env;
    static const int padskip_env = [] {
        const char* e = getenv("VX_BA_PADSKIP");
        return e && e[0] == '0' ? 0 : 1;
    }();
    f.padskip = padskip_env;
    return f;
}

// the fused path's launches: prologue (iteration 0's pose stage, it = -1) or k_ba_iter(it)
// $VX_BA_COMPACT=0: the 512-thread iterations without the compacted pose stage (A/B runs)
bool ba_compact() {
    static const bool on = [] {
        // off by default: measured 0.0559 vs 0.0540 ms per C3 window (profiles/r04), VX_BA_COMPACT=1 on
        const char* e = std::getenv("VX_BA_COMPACT");
        return e && e[0] == '1';
    }();
    return on;
}

template <int kFT>
int fused_launch_t(vx_ctx* c, vx_ba_plan* p, const BAArgs& a, const FusedArgs& f, int it) {
    constexpr int lds = (int)fused_lds(kFT);
    constexpr int lds_c = (int)fused_lds_cmp(kFTSmall);
    static std::atomic<uint64_t> d0{0}, d1{0}, d2{0};  // (per device: ADVICE r4)
    VX_HIP(c, lds_attr_once(c->device, reinterpret_cast<const void*>(&k_ba_iter<true, kFT>), lds, d0));
    VX_HIP(c, lds_attr_once(c->device, reinterpret_cast<const void*>(&k_ba_iter<false, kFT>), lds, d1));
    VX_HIP(c, lds_attr_once(c->device, reinterpret_cast<const void*>(&k_ba_iter<false, kFTSmall, true>), lds_c, d2));
    if (it < 0)
        VX_HIP(c, launch(c, kStBaPrologue, k_ba_iter<true, kFT>, dim3(p->f_blocks), dim3(kFT), (uint32_t)lds, c->stream,
                         a, f, -1));
    else if (kFT == kFTSmall && ba_compact())
        VX_HIP(c, launch(c, kStBaIter, k_ba_iter<false, kFTSmall, true>, dim3(p->f_blocks), dim3(kFTSmall),
                         (uint32_t)lds_c, c->stream, a, f, it));
    else
        VX_HIP(c, launch(c, kStBaIter, k_ba_iter<false, kFT>, dim3(p->f_blocks), dim3(kFT), (uint32_t)lds, c->stream,
                         a, f, it));
    return VX_OK;
}
int fused_launch(vx_ctx* c, vx_ba_plan* p, const BAArgs& a, const FusedArgs& f, int it) {
    if (p->f_threads == kFTLarge) return fused_launch_t<kFTLarge>(c, p, a, f, it);
    if (p->f_threads == kFTNarrow) return fused_launch_t<kFTNarrow>(c, p, a, f, it);
    return fused_launch_t<kFTSmall>(c, p, a, f, it);
}
// sharded fused path: the rows of the partial buffer iteration it reads (parity it & 1) -> f_rowpart
int fused_row_sum(vx_ctx* c, vx_ba_plan* p, int it) {
    const int n = p->n_kf * kStride;
    ProfScope ps(c, kStBaPoseSum);
    hipLaunchKernelGGL(k_row_sum, dim3((n + 255) / 256), dim3(256), 0, c->stream,
                       (const double*)(p->f_part.as<double>() + (size_t)(it & 1) * p->n_kf * p->f_maxl * kStride),
                       p->n_kf, p->f_maxl, p->f_rowpart.as<double>());
    VX_LAUNCH_CHECK(c, "k_row_sum");
    return VX_OK;
}

// the peer reduction of iteration it's row sums into f_rowpart (plans set up by peer_setup or the
// emulation; every rank / shard of the window enqueues the same generations)
size_t peer_len(const vx_ba_plan* p) { return (size_t)p->n_kf * kStride; }
int peer_publish(vx_ctx* c, vx_ba_plan* p, int it, unsigned long long gen) {
    const size_t len = peer_len(p);
    double* blk = static_cast<double*>(p->peer_mem);
    if (!blk) return set_error(c, VX_ERR_STATE, "peer reduction: no block of its own");
    hipLaunchKernelGGL(k_peer_publish, dim3(1), dim3(1024), 0, c->stream,
                       (const double*)(p->f_part.as<double>() + (size_t)(it & 1) * p->n_kf * p->f_maxl * kStride), p->n_kf,
                       p->f_maxl, blk + (gen & 1) * len, reinterpret_cast<unsigned long long*>(blk + 2 * len), gen);
    VX_LAUNCH_CHECK(c, "k_peer_publish");
    return VX_OK;
}
int peer_gather(vx_ctx* c, vx_ba_plan* p, unsigned long long gen) {
    const size_t len = peer_len(p);
    const int n = (int)p->peer_base.size();
    PeerPtrs pp{};
    if (n < 1 || n > kMaxPeers) return set_error(c, VX_ERR_STATE, "peer reduction: %d ranks", n);
    for (int r = 0; r < n; ++r) {
        const double* b = static_cast<const double*>(p->peer_base[r]);
        if (!b) return set_error(c, VX_ERR_STATE, "peer reduction: rank %d's block is not mapped", r);
        pp.rows[r] = b;
        pp.flag[r] = reinterpret_cast<const unsigned long long*>(b + 2 * len);
    }
    hipLaunchKernelGGL(k_peer_gather, dim3(1), dim3(1024), 0, c->stream, pp, n, (int)len, (int)((gen & 1) * len), gen,
                       p->f_rowpart.as<double>(), reinterpret_cast<int*>(p->state.as<uint8_t>() + offsetof(BAState, fault)));
    VX_LAUNCH_CHECK(c, "k_peer_gather");
    return VX_OK;
}
size_t peer_bytes(const vx_ba_plan* p) { return ((2 * peer_len(p) + 8) * sizeof(double) + 4095) & ~(size_t)4095; }

#ifndef VX_NO_RCCL
// this rank's block (uncached device memory: the peers read it over xGMI), its IPC handle gathered
// from every rank over RCCL, the peers' blocks opened; once per plan, at its first sharded run
int peer_setup(vx_ctx* c, vx_ba_plan* p) {
    const int n = p->shard_count, me = p->shard_rank;
    if (n > kMaxPeers) return set_error(c, VX_ERR_INVALID, "$VX_BA_PEER: at most %d ranks", kMaxPeers);
    if (c->nranks != n || c->rank != me)  // (the handle table is indexed by communicator rank)
        return set_error(c, VX_ERR_INVALID, "$VX_BA_PEER: shard %d of %d on communicator rank %d of %d", me, n, c->rank,
                         c->nranks);
    const size_t bytes = peer_bytes(p);
    VX_HIP(c, hipExtMallocWithFlags(&p->peer_mem, bytes, hipDeviceMallocUncached));
    VX_HIP(c, hipMemsetAsync(p->peer_mem, 0, bytes, c->stream));  // (flags 0 before any rank can read them)
    hipIpcMemHandle_t h;
    VX_HIP(c, hipIpcGetMemHandle(&h, p->peer_mem));
    DevBuf d;
    VX_HIP(c, d.ensure((size_t)n * sizeof h));
    VX_HIP(c, hipMemcpyAsync(d.as<uint8_t>() + (size_t)me * sizeof h, &h, sizeof h, hipMemcpyHostToDevice, c->stream));
    ncclResult_t r = ncclAllGather(d.as<uint8_t>() + (size_t)me * sizeof h, d.p, sizeof h, ncclUint8, c->comm, c->stream);
    if (r != ncclSuccess) return set_error(c, VX_ERR_COMM, "ncclAllGather (peer handles): %s", ncclGetErrorString(r));
    std::vector<hipIpcMemHandle_t> all(n);
    VX_HIP(c, hipMemcpyAsync(all.data(), d.p, (size_t)n * sizeof h, hipMemcpyDeviceToHost, c->stream));
    VX_HIP(c, hipStreamSynchronize(c->stream));
    p->peer_base.assign(n, nullptr);
    for (int q = 0; q < n; ++q) {
        if (q == me) {
            p->peer_base[q] = p->peer_mem;
            continue;
        }
        void* ptr = nullptr;
        VX_HIP(c, hipIpcOpenMemHandle(&ptr, all[q], hipIpcMemLazyEnablePeerAccess));
        p->peer_opened.push_back(ptr);
        p->peer_base[q] = ptr;
    }
    p->peer = true;
    return VX_OK;
}
#endif

bool peer_requested() {
    const char* e = getenv("VX_BA_PEER");
    return e && e[0] == '1';
}

WinArgs make_win_args(vx_ba_plan* p) {
    uint8_t* W = p->f_win.as<uint8_t>();
    WinArgs w{};
    w.part = reinterpret_cast<wgran*>(W + p->win_part_off);
    w.stop = reinterpret_cast<wgran*>(W + p->win_stop_off);
    w.hello = reinterpret_cast<unsigned*>(W + p->win_hello_off);
    w.gen = reinterpret_cast<int*>(W + p->win_gen_off);
    w.bias = p->win_bias;
    w.fault = reinterpret_cast<int*>(p->state.as<uint8_t>() + offsetof(BAState, fault));
    return w;
}

bool win_active(const vx_ba_plan* p) { return p->fused && p->f_persist && !p->win_off && p->shard_count <= 1; }

// The one-device emulation's stand-in for the all-reduce (vx_ba_shard_emulate_run): the element-wise
// sum of the shards' blocks, in rank order, written back to every shard.
constexpr int kMaxEmuShards = 16;
struct PartPtrs {
    double* p[kMaxEmuShards];
};
__global__ void k_sum_parts(PartPtrs parts, int n, long long len) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len) return;
    double s = parts.p[0][i];
    for (int r = 1; r < n; ++r) s += parts.p[r][i];
    for (int r = 0; r < n; ++r) parts.p[r][i] = s;
}

// one buffer of every shard, summed over the shards: ncclAllReduce on a real rank (buf(p) this rank's),
// k_sum_parts over the n plans in the emulation
template <class Buf>
int sum_over_shards(vx_ctx* c, vx_ba_plan* const* plans, int n, size_t len, Buf buf) {
    if (one_of_many_ranks(plans[0], n)) {
#ifndef VX_NO_RCCL
        ProfScope ps(c, kStBaAllreduce);
        ncclResult_t r = ncclAllReduce(buf(plans[0]), buf(plans[0]), len, ncclDouble, ncclSum, c->comm, c->stream);
        if (r != ncclSuccess) return set_error(c, VX_ERR_COMM, "ncclAllReduce: %s", ncclGetErrorString(r));
        return VX_OK;
#else
        return set_error(c, VX_ERR_COMM, "built without RCCL");
#endif
    }
    PartPtrs parts{};
    for (int r = 0; r < n; ++r) parts.p[r] = buf(plans[r]);
    hipLaunchKernelGGL(k_sum_parts, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, c->stream, parts, n, (long long)len);
    VX_LAUNCH_CHECK(c, "k_sum_parts");
    return VX_OK;
}

// The row reducer: what iteration `it` of every shard reads is summed over the shards of the window.
// It is the only thing in which an unsharded run, a real rank's and the emulation's differ:
//   unsharded             nothing
//   fused form            every shard's k_row_sum -> f_rowpart, summed over the shards; with the peer
//                         reduction ($VX_BA_PEER=1) every shard publishes, then every shard gathers,
//                         under one generation counted alike by all of them
//   two-kernel form       kf_part summed over the shards
int reduce_rows(vx_ctx* c, vx_ba_plan* const* plans, int n, int it, bool fused, bool peer) {
    vx_ba_plan* p0 = plans[0];
    if (p0->shard_count <= 1) return VX_OK;
    int rc;
    if (!fused)
        return sum_over_shards(c, plans, n, (size_t)p0->n_kf * p0->n_split * kStride,
                               [](vx_ba_plan* p) { return p->kf_part.as<double>(); });
    if (peer) {
        const unsigned long long gen = p0->peer_gen + 1;
        for (int r = 0; r < n; ++r) {
            plans[r]->peer_gen = gen;
            if ((rc = peer_publish(c, plans[r], it, gen))) return rc;
        }
        for (int r = 0; r < n; ++r)
            if ((rc = peer_gather(c, plans[r], gen))) return rc;
        return VX_OK;
    }
    for (int r = 0; r < n; ++r)
        if ((rc = fused_row_sum(c, plans[r], it))) return rc;
    return sum_over_shards(c, plans, n, (size_t)p0->n_kf * kStride, [](vx_ba_plan* p) { return p->f_rowpart.as<double>(); });
}

// ONE RUN of a window, over its n >= 1 plans: an unsharded plan or a real rank's shard (n = 1), or every
// shard of the window on one device (the emulation).  The only statement of a run's order; per step
// the launches go over the plans in rank order.  The callers have checked that the plans are of one
// window (vx_ba_shard_emulate_run) or that the communicator fits the shard (plan_run).
int run_window(vx_ctx* c, vx_ba_plan* const* plans, int n) {
    vx_ba_plan* p0 = plans[0];
    if (p0->status != 0) {  // (nothing to optimise: nothing runs)
        for (int r = 0; r < n; ++r) plans[r]->ran = true;
        return VX_OK;
    }
    int rc;
    if ((rc = choose_kernels(c, plans, n))) return rc;
    const bool fused = p0->fused_all;
    const int M = p0->opt.max_iterations;
    BAArgs a[kMaxEmuShards];  // (filled up to n: no heap, nothing cleared beyond what runs)
    FusedArgs f[kMaxEmuShards];
    for (int r = 0; r < n; ++r) {
        a[r] = make_args(plans[r]);
        if (fused) f[r] = make_fused_args(plans[r]);
        if ((rc = reset_if_no_iterations(c, a[r]))) return rc;
    }
    if (M > 0 && n == 1 && win_active(p0)) {  // the persistent window: the whole run is one launch
        constexpr int lds = (int)win_lds(kFTSmall);
        static std::atomic<uint64_t> dw{0};
        VX_HIP(c, lds_attr_once(c->device, reinterpret_cast<const void*>(&k_ba_win<kFTSmall>), lds, dw));
        VX_HIP(c, launch(c, kStBaWin, k_ba_win<kFTSmall>, dim3(p0->f_blocks), dim3(kFTSmall), (uint32_t)lds, c->stream,
                         a[0], f[0], make_win_args(p0)));
    } else if (M > 0 && fused) {  // prologue (iteration 0's pose stage), then rows reduced -> k_ba_iter
        for (int r = 0; r < n; ++r)
            if ((rc = fused_launch(c, plans[r], a[r], f[r], -1))) return rc;
        // the peer reduction ($VX_BA_PEER=1): a real rank maps its block once per plan, at its first
        // run; the emulation's caller has set up every shard's and decides by the environment
        bool peer = p0->shard_count > 1 && peer_requested();
#ifndef VX_NO_RCCL
        if (one_of_many_ranks(p0, n)) {
            if (!p0->peer && peer && (rc = peer_setup(c, p0))) return rc;
            peer = p0->peer;
        }
#endif
        for (int it = 0; it < M; ++it) {
            if ((rc = reduce_rows(c, plans, n, it, true, peer))) return rc;
            for (int r = 0; r < n; ++r)
                if ((rc = fused_launch(c, plans[r], a[r], f[r], it))) return rc;
        }
    } else {  // two kernels per iteration: pose stage -> kf_part reduced -> landmark stage
        for (int it = 0; it < M; ++it) {
            for (int r = 0; r < n; ++r)
                if ((rc = pose_stage(c, a[r], it))) return rc;
            if ((rc = reduce_rows(c, plans, n, it, false, false))) return rc;
            for (int r = 0; r < n; ++r)
                if ((rc = landmark_stage(c, a[r], it, plans[r]->n_lm_blocks, plans[r]->lds_poses))) return rc;
        }
    }
    for (int r = 0; r < n; ++r) plans[r]->ran = true;
    return VX_OK;
}

int plan_run(vx_ctx* c, vx_ba_plan* p) {
    if (p->status == 0 && p->shard_count > 1) {
#ifndef VX_NO_RCCL
        if (!c->comm || c->nranks != p->shard_count || c->rank != p->shard_rank)
            return set_error(c, VX_ERR_STATE, "sharded plan needs vx_comm_init(%d ranks)", p->shard_count);
#else
        return set_error(c, VX_ERR_COMM, "built without RCCL");
#endif
    }
    return run_window(c, &p, 1);
}

// A persistent run whose wait ran out (its workgroups could not all be resident at once) is void: the
// plan keeps the per-iteration launches from now on and runs the window again.
int win_fallback(vx_ctx* c, vx_ba_plan* p) {
    p->win_off = true;
    p->graph.reset();
    VX_HIP(c, hipMemsetAsync(p->state.as<uint8_t>() + offsetof(BAState, fault), 0, sizeof(int), c->stream));
    return plan_run(c, p);
}

}  // namespace

// The iterations of a lean plan (ba_lean.hip): the two-kernel form's stages with the LDS-pose kernel
// over the capacity grid, the counts read from d.a.dyn on the device — no host synchronisation.
int ba_run_dyn(vx_ctx* c, const DynPlan& d) {
    int rc;
    for (int it = 0; it < d.a.max_iter; ++it)
        if ((rc = pose_stage(c, d.a, it)) || (rc = landmark_stage(c, d.a, it, d.grid_blocks, true))) return rc;
    return VX_OK;
}

}  // namespace vx

using namespace vx;

VX_KT_EXPORT(vx_ktrace_read_ba);

namespace vx {
// ba_lean.hip: vx_ba_optimize_map's one-call path (*fallback: the window needs a plan)
int lean_optimize_view(vx_ctx* c, vx_map_view* v, uint64_t ref, int has_ref, const vx_ba_options& o, vx_ba_stats* st,
                       bool* fallback);
}  // namespace vx

namespace {
// What both plan constructors do once their own arguments stood the null checks: the option and shard
// checks, a registered plan, the test's injected failure, the build (which first sets its own flags on
// the plan) and the destroy of a plan whose build failed.
template <class Build>
int create_plan(vx_ctx* c, const vx_ba_options& opt, int shard_rank, int shard_count, vx_ba_plan** out, Build build) {
    *out = nullptr;
    if (opt.max_iterations < 0 || opt.max_iterations > kMaxIter)
        return set_error(c, VX_ERR_INVALID, "max_iterations must be in [0, %d]", kMaxIter);
    if (shard_count < 1 || shard_rank < 0 || shard_rank >= shard_count)
        return set_error(c, VX_ERR_INVALID, "bad shard %d/%d", shard_rank, shard_count);
    auto* p = plan_new(c);
    p->opt = opt;
    p->shard_rank = shard_rank;
    p->shard_count = shard_count;
    int rc = plan_fault_injected(c);
    if (!rc) rc = build(p);
    if (rc) {
        vx_ba_plan_destroy(p);  // (also leaves c->plan_live)
        return rc;
    }
    *out = p;
    return VX_OK;
}
}  // namespace

extern "C" {

void vx_ba_default_options(vx_ba_options* o) {
    if (!o) return;
    o->window_size = 5;
    o->max_iterations = 5;
    o->min_pose_observations = 20;
    o->min_point_observations = 2;
    o->huber_delta = 5.0;
    o->max_reproj_error = 5.0;
}

int vx_ba_plan_create(vx_ctx* c, const vx_map_view* m, uint64_t ref, int has_ref, const vx_ba_options* opt,
                      int shard_rank, int shard_count, vx_ba_plan** out) {
    return vx_ba_plan_create_ex(c, m, ref, has_ref, opt, shard_rank, shard_count, 0, out);
}

int vx_ba_plan_create_ex(vx_ctx* c, const vx_map_view* m, uint64_t ref, int has_ref, const vx_ba_options* opt,
                         int shard_rank, int shard_count, int flags, vx_ba_plan** out) {
    if (!c || !out || !opt) return VX_ERR_INVALID;
    return create_plan(c, *opt, shard_rank, shard_count, out, [&](vx_ba_plan* p) {
        p->global_poses = (flags & VX_PLAN_GLOBAL_POSES) != 0;
        return (flags & VX_PLAN_HOST_BUILD) ? build_plan(c, m, ref, has_ref, p) : build_plan_device(c, m, ref, has_ref, p);
    });
}

int vx_ba_plan_create_dmap(vx_ctx* c, vx_dmap* m, uint64_t ref, int has_ref, const vx_ba_options* opt, int shard_rank,
                           int shard_count, vx_ba_plan** out) {
    if (!c || !out || !opt || !m || m->c != c) return c ? set_error(c, VX_ERR_INVALID, "vx_ba_plan_create_dmap: bad arguments") : VX_ERR_INVALID;
    return create_plan(c, *opt, shard_rank, shard_count, out, [&](vx_ba_plan* p) {
        p->from_dmap = true;
        return build_plan_dmap(c, m, ref, has_ref, p);
    });
}

int vx_ba_plan_apply_dmap(vx_ctx* c, vx_ba_plan* p, vx_dmap* m) {
    if (!c || !p || !m || p->c != c || m->c != c) return c ? set_error(c, VX_ERR_INVALID, "vx_ba_plan_apply_dmap: bad arguments") : VX_ERR_INVALID;
    if (!p->from_dmap) return set_error(c, VX_ERR_STATE, "plan was not built from a vx_dmap");
    if (!p->ran) return set_error(c, VX_ERR_STATE, "plan not run");
    if (p->status != 0) return VX_OK;
    if (win_active(p)) {  // (a persistent run whose waits ran out is void: run it again first)
        int fault = 0;
        VX_HIP(c, hipMemcpyAsync(&fault, p->state.as<uint8_t>() + offsetof(BAState, fault), sizeof fault,
                                 hipMemcpyDeviceToHost, c->stream));
        VX_HIP(c, hipStreamSynchronize(c->stream));
        if (fault)
            if (int rc = win_fallback(c, p)) return rc;
    }
    const int n = std::max(p->n_kf, p->n_opt);
    hipLaunchKernelGGL(k_apply_dmap, dim3((n + 255) / 256), dim3(256), 0, c->stream, (const BAState*)p->state.as<BAState>(),
                       (const double*)p->kf_pose.as<double>(), p->n_kf, (const double*)p->lm_pos.as<double>(), p->n_opt,
                       (const int*)p->kf_map_dev.as<int>(), (const int*)p->lm_map_dev.as<int>(), m->kf_pose.as<double>(),
                       m->lm_pos.as<double>());
    VX_LAUNCH_CHECK(c, "k_apply_dmap");
    return VX_OK;
}

int vx_ba_plan_run_async(vx_ctx* c, vx_ba_plan* p) {
    if (!c || !p || p->c != c) return VX_ERR_INVALID;
    if (p->status != 0) return plan_run(c, p);
    // Sharded plans: the first run is eager (its one small all-reduce fixes the kernel set on every
    // rank and synchronises); later runs replay ONE hipGraph of the whole sequence, the per-iteration
    // k_row_sum -> ncclAllReduce -> k_ba_iter chain included (RCCL collectives are capturable: the
    // graph holds their kernels).  A capture that fails leaves the plan eager; $VX_SHARDED_GRAPHS=0
    // keeps every sharded run eager, and so does the peer reduction ($VX_BA_PEER=1).
    if (p->shard_count > 1) {
        const char* e = std::getenv("VX_SHARDED_GRAPHS");
        // (the peer reduction stays eager: its generations change from run to run)
        if (!p->choice_made || p->graph_eager || p->peer || peer_requested() || (e && e[0] == '0')) return plan_run(c, p);
        const bool capturing = c->use_graphs && !c->prof && p->graph.seen && !p->graph.exec;
        p->ran = true;
        const int rc =
            graph_run_owned(c, p->graph, [](vx_ctx* cc, void* v) { return plan_run(cc, static_cast<vx_ba_plan*>(v)); }, p);
        if (rc != VX_OK && capturing) {
            p->graph_eager = true;
            return plan_run(c, p);
        }
        return rc;
    }
    p->ran = true;
    // the persistent window is ONE kernel: launched directly (a graph launch of one kernel node costs
    // the host more and the stream extra packets, $VX_BA_WIN_GRAPH=1 for it)
    static const bool win_graph = [] {
        const char* e = std::getenv("VX_BA_WIN_GRAPH");
        return e && e[0] == '1';
    }();
    if (win_active(p) && !win_graph && !c->prof) return plan_run(c, p);
    return graph_run_owned(c, p->graph, [](vx_ctx* cc, void* v) { return plan_run(cc, static_cast<vx_ba_plan*>(v)); }, p);
}

namespace {
int shard_emulate_enqueue(vx_ctx* c, vx_ba_plan* const* plans, int n);
struct EmuArgs {
    vx_ba_plan* const* plans;
    int n;
};
}  // namespace

// The emulated sharded run goes through the context's graph cache like a real sharded run's
// sequence: eager on its first sighting, captured on the second, replayed afterwards (keyed by the
// shard plans), so the tests exercise the captured form of the row sum -> reduction -> k_ba_iter chain.
int vx_ba_shard_emulate_run(vx_ctx* c, vx_ba_plan* const* plans, int n) {
    if (!c || !plans || n < 1 || n > kMaxEmuShards) return c ? set_error(c, VX_ERR_INVALID, "vx_ba_shard_emulate_run: bad arguments") : VX_ERR_INVALID;
    for (int r = 0; r < n; ++r)
        if (!plans[r] || plans[r]->c != c) return set_error(c, VX_ERR_INVALID, "shard %d: plan of another context", r);
    std::vector<uint64_t> key{0xE3u, (uint64_t)n};
    for (int r = 0; r < n; ++r) key.push_back((uint64_t)(uintptr_t)plans[r]);
    EmuArgs ea{plans, n};
    // (eager: the first run decides the kernels; the peer reduction's generations change every run; one
    // unsharded plan's persistent window is one launch, and a captured one would outlive its win_off)
    if (plans[0]->status != 0 || !plans[0]->choice_made || peer_requested() || (n == 1 && win_active(plans[0])))
        return shard_emulate_enqueue(c, plans, n);
    for (int r = 0; r < n; ++r) plans[r]->ran = true;
    return graph_run(c, key, [](vx_ctx* cc, void* v) {
        const EmuArgs* x = static_cast<const EmuArgs*>(v);
        return shard_emulate_enqueue(cc, x->plans, x->n);
    }, &ea);
}

namespace {
int shard_emulate_enqueue(vx_ctx* c, vx_ba_plan* const* plans, int n) {
    vx_ba_plan* p0 = plans[0];
    for (int r = 0; r < n; ++r) {
        const vx_ba_plan* p = plans[r];
        if (!p || p->c != c || p->shard_count != n || p->shard_rank != r)
            return set_error(c, VX_ERR_INVALID, "shard %d: plan of another context or shard layout", r);
        if (p->status != p0->status || p->n_kf != p0->n_kf || p->n_split != p0->n_split ||
            p->opt.max_iterations != p0->opt.max_iterations)
            return set_error(c, VX_ERR_INVALID, "shard %d: plan built from another window", r);
    }
    // $VX_BA_PEER=1 (sharded fused plans): the peer reduction's kernels in place of k_sum_parts, each
    // shard's block in device memory of its own and every shard's base table naming all of them (the
    // IPC mapping of a real multi-GPU run: peer_setup); the run counts generations as a real run does
    bool peer = p0->status == 0 && n > 1 && peer_requested();
    for (int r = 0; r < n; ++r) peer = peer && plans[r]->fused;
    if (peer) {
        for (int r = 0; r < n; ++r)
            if (!plans[r]->peer_mem) {
                VX_HIP(c, hipMalloc(&plans[r]->peer_mem, peer_bytes(plans[r])));
                VX_HIP(c, hipMemsetAsync(plans[r]->peer_mem, 0, peer_bytes(plans[r]), c->stream));
            }
        for (int r = 0; r < n; ++r) {  // (every block allocated before any table names it)
            plans[r]->peer_base.assign(n, nullptr);
            for (int q = 0; q < n; ++q) plans[r]->peer_base[q] = plans[q]->peer_mem;
        }
    }
    return run_window(c, plans, n);
}
}  // namespace

int vx_ba_plan_fetch(vx_ctx* c, vx_ba_plan* p, vx_map_view* m, vx_ba_stats* st) {
    if (!c || !p || p->c != c) return VX_ERR_INVALID;
    if (!p->ran) return set_error(c, VX_ERR_STATE, "plan not run");
    if (m && p->from_dmap) return set_error(c, VX_ERR_STATE, "dmap plan: scatter with vx_ba_plan_apply_dmap");
    vx_ba_stats s{};
    s.gate_margin = -1.0;
    s.status = p->status;
    s.n_window_kf = p->n_window_kf;
    s.n_landmarks = p->n_landmarks_global;
    if (p->status == 0) {
        // one synchronisation: the state, BOTH pose parities (the last iteration's is known only from
        // the state) and the positions into one host-cached pinned block
        const size_t sb = sizeof(BAState), pb = 2 * (size_t)p->n_kf * 8 * sizeof(double),
                     lb = (size_t)p->n_opt * 4 * sizeof(double);
        const size_t o_pose = (sb + 63) & ~(size_t)63, o_lm = o_pose + ((pb + 63) & ~(size_t)63);
        VX_HIP(c, p->fetch_host.ensure(o_lm + lb + 64, true));
        uint8_t* H = static_cast<uint8_t*>(p->fetch_host.p);
        auto read_back = [&]() -> int {
            VX_HIP(c, hipMemcpyAsync(H, p->state.p, sb, hipMemcpyDeviceToHost, c->stream));
            VX_HIP(c, hipMemcpyAsync(H + o_pose, p->kf_pose.p, pb, hipMemcpyDeviceToHost, c->stream));
            if (lb) VX_HIP(c, hipMemcpyAsync(H + o_lm, p->lm_pos.p, lb, hipMemcpyDeviceToHost, c->stream));
            VX_HIP(c, hipStreamSynchronize(c->stream));
            return VX_OK;
        };
        int rc = read_back();
        if (rc) return rc;
        BAState hs;
        std::memcpy(&hs, H, sb);
        if (hs.fault && !p->peer_base.empty() && p->shard_count > 1)
            return set_error(c, VX_ERR_COMM, "peer reduction: a rank's row sums did not arrive within 200 ms");
        if (hs.fault && win_active(p)) {
            if ((rc = win_fallback(c, p))) return rc;
            if ((rc = read_back())) return rc;
            std::memcpy(&hs, H, sb);
        }
        // the poses of the last iteration run are in ping-pong buffer (iterations & 1)
        const double* pose = reinterpret_cast<const double*>(H + o_pose) + (size_t)(hs.iterations & 1) * p->n_kf * 8;
        const double* lm = reinterpret_cast<const double*>(H + o_lm);
        if (c->prof) prof_collect(c);
        state_to_stats(hs, &s);
        if (m) {
            for (int r = 0; r < p->n_kf; ++r)
                for (int j = 0; j < 7; ++j) m->kf_pose[7 * p->kf_map_idx[r] + j] = pose[8 * r + j];
            for (int sl = 0; sl < p->n_opt; ++sl)
                for (int j = 0; j < 3; ++j) m->lm_pos[3 * p->lm_map_idx[sl] + j] = lm[4 * sl + j];
        }
    }
    if (st) *st = s;
    return VX_OK;
}

void vx_ba_plan_destroy(vx_ba_plan* p) {
    if (!p) return;
    vx_ctx* c = p->c;
    if (c) {
        auto& live = c->plan_live;
        live.erase(std::remove(live.begin(), live.end(), p), live.end());
        // captured emulated sharded sequences naming this plan (vx_ba_shard_emulate_run's keys
        // {0xE3, n, plans...}) bake its buffers in: drop them before the address can be reused
        auto& ge = c->graphs.entries;
        for (auto it = ge.begin(); it != ge.end();) {
            const bool names = !it->key.empty() && it->key[0] == 0xE3u &&
                               std::find(it->key.begin() + 2, it->key.end(), (uint64_t)(uintptr_t)p) != it->key.end();
            if (names) {
                if (it->exec) (void)hipGraphExecDestroy(it->exec);
                it = ge.erase(it);
            } else {
                ++it;
            }
        }
        if (c->plan_husks.size() < kMaxPlanHusks) {  // park the buffers (no hipFree)
            auto* h = new vx_ba_plan();
            adopt_buffers(h, p);
            c->plan_husks.push_back(h);
        }
    }
    for (void* q : p->peer_opened) (void)hipIpcCloseMemHandle(q);
    if (p->peer_mem) (void)hipFree(p->peer_mem);
    delete p;
}

int vx_ba_plan_inspect(const vx_map_view* m, uint64_t ref, int has_ref, const vx_ba_options* opt, int shard_rank,
                       int shard_count, int64_t* out8, int32_t* lm_map_idx, int cap_lm, int32_t* kf_map_idx,
                       int cap_kf) {
    if (!opt || !out8 || shard_count < 1 || shard_rank < 0 || shard_rank >= shard_count) return VX_ERR_INVALID;
    vx_ba_plan p;
    p.opt = *opt;
    p.shard_rank = shard_rank;
    p.shard_count = shard_count;
    const int rc = build_plan(nullptr, m, ref, has_ref, &p, false);
    if (rc) return rc;
    const int64_t v[8] = {p.status, p.n_window_kf, p.n_landmarks_global, p.n_kf, p.n_opt, p.n_lm, p.n_pose_obs,
                          p.n_lm_obs};
    for (int i = 0; i < 8; ++i) out8[i] = v[i];
    if (lm_map_idx) {
        if ((int)p.lm_map_idx.size() > cap_lm) return VX_ERR_CAPACITY;
        for (size_t i = 0; i < p.lm_map_idx.size(); ++i) lm_map_idx[i] = p.lm_map_idx[i];
    }
    if (kf_map_idx) {
        if ((int)p.kf_map_idx.size() > cap_kf) return VX_ERR_CAPACITY;
        for (size_t i = 0; i < p.kf_map_idx.size(); ++i) kf_map_idx[i] = p.kf_map_idx[i];
    }
    return VX_OK;
}

uint32_t vx_ba_shard_of(uint64_t lm_id, int shard_count) {
    return shard_count <= 1 ? 0u : (uint32_t)(vx::ba::splitmix64(lm_id) % (uint64_t)shard_count);
}

int vx_ba_plan_info(const vx_ba_plan* p, int64_t* out8) {
    if (!p || !out8) return VX_ERR_INVALID;
    const int64_t v[8] = {p->n_kf, p->n_lm, p->n_pose_obs, p->n_lm_obs, p->n_opt, p->n_split, p->n_lm_blocks,
                          p->max_lm_obs};
    for (int i = 0; i < 8; ++i) out8[i] = v[i];
    return VX_OK;
}

int vx_ba_plan_layout(const vx_ba_plan* p, int64_t* out4) {
    if (!p || !out4) return VX_ERR_INVALID;
    out4[0] = p->fused ? 1 : 0;
    out4[1] = p->fused ? p->f_threads : 0;
    out4[2] = p->fused ? p->f_blocks : 0;
    out4[3] = p->fused ? p->f_maxl : 0;
    return VX_OK;
}

int vx_ba_plan_persistent(const vx_ba_plan* p) { return p && win_active(p) ? 1 : 0; }

int vx_ba_plan_fused_tables(vx_ctx* c, const vx_ba_plan* p, void* dst, size_t cap, size_t* bytes) {
    if (!c || !p || !bytes || p->c != c) return VX_ERR_INVALID;
    if (!p->fused) return set_error(c, VX_ERR_STATE, "plan has no fused layout");
    const FusedOffsets& F = p->f_off;
    const size_t n_lp = (size_t)p->f_blocks * p->f_threads;
    const std::pair<size_t, size_t> part[] = {
        {F.blk, (size_t)p->f_blocks * fused_blk_ints(p->f_threads) * 4},
        {F.lm_slot, n_lp * 4},
        {F.lm_run, n_lp * 8},
        {F.lobs_rec, n_lp * 16},
        {F.kent, (size_t)p->f_blocks * kFK * 32},
        {F.lobs_src, n_lp * 4},
        {F.pobs_src, p->f_npp * 4},
        {F.pobs_code, p->f_npp * 4}};
    size_t total = 0;
    for (const auto& x : part) total += x.second;
    *bytes = total;
    if (!dst) return VX_OK;
    if (cap < total) return VX_ERR_CAPACITY;
    VX_HIP(c, hipSetDevice(c->device));
    size_t at = 0;
    for (const auto& x : part) {
        if (x.second)
            VX_HIP(c, hipMemcpyAsync(static_cast<uint8_t*>(dst) + at, p->f_tab.as<uint8_t>() + x.first, x.second,
                                     hipMemcpyDeviceToHost, c->stream));
        at += x.second;
    }
    VX_HIP(c, hipStreamSynchronize(c->stream));
    return VX_OK;
}

int vx_ba_optimize_map(vx_ctx* c, vx_map_view* m, uint64_t ref, int has_ref, const vx_ba_options* opt,
                       vx_ba_stats* st) {
    if (!c) return VX_ERR_INVALID;
    // ($VX_OPT_TIMING=1: the call's phases on stderr, scripts/adapter_timing.py)
    static const bool timing = getenv("VX_OPT_TIMING") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (timing)
            std::fprintf(stderr, "[vx optmap] %s %.1f us\n", what,
                         std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    };
    // the lean one-call build on the view loaded into the context's scratch map for windows of up to
    // 64 keyframes; the plan below for larger ones (C3, 50: 0.37 against 0.62 ms; C4, 100: the plan's
    // fused window wins, 0.93 against 1.20 ms, profiles/r06/bench_c4_r06.json) and for a window the
    // lean build does not take.  $VX_OPTMAP_LEAN=0 / 1: always the plan / the lean build (A/B runs)
    static const int lean_env = [] {
        const char* e = getenv("VX_OPTMAP_LEAN");
        return e ? (e[0] == '0' ? 0 : 1) : -1;
    }();
    const bool lean = m && opt && opt->max_iterations >= 0 && opt->max_iterations <= 64 &&
                      (lean_env == 1 || (lean_env < 0 && std::min(opt->window_size, m->n_kf) <= 64));
    if (lean) {
        bool fb = false;
        const int rc = lean_optimize_view(c, m, ref, has_ref, *opt, st, &fb);
        lap("lean");
        if (!fb) return rc;
    }
    vx_ba_plan* p = nullptr;
    int rc = vx_ba_plan_create(c, m, ref, has_ref, opt, 0, 1, &p);
    lap("plan_create");
    if (rc) return rc;
    rc = vx_ba_plan_run_async(c, p);
    if (timing) (void)hipStreamSynchronize(c->stream);
    lap("run");
    if (!rc) rc = vx_ba_plan_fetch(c, p, m, st);
    lap("fetch");
    (void)hipStreamSynchronize(c->stream);
    vx_ba_plan_destroy(p);
    lap("destroy");
    return rc;
}

}  // extern "C"
