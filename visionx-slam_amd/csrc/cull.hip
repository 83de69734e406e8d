// cull.hip — Tracking::CullLandmarks (core/frontend/tracking.cpp:652-750), Tracking::CullKeyFrames
// (:775-840) and Tracking::RemoveKeyFrame (:752-773) on the device-resident map (vx_dmap_cull_*).
//
// The reference walks Map::Landmarks() with one Map::GetFrame (a mutex and a std::map lookup) and one
// projection per observation, and Map::KeyFrames() with one Map::GetLandmark per feature.  Everything
// those walks read is resident: the landmark-major observation CSR (optr / okf / ofi, dmap.hip), the
// features, the landmark id -> row table (lm_hash.hpp), and — after a LocalBA on the map — the only
// current copy of the poses and positions.  The sequence of a CullLandmarks call is
//
//   [dmap_build_csr, ht_sync]  ->  upload of the live keyframe rows (ascending id)  ->  k_cull_kfgeo
//   ->  k_cull_scan  ->  k_cull_prefix  ->  k_cull_apply  ->  one synchronisation
//
// k_cull_kfgeo   one thread per live keyframe: rotation matrix of the pose quaternion, t, intrinsics
//                (16 doubles), read once per call instead of once per observation.
// k_cull_scan    one thread per landmark row, kBlock rows per workgroup.  The keyframe table (id, feature
//                range, camera flag, the 16 doubles: 152 B per keyframe) is copied into LDS when the
//                map has at most kLdsKf live keyframes and binary-searched by each observation's
//                keyframe id; above that the same search reads the table from global memory.  A
//                thread walks its landmark's CSR segment in insertion order, so err_sum is one
//                sequential sum whose order is the map's: repeated runs are bitwise equal.  The
//                outcome does not depend on the order (any error > 2 tau culls, wherever it comes; the
//                sum is used only when there is none), so stopping at the first large error as the
//                reference does over its unordered_map decides the same.  Per row: reason, projected
//                count, mean, and — for a culled row — how many features its removal resets; per
//                workgroup: the two totals.
// k_cull_prefix  one workgroup: exclusive prefix of the workgroup totals, and the two grand totals.
// k_cull_apply   same grid: a culled row's place in the lists is its workgroup's offset plus its rank
//                inside the workgroup (wave64 ballot + mbcnt for the landmark list, a shuffle scan for
//                the feature list, wave totals through LDS), so both lists come out in landmark row
//                order whatever the dispatch order — no atomic append.  It writes the records into
//                the map's pinned host block, resets the features (feat_lm = 0, feat_fl = outlier)
//                and sets lm_bad = kLmRemoved.
//
// CullKeyFrames: k_cull_redundancy (one workgroup per live keyframe: total / redundant over its
// features through ht_get, lm_bad and the CSR segment length) -> synchronisation, the host picks the
// keyframe with the reference's own double expression -> k_cull_rmkf (one workgroup, the keyframe's
// features in order: tombstones the (landmark, keyframe) rows through the CSR's sort permutation,
// marks the CSR entries dead for the scan that follows, resets the features) -> the sequence above
// -> synchronisation.
//
// Every store is a plain vector store; no atomics.  Algorithmic bytes: DESIGN.md §27.
#include <algorithm>
#include <cstring>

#include "vx_internal.hpp"
#include "dmap.hpp"
#include "lm_hash.hpp"

namespace vx {
namespace {

constexpr int kBlock = 256;         // landmark rows per scan workgroup
constexpr int kWaves = kBlock / 64;
constexpr int kLdsKf = 128;         // live keyframes whose table the scan holds in LDS (19 KB)
constexpr int kKfBlock = 1024;      // k_cull_rmkf: one workgroup, chunks of 1024 features
constexpr int kKfWaves = kKfBlock / 64;
constexpr uint8_t kResetFlags = 2;  // has_landmark = false, is_outlier = true

struct KfTable {          // live keyframes in ascending id
    int n;
    const uint64_t* id;
    const int64_t* f0;    // first resident feature row
    const int* row;       // map row
    const int* nf;        // features
    const int* cam;       // has a camera
    const double* geo;    // 16 per keyframe: R (row major) | t | fx fy cx cy
};

struct ScanArgs {
    KfTable kt;
    int64_t nl;
    int min_obs;
    double tau;
    const int64_t* optr;
    const uint64_t* okf;
    const uint64_t* ofi;
    const uint8_t* odead;   // null: no CSR entry is dead
    const uint64_t* lm_id;
    const double* lm_pos;
    uint8_t* lm_bad;
    const double* feat_uv;
    uint64_t* feat_lm;
    uint8_t* feat_fl;
    // per row / per workgroup
    int* reason;
    int* cnt;
    double* mean;
    int* nreset;
    int2* blk_cnt;
    const int2* blk_off;
    // pinned host block
    int* hdr;
    vx_cull_landmark* out_lm;
    vx_cull_feature* out_ft;
    int cap_lm, cap_ft;
};

// Map::GetFrame(kf): index in the table, -1 when the keyframe is not in the map
__device__ __forceinline__ int kf_find(const uint64_t* id, int n, uint64_t k) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (id[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return (lo < n && id[lo] == k) ? lo : -1;
}

__global__ void __launch_bounds__(kBlock) k_cull_kfgeo(int n, const int* row, const double* kf_pose,
                                                       const double* kf_intr, double* geo) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double* q = kf_pose + 7 * (int64_t)row[i];
    const double* in = kf_intr + 4 * (int64_t)row[i];
    double* g = geo + 16 * (int64_t)i;
    // Eigen Quaternion::toRotationMatrix
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    g[0] = 1.0 - (tyy + tzz), g[1] = txy - twz, g[2] = txz + twy;
    g[3] = txy + twz, g[4] = 1.0 - (txx + tzz), g[5] = tyz - twx;
    g[6] = txz - twy, g[7] = tyz + twx, g[8] = 1.0 - (txx + tyy);
    g[9] = q[4], g[10] = q[5], g[11] = q[6];
    g[12] = in[0], g[13] = in[1], g[14] = in[2], g[15] = in[3];
}

// the feature an observation (keyframe id, feature index) names, when the keyframe is in the map and
// the index in range (tracking.cpp:681-687, :735-738): its resident row, else -1; *e = the table index
__device__ __forceinline__ int64_t obs_feature(const uint64_t* t_id, const int64_t* t_f0, const int* t_nf, int nk,
                                               uint64_t kf, uint64_t fi, int* e) {
    const int i = kf_find(t_id, nk, kf);
    *e = i;
    if (i < 0 || fi >= (uint64_t)t_nf[i]) return -1;
    return t_f0[i] + (int64_t)fi;
}

template <bool kLds>
__global__ void __launch_bounds__(kBlock) k_cull_scan(ScanArgs a) {
    __shared__ uint64_t s_id[kLds ? kLdsKf : 1];
    __shared__ int64_t s_f0[kLds ? kLdsKf : 1];
    __shared__ int s_nf[kLds ? kLdsKf : 1];
    __shared__ int s_cam[kLds ? kLdsKf : 1];
    __shared__ double s_geo[kLds ? 16 * kLdsKf : 1];
    __shared__ int s_lm[kWaves], s_ft[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nk = a.kt.n;
    const uint64_t* t_id;
    const int64_t* t_f0;
    const int* t_nf;
    const int* t_cam;
    const double* t_geo;
    if constexpr (kLds) {
        for (int i = tid; i < nk; i += kBlock) {
            s_id[i] = a.kt.id[i];
            s_f0[i] = a.kt.f0[i];
            s_nf[i] = a.kt.nf[i];
            s_cam[i] = a.kt.cam[i];
        }
        for (int i = tid; i < 16 * nk; i += kBlock) s_geo[i] = a.kt.geo[i];
        __syncthreads();
        t_id = s_id, t_f0 = s_f0, t_nf = s_nf, t_cam = s_cam, t_geo = s_geo;
    } else {
        t_id = a.kt.id, t_f0 = a.kt.f0, t_nf = a.kt.nf, t_cam = a.kt.cam, t_geo = a.kt.geo;
    }

    const int64_t r = (int64_t)blockIdx.x * kBlock + tid;
    int reason = 0, cnt = 0, nreset = 0;
    double mean = 0.0;
    if (r < a.nl && a.lm_bad[r] != kLmRemoved) {
        const int64_t o0 = a.optr[r], o1 = a.optr[r + 1];
        const uint64_t id = a.lm_id[r];
        int64_t live = o1 - o0;  // ObservationCount(): the live pairs, whatever keyframe they name
        if (a.odead)
            for (int64_t o = o0; o < o1; ++o) live -= a.odead[o];
        if (a.lm_bad[r] != 0) {
            reason = VX_CULL_ALREADY_BAD;                 // (:666)
        } else if (live < (int64_t)a.min_obs) {
            reason = VX_CULL_FEW_OBSERVATIONS;            // (:670)
        } else {
            const double px = a.lm_pos[3 * r], py = a.lm_pos[3 * r + 1], pz = a.lm_pos[3 * r + 2];
            double sum = 0.0;
            bool large = false;
            for (int64_t o = o0; o < o1 && !large; ++o) {
                if (a.odead && a.odead[o]) continue;
                int e;
                const int64_t f = obs_feature(t_id, t_f0, t_nf, nk, a.okf[o], a.ofi[o], &e);
                if (f < 0) continue;                                        // (:682-687)
                if (!(a.feat_fl[f] & 1) || a.feat_lm[f] != id) continue;    // (:689)
                if (!t_cam[e]) continue;                                    // (:694)
                const double* g = t_geo + 16 * e;
                // ProjectToPixel (common/projection.h:16-25)
                const double cx_ = g[0] * px + g[1] * py + g[2] * pz + g[9];
                const double cy_ = g[3] * px + g[4] * py + g[5] * pz + g[10];
                const double cz_ = g[6] * px + g[7] * py + g[8] * pz + g[11];
                if (cz_ <= 1e-6) continue;
                const double inv_z = 1.0 / cz_;
                const double u = g[12] * (cx_ * inv_z) + g[14], v = g[13] * (cy_ * inv_z) + g[15];
                const double dx = a.feat_uv[2 * f] - u, dy = a.feat_uv[2 * f + 1] - v;
                const double err = sqrt(dx * dx + dy * dy);
                sum += err;
                ++cnt;
                if (err > a.tau * 2.0) large = true;                        // (:707)
            }
            if (cnt == 0) reason = VX_CULL_NO_PROJECTION;                   // (:713)
            else if (large) reason = VX_CULL_LARGE_ERROR;
            else if (sum / cnt > a.tau) {                                   // (:719)
                reason = VX_CULL_MEAN_ERROR;
                mean = sum / cnt;
            }
        }
        if (reason) {  // the features its removal resets (:734-745)
            for (int64_t o = o0; o < o1; ++o) {
                if (a.odead && a.odead[o]) continue;
                int e;
                const int64_t f = obs_feature(t_id, t_f0, t_nf, nk, a.okf[o], a.ofi[o], &e);
                if (f >= 0 && a.feat_lm[f] == id) ++nreset;
            }
        }
    }
    if (r < a.nl) {
        a.reason[r] = reason;
        a.cnt[r] = cnt;
        a.mean[r] = mean;
        a.nreset[r] = nreset;
    }
    // workgroup totals, fixed order
    int c_lm = reason ? 1 : 0, c_ft = nreset;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        c_lm += __shfl_xor(c_lm, off);
        c_ft += __shfl_xor(c_ft, off);
    }
    if (lane == 0) {
        s_lm[wave] = c_lm;
        s_ft[wave] = c_ft;
    }
    __syncthreads();
    if (tid == 0) {
        int x = 0, y = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            x += s_lm[w];
            y += s_ft[w];
        }
        a.blk_cnt[blockIdx.x] = make_int2(x, y);
    }
}

// exclusive prefix of the workgroup totals (one workgroup), the grand totals into hdr[0], hdr[1]
__global__ void __launch_bounds__(kBlock) k_cull_prefix(const int2* cnt, int nb, int2* off, int* hdr) {
    __shared__ int s_x[kWaves], s_y[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int bx = 0, by = 0;
    for (int base = 0; base < nb; base += kBlock) {
        const int i = base + tid;
        const int2 v = i < nb ? cnt[i] : make_int2(0, 0);
        int x = v.x, y = v.y;  // inclusive scan inside the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int ox = __shfl_up(x, d), oy = __shfl_up(y, d);
            if (lane >= d) {
                x += ox;
                y += oy;
            }
        }
        if (lane == 63) {
            s_x[wave] = x;
            s_y[wave] = y;
        }
        __syncthreads();
        int px = 0, py = 0, tx = 0, ty = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            px += w < wave ? s_x[w] : 0;
            py += w < wave ? s_y[w] : 0;
            tx += s_x[w];
            ty += s_y[w];
        }
        __syncthreads();
        if (i < nb) off[i] = make_int2(bx + px + x - v.x, by + py + y - v.y);
        bx += tx;
        by += ty;
    }
    if (tid == 0) {
        hdr[0] = bx;
        hdr[1] = by;
    }
}

__global__ void __launch_bounds__(kBlock) k_cull_apply(ScanArgs a) {
    __shared__ int s_lm[kWaves], s_ft[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r = (int64_t)blockIdx.x * kBlock + tid;
    const int reason = r < a.nl ? a.reason[r] : 0;
    const int nreset = r < a.nl ? a.nreset[r] : 0;
    // rank among the workgroup's culled rows: ballot + mbcnt; feature offset: shuffle scan
    const uint64_t b = __ballot(reason != 0);
    int k_lm = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
    int inc = nreset;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    if (lane == 63) s_ft[wave] = inc;
    if (lane == 0) s_lm[wave] = __popcll(b);
    __syncthreads();
    int k_ft = inc - nreset;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        k_lm += w < wave ? s_lm[w] : 0;
        k_ft += w < wave ? s_ft[w] : 0;
    }
    if (!reason) return;
    const int2 base = a.blk_off[blockIdx.x];
    k_lm += base.x;
    k_ft += base.y;
    const uint64_t id = a.lm_id[r];
    if (k_lm < a.cap_lm) {
        vx_cull_landmark rec;
        rec.lm_id = id;
        rec.row = (int)r;
        rec.reason = reason;
        rec.n_projected = a.cnt[r];
        rec.reserved = 0;
        rec.mean_err = a.mean[r];
        a.out_lm[k_lm] = rec;
    }
    // the reset of :734-745 over the landmark's live pairs, in insertion order
    const int nk = a.kt.n;
    const int64_t o0 = a.optr[r], o1 = a.optr[r + 1];
    int j = 0;
    for (int64_t o = o0; o < o1 && j < nreset; ++o) {
        if (a.odead && a.odead[o]) continue;
        int e;
        const int64_t f = obs_feature(a.kt.id, a.kt.f0, a.kt.nf, nk, a.okf[o], a.ofi[o], &e);
        if (f < 0 || a.feat_lm[f] != id) continue;
        a.feat_lm[f] = 0;
        a.feat_fl[f] = kResetFlags;
        if (k_ft + j < a.cap_ft) {
            vx_cull_feature rec;
            rec.kf_id = a.okf[o];
            rec.kf_row = a.kt.row[e];
            rec.feat_idx = (int)a.ofi[o];
            a.out_ft[k_ft + j] = rec;
        }
        ++j;
    }
    a.lm_bad[r] = kLmRemoved;  // Map::RemoveLandmark (:746)
}

struct RedArgs {
    KfTable kt;
    int min_shared;
    const uint64_t* feat_lm;
    const uint8_t* feat_fl;
    const uint64_t* ht_key;
    const int* ht_val;
    unsigned ht_mask;
    const uint8_t* lm_bad;
    const int64_t* optr;
    int2* out;
};

// tracking.cpp:804-820 for live keyframe blockIdx.x; integer sums in a fixed order
__global__ void __launch_bounds__(kBlock) k_cull_redundancy(RedArgs a) {
    __shared__ int s_t[kWaves], s_r[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = blockIdx.x;
    const int64_t f0 = a.kt.f0[k];
    const int nf = a.kt.nf[k];
    int total = 0, red = 0;
    for (int i = tid; i < nf; i += kBlock) {
        const int64_t f = f0 + i;
        if (!(a.feat_fl[f] & 1)) continue;                                          // (:808)
        ++total;
        const int row = ht_get(a.ht_key, a.ht_val, a.ht_mask, a.feat_lm[f]);        // GetLandmark (:812)
        if (row < 0 || a.lm_bad[row] != 0) continue;                                // !lm || IsBad (:813)
        if (a.optr[row + 1] - a.optr[row] >= (int64_t)a.min_shared) ++red;          // (:816)
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        total += __shfl_xor(total, off);
        red += __shfl_xor(red, off);
    }
    if (lane == 0) {
        s_t[wave] = total;
        s_r[wave] = red;
    }
    __syncthreads();
    if (tid == 0) {
        int x = 0, y = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            x += s_t[w];
            y += s_r[w];
        }
        a.out[k] = make_int2(x, y);
    }
}

struct RmKfArgs {
    uint64_t kf_id;
    int64_t f0;
    int nf;
    int64_t nobs;           // observation rows (bound of the sort permutation)
    uint64_t* feat_lm;
    uint8_t* feat_fl;
    const uint64_t* ht_key;
    const int* ht_val;
    unsigned ht_mask;
    const uint8_t* lm_bad;
    const int64_t* optr;
    const uint64_t* okf;
    const int* perm;        // CSR entry -> observation row
    int* obs_lm;
    uint8_t* odead;
    int* hdr;               // hdr[2] = records written
    int2* out;              // {feature index, landmark row (~row: it held no observation of the keyframe)}
    int cap;
};

// Tracking::RemoveKeyFrame's feature loop (:758-770), one workgroup, the records in feature order
__global__ void __launch_bounds__(kKfBlock) k_cull_rmkf(RmKfArgs a) {
    __shared__ int s_cnt[kKfWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int n_out = 0;
    for (int base = 0; base < a.nf; base += kKfBlock) {
        const int i = base + tid;
        bool hit = false;
        int row = -1;
        int64_t at = -1;
        if (i < a.nf && (a.feat_fl[a.f0 + i] & 1)) {                                    // (:759)
            row = ht_get(a.ht_key, a.ht_val, a.ht_mask, a.feat_lm[a.f0 + i]);          // GetLandmark (:762)
            if (row >= 0 && a.lm_bad[row] != kLmRemoved) {
                hit = true;
                for (int64_t o = a.optr[row]; o < a.optr[row + 1]; ++o)
                    if (a.okf[o] == a.kf_id) {
                        at = o;
                        break;
                    }
            }
        }
        const uint64_t b = __ballot(hit);
        int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
        if (lane == 0) s_cnt[wave] = __popcll(b);
        __syncthreads();
        int all = 0;
#pragma unroll
        for (int w = 0; w < kKfWaves; ++w) {
            const int v = s_cnt[w];
            rank += w < wave ? v : 0;
            all += v;
        }
        __syncthreads();
        if (hit) {
            if (at >= 0) {  // Landmark::RemoveObservation (:766)
                const int64_t orow = a.perm[at];
                if (orow >= 0 && orow < a.nobs) a.obs_lm[orow] = kDeadObs;
                a.odead[at] = 1;
            }
            a.feat_lm[a.f0 + i] = 0;                                                    // (:767-769)
            a.feat_fl[a.f0 + i] = kResetFlags;
            if (n_out + rank < a.cap) a.out[n_out + rank] = make_int2(i, at >= 0 ? row : ~row);
        }
        n_out += all;
    }
    if (tid == 0) a.hdr[2] = n_out;
}

struct Prep {
    std::vector<int> rows;  // live keyframe rows, ascending id
    KfTable kt{};
};

// CSR and id table up to date (on the map context's stream, which c's then follows), the live keyframes'
// table uploaded and its geometry computed.  `skip_row`: a keyframe row left out (-1: none).
int prepare(vx_ctx* c, vx_dmap* m, int skip_row, bool geo, Prep& P) {
    auto& C = m->cull;
    int rc;
    if ((rc = dmap_build_csr(m->c, m))) return m->c == c ? rc : set_error(c, rc, "observation CSR: %s", vx_last_error(m->c));
    if ((rc = ht_sync(m->c, m))) return m->c == c ? rc : set_error(c, rc, "landmark id table: %s", vx_last_error(m->c));
    if (m->c != c && (rc = vx_stream_wait_ctx(c, m->c))) return rc;
    std::vector<std::pair<uint64_t, int>> live;
    live.reserve(m->kf_index.size());
    for (const auto& kv : m->kf_index)
        if (kv.second != skip_row) live.emplace_back(kv.first, kv.second);
    std::sort(live.begin(), live.end());
    const int n = (int)live.size();
    const size_t cap = (size_t)std::max(n, 1);
    const size_t o_id = 0, o_f0 = 8 * cap, o_row = 16 * cap, o_nf = 20 * cap, o_cam = 24 * cap, bytes = 28 * cap;
    VX_HIP(c, C.up_host.ensure(bytes, true));
    VX_HIP(c, C.kin.ensure(bytes));
    VX_HIP(c, C.geo.ensure(cap * 16 * sizeof(double)));
    uint8_t* H = static_cast<uint8_t*>(C.up_host.p);
    P.rows.resize(n);
    for (int i = 0; i < n; ++i) {
        const int k = live[i].second;
        P.rows[i] = k;
        reinterpret_cast<uint64_t*>(H + o_id)[i] = live[i].first;
        reinterpret_cast<int64_t*>(H + o_f0)[i] = m->kf_feat_ptr[k];
        reinterpret_cast<int*>(H + o_row)[i] = k;
        reinterpret_cast<int*>(H + o_nf)[i] = (int)(m->kf_feat_ptr[k + 1] - m->kf_feat_ptr[k]);
        reinterpret_cast<int*>(H + o_cam)[i] = m->kf_has_cam[k];
    }
    if (n) VX_HIP(c, hipMemcpyAsync(C.kin.p, H, bytes, hipMemcpyHostToDevice, c->stream));
    const uint8_t* D = C.kin.as<uint8_t>();
    P.kt.n = n;
    P.kt.id = reinterpret_cast<const uint64_t*>(D + o_id);
    P.kt.f0 = reinterpret_cast<const int64_t*>(D + o_f0);
    P.kt.row = reinterpret_cast<const int*>(D + o_row);
    P.kt.nf = reinterpret_cast<const int*>(D + o_nf);
    P.kt.cam = reinterpret_cast<const int*>(D + o_cam);
    P.kt.geo = C.geo.as<double>();
    if (geo && n) {
        hipLaunchKernelGGL(k_cull_kfgeo, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, n, P.kt.row,
                           (const double*)m->kf_pose.as<double>(), (const double*)m->kf_intr.as<double>(),
                           C.geo.as<double>());
        VX_LAUNCH_CHECK(c, "k_cull_kfgeo");
    }
    return VX_OK;
}

// pinned block: hdr (64 B) | landmark records | feature records | removed keyframe's records
struct HostLayout {
    size_t o_lm, o_ft, o_kf, bytes;
    int cap_lm, cap_ft, cap_kf;
};
HostLayout host_layout(const vx_dmap* m, int cap_kf) {
    HostLayout L;
    L.cap_lm = (int)std::max<int64_t>(m->n_lm, 1);
    L.cap_ft = (int)std::max<int64_t>(m->n_obs, 1);
    L.cap_kf = std::max(cap_kf, 1);
    L.o_lm = 64;
    L.o_ft = align64(L.o_lm + (size_t)L.cap_lm * sizeof(vx_cull_landmark));
    L.o_kf = align64(L.o_ft + (size_t)L.cap_ft * sizeof(vx_cull_feature));
    L.bytes = align64(L.o_kf + (size_t)L.cap_kf * sizeof(int2));
    return L;
}

// scan + prefix + apply enqueued on c's stream (the lists land in the pinned block)
int enqueue_landmarks(vx_ctx* c, vx_dmap* m, const vx_cull_options* o, const Prep& P, const HostLayout& L, bool dead) {
    auto& C = m->cull;
    const int64_t nl = m->n_lm;
    const int nb = (int)((nl + kBlock - 1) / kBlock);
    VX_HIP(c, C.reason.ensure((size_t)nl * 4));
    VX_HIP(c, C.cnt.ensure((size_t)nl * 4));
    VX_HIP(c, C.nreset.ensure((size_t)nl * 4));
    VX_HIP(c, C.mean.ensure((size_t)nl * 8));
    VX_HIP(c, C.blk_cnt.ensure((size_t)nb * sizeof(int2)));
    VX_HIP(c, C.blk_off.ensure((size_t)nb * sizeof(int2)));
    uint8_t* H = static_cast<uint8_t*>(C.host.p);
    ScanArgs a{};
    a.kt = P.kt;
    a.nl = nl;
    a.min_obs = o->min_landmark_observations;
    a.tau = o->landmark_max_reproj_error;
    a.optr = m->optr.as<int64_t>();
    a.okf = m->okf.as<uint64_t>();
    a.ofi = m->ofi.as<uint64_t>();
    a.odead = dead ? C.odead.as<uint8_t>() : nullptr;
    a.lm_id = m->lm_id.as<uint64_t>();
    a.lm_pos = m->lm_pos.as<double>();
    a.lm_bad = m->lm_bad.as<uint8_t>();
    a.feat_uv = m->feat_uv.as<double>();
    a.feat_lm = m->feat_lm.as<uint64_t>();
    a.feat_fl = m->feat_fl.as<uint8_t>();
    a.reason = C.reason.as<int>();
    a.cnt = C.cnt.as<int>();
    a.mean = C.mean.as<double>();
    a.nreset = C.nreset.as<int>();
    a.blk_cnt = C.blk_cnt.as<int2>();
    a.blk_off = C.blk_off.as<int2>();
    a.hdr = reinterpret_cast<int*>(H);
    a.out_lm = reinterpret_cast<vx_cull_landmark*>(H + L.o_lm);
    a.out_ft = reinterpret_cast<vx_cull_feature*>(H + L.o_ft);
    a.cap_lm = L.cap_lm;
    a.cap_ft = L.cap_ft;
    if (P.kt.n <= kLdsKf) hipLaunchKernelGGL(k_cull_scan<true>, dim3(nb), dim3(kBlock), 0, c->stream, a);
    else hipLaunchKernelGGL(k_cull_scan<false>, dim3(nb), dim3(kBlock), 0, c->stream, a);
    VX_LAUNCH_CHECK(c, "k_cull_scan");
    hipLaunchKernelGGL(k_cull_prefix, dim3(1), dim3(kBlock), 0, c->stream, (const int2*)a.blk_cnt, nb,
                       C.blk_off.as<int2>(), a.hdr);
    VX_LAUNCH_CHECK(c, "k_cull_prefix");
    hipLaunchKernelGGL(k_cull_apply, dim3(nb), dim3(kBlock), 0, c->stream, a);
    VX_LAUNCH_CHECK(c, "k_cull_apply");
    return VX_OK;
}

// the host mirrors after the lists arrived: what vx_dmap_set_features and vx_dmap_remove_landmarks
// leave for the same landmarks and features
int mirror_landmarks(vx_ctx* c, vx_dmap* m, const HostLayout& L) {
    auto& C = m->cull;
    const uint8_t* H = static_cast<const uint8_t*>(C.host.p);
    const int* hdr = reinterpret_cast<const int*>(H);
    const int n_lm = hdr[0], n_ft = hdr[1];
    if (n_lm < 0 || n_lm > L.cap_lm || n_ft < 0 || n_ft > L.cap_ft)
        return set_error(c, VX_ERR_STATE, "cull lists: %d landmarks / %d features outside the capacities %d / %d", n_lm,
                         n_ft, L.cap_lm, L.cap_ft);
    const size_t ft0 = C.feat.size();
    C.lm.resize(n_lm);
    C.feat.resize(ft0 + n_ft);
    if (n_lm) std::memcpy(C.lm.data(), H + L.o_lm, (size_t)n_lm * sizeof(vx_cull_landmark));
    if (n_ft) std::memcpy(C.feat.data() + ft0, H + L.o_ft, (size_t)n_ft * sizeof(vx_cull_feature));
    for (int i = 0; i < n_ft; ++i) {
        const vx_cull_feature& f = C.feat[ft0 + i];
        const int64_t g = m->kf_feat_ptr[f.kf_row] + f.feat_idx;
        m->kf_valid_cnt[f.kf_row] -= m->feat_flags[g] & 1;
        m->feat_flags[g] = kResetFlags;
    }
    for (int i = 0; i < n_lm; ++i) {
        const vx_cull_landmark& l = C.lm[i];
        m->n_obs_live -= m->lm_obs_live[l.row];
        m->lm_obs_live[l.row] = 0;
        m->lm_removed[l.row] = 1;
        m->lm_index.erase(l.lm_id);
    }
    m->n_lm_live -= n_lm;
    if (n_lm && (int64_t)m->obs_index.size() > 2 * m->n_obs_live + 4096)  // (as vx_dmap_remove_landmarks)
        for (auto it = m->obs_index.begin(); it != m->obs_index.end();)
            it = m->lm_removed[it->first.first] ? m->obs_index.erase(it) : std::next(it);
    return VX_OK;
}

int check_args(vx_ctx* c, const vx_dmap* m, const vx_cull_options* o, const char* who) {
    if (!m || !m->c || !o) return set_error(c, VX_ERR_INVALID, "%s: null argument", who);
    if (m->c->device != c->device) return set_error(c, VX_ERR_INVALID, "map and context on different devices");
    if (!(o->landmark_max_reproj_error == o->landmark_max_reproj_error) || !(o->kf_redundant_ratio == o->kf_redundant_ratio))
        return set_error(c, VX_ERR_INVALID, "%s: NaN option", who);
    return VX_OK;
}

int redundancy(vx_ctx* c, vx_dmap* m, const vx_cull_options* o, Prep& P, int skip_geo) {
    auto& C = m->cull;
    int rc;
    if ((rc = prepare(c, m, -1, !skip_geo, P))) return rc;
    const int n = P.kt.n;
    VX_HIP(c, C.red.ensure((size_t)std::max(n, 1) * sizeof(int2)));
    VX_HIP(c, C.red_host.ensure((size_t)std::max(n, 1) * sizeof(int2)));
    if (!n) return VX_OK;
    RedArgs a{};
    a.kt = P.kt;
    a.min_shared = o->kf_min_shared_observations;
    a.feat_lm = m->feat_lm.as<uint64_t>();
    a.feat_fl = m->feat_fl.as<uint8_t>();
    a.ht_key = m->ht_key.as<uint64_t>();
    a.ht_val = m->ht_val.as<int>();
    a.ht_mask = m->ht_cap - 1;
    a.lm_bad = m->lm_bad.as<uint8_t>();
    a.optr = m->optr.as<int64_t>();
    a.out = C.red.as<int2>();
    hipLaunchKernelGGL(k_cull_redundancy, dim3(n), dim3(kBlock), 0, c->stream, a);
    VX_LAUNCH_CHECK(c, "k_cull_redundancy");
    VX_HIP(c, hipMemcpyAsync(C.red_host.p, C.red.p, (size_t)n * sizeof(int2), hipMemcpyDeviceToHost, c->stream));
    VX_HIP(c, hipStreamSynchronize(c->stream));
    return VX_OK;
}

}  // namespace
}  // namespace vx

using namespace vx;

extern "C" {

void vx_cull_default_options(vx_cull_options* o) {
    if (!o) return;
    o->min_landmark_observations = 2;  // Tracking::Options (tracking.h:33-40)
    o->min_landmarks_for_culling = 200;
    o->min_keyframes_for_culling = 3;
    o->max_keyframes = 30;
    o->kf_min_shared_observations = 3;
    o->reserved = 0;
    o->kf_redundant_ratio = 0.9;
    o->landmark_max_reproj_error = 5.0;
}

int vx_cull_block(void) { return kBlock; }
int vx_cull_lds_keyframes(void) { return kLdsKf; }

int vx_dmap_cull_landmarks(vx_ctx* c, vx_dmap* m, const vx_cull_options* o, int* n_landmarks, int* n_features) {
    if (!c) return VX_ERR_INVALID;
    int rc;
    if ((rc = check_args(c, m, o, "vx_dmap_cull_landmarks"))) return rc;
    auto& C = m->cull;
    C.lm.clear();
    C.feat.clear();
    if (n_landmarks) *n_landmarks = 0;
    if (n_features) *n_features = 0;
    // LandmarkSize() < min_landmarks_for_culling (:656)
    if (m->n_lm_live < (int64_t)o->min_landmarks_for_culling || m->n_lm == 0) return VX_OK;
    VX_HIP(c, hipSetDevice(c->device));
    Prep P;
    if ((rc = prepare(c, m, -1, true, P))) return rc;
    const HostLayout L = host_layout(m, 1);
    VX_HIP(c, C.host.ensure(L.bytes));
    if ((rc = enqueue_landmarks(c, m, o, P, L, false))) return rc;
    VX_HIP(c, hipStreamSynchronize(c->stream));
    if ((rc = mirror_landmarks(c, m, L))) return rc;
    if (n_landmarks) *n_landmarks = (int)C.lm.size();
    if (n_features) *n_features = (int)C.feat.size();
    return VX_OK;
}

int vx_dmap_keyframe_redundancy(vx_ctx* c, vx_dmap* m, const vx_cull_options* o, int cap, uint64_t* kf_id,
                                int32_t* total, int32_t* redundant, int* n_out) {
    if (!c) return VX_ERR_INVALID;
    int rc;
    if ((rc = check_args(c, m, o, "vx_dmap_keyframe_redundancy"))) return rc;
    if (!n_out) return set_error(c, VX_ERR_INVALID, "vx_dmap_keyframe_redundancy: null count");
    VX_HIP(c, hipSetDevice(c->device));
    Prep P;
    if ((rc = redundancy(c, m, o, P, 1))) return rc;
    const int n = P.kt.n;
    *n_out = n;
    if (n > cap) return set_error(c, VX_ERR_CAPACITY, "need %d keyframes, cap %d", n, cap);
    const int2* r = static_cast<const int2*>(m->cull.red_host.p);
    for (int i = 0; i < n; ++i) {
        if (kf_id) kf_id[i] = m->kf_id[P.rows[i]];
        if (total) total[i] = r[i].x;
        if (redundant) redundant[i] = r[i].y;
    }
    return VX_OK;
}

int vx_dmap_cull_keyframes(vx_ctx* c, vx_dmap* m, const vx_cull_options* o, const uint64_t* protect_ids, int n_protect,
                           int* removed, uint64_t* removed_kf_id, double* ratio_out, int* n_landmarks,
                           int* n_features) {
    if (!c) return VX_ERR_INVALID;
    int rc;
    if ((rc = check_args(c, m, o, "vx_dmap_cull_keyframes"))) return rc;
    if (n_protect < 0 || (n_protect > 0 && !protect_ids))
        return set_error(c, VX_ERR_INVALID, "vx_dmap_cull_keyframes: bad protected ids");
    auto& C = m->cull;
    C.lm.clear();
    C.feat.clear();
    if (removed) *removed = 0;
    if (removed_kf_id) *removed_kf_id = 0;
    if (ratio_out) *ratio_out = 0.0;
    if (n_landmarks) *n_landmarks = 0;
    if (n_features) *n_features = 0;
    // keyframes.size() <= min_keyframes_for_culling (:781)
    if (m->n_kf_live <= (int64_t)o->min_keyframes_for_culling) return VX_OK;
    const bool exceeded = o->max_keyframes > 0 && m->n_kf_live > (int64_t)o->max_keyframes;  // (:785-787)
    VX_HIP(c, hipSetDevice(c->device));
    Prep P;
    if ((rc = redundancy(c, m, o, P, 1))) return rc;
    int pick = -1;
    double removed_ratio = 0.0;
    const int2* red = static_cast<const int2*>(C.red_host.p);
    for (int i = 0; i < P.kt.n && pick < 0; ++i) {
        const uint64_t id = m->kf_id[P.rows[i]];
        if (std::find(protect_ids, protect_ids + n_protect, id) != protect_ids + n_protect) continue;  // (:797-802)
        const int total = red[i].x, redundant = red[i].y;
        if (total == 0) continue;                                                                       // (:822)
        const double ratio = static_cast<double>(redundant) / static_cast<double>(total);              // (:826)
        if (ratio > o->kf_redundant_ratio && (exceeded || ratio > 0.95)) {                              // (:827)
            pick = i;
            removed_ratio = ratio;
        }
    }
    if (pick < 0) return VX_OK;
    const int k = P.rows[pick];
    const uint64_t kid = m->kf_id[k];
    const int64_t f0 = m->kf_feat_ptr[k];
    const int nf = (int)(m->kf_feat_ptr[k + 1] - f0);
    const HostLayout L = host_layout(m, nf);
    VX_HIP(c, C.host.ensure(L.bytes));
    VX_HIP(c, C.odead.ensure((size_t)std::max<int64_t>(m->n_obs, 1)));
    VX_HIP(c, hipMemsetAsync(C.odead.p, 0, (size_t)std::max<int64_t>(m->n_obs, 1), c->stream));
    uint8_t* H = static_cast<uint8_t*>(C.host.p);
    RmKfArgs a{};
    a.kf_id = kid;
    a.f0 = f0;
    a.nf = nf;
    a.nobs = m->n_obs;
    a.feat_lm = m->feat_lm.as<uint64_t>();
    a.feat_fl = m->feat_fl.as<uint8_t>();
    a.ht_key = m->ht_key.as<uint64_t>();
    a.ht_val = m->ht_val.as<int>();
    a.ht_mask = m->ht_cap - 1;
    a.lm_bad = m->lm_bad.as<uint8_t>();
    a.optr = m->optr.as<int64_t>();
    a.okf = m->okf.as<uint64_t>();
    a.perm = m->sort_vals2.as<int>();
    a.obs_lm = m->obs_lm.as<int>();
    a.odead = C.odead.as<uint8_t>();
    a.hdr = reinterpret_cast<int*>(H);
    a.out = reinterpret_cast<int2*>(H + L.o_kf);
    a.cap = L.cap_kf;
    hipLaunchKernelGGL(k_cull_rmkf, dim3(1), dim3(kKfBlock), 0, c->stream, a);
    VX_LAUNCH_CHECK(c, "k_cull_rmkf");
    // CullLandmarks once more (:838), under its own gate (:656; RemoveKeyFrame removes no landmark)
    const bool scan = m->n_lm_live >= (int64_t)o->min_landmarks_for_culling && m->n_lm > 0;
    Prep P2;
    if (scan) {
        // (the CSR and the id table are current: prepare only rebuilds the keyframe table, without k)
        if ((rc = prepare(c, m, k, true, P2))) return rc;
        if ((rc = enqueue_landmarks(c, m, o, P2, L, true))) return rc;
    }
    VX_HIP(c, hipStreamSynchronize(c->stream));
    // Tracking::RemoveKeyFrame's mirrors: vx_dmap_remove_observations + vx_dmap_set_features + vx_dmap_remove_keyframe
    const int* hdr = reinterpret_cast<const int*>(H);
    const int n_kf = hdr[2];
    if (n_kf < 0 || n_kf > L.cap_kf)
        return set_error(c, VX_ERR_STATE, "cull lists: %d features of the removed keyframe, capacity %d", n_kf, L.cap_kf);
    std::vector<int2> own(n_kf);
    if (n_kf) std::memcpy(own.data(), H + L.o_kf, (size_t)n_kf * sizeof(int2));
    bool tomb = false;
    for (const int2& r : own) {
        const int64_t g = f0 + r.x;
        m->kf_valid_cnt[k] -= m->feat_flags[g] & 1;
        m->feat_flags[g] = kResetFlags;
        if (r.y < 0) continue;
        auto it = m->obs_index.find(std::make_pair(r.y, kid));
        if (it == m->obs_index.end()) continue;  // (two features of the keyframe naming one landmark)
        m->obs_index.erase(it);
        --m->lm_obs_live[r.y];
        --m->n_obs_live;
        tomb = true;
    }
    if (tomb) m->csr_dirty = true;
    m->kf_alive[k] = 0;
    m->kf_index.erase(kid);
    --m->n_kf_live;
    if (scan && (rc = mirror_landmarks(c, m, L))) return rc;
    for (const int2& r : own) C.feat.push_back(vx_cull_feature{kid, k, r.x});
    if (removed) *removed = 1;
    if (removed_kf_id) *removed_kf_id = kid;
    if (ratio_out) *ratio_out = removed_ratio;
    if (n_landmarks) *n_landmarks = (int)C.lm.size();
    if (n_features) *n_features = (int)C.feat.size();
    return VX_OK;
}

int vx_dmap_cull_results(vx_dmap* m, int cap_lm, vx_cull_landmark* lm_records, int cap_feat,
                         vx_cull_feature* feat_records, int* n_lm, int* n_feat) {
    if (!m) return VX_ERR_INVALID;
    const auto& C = m->cull;
    const int nl = (int)C.lm.size(), nf = (int)C.feat.size();
    if (n_lm) *n_lm = nl;
    if (n_feat) *n_feat = nf;
    if ((lm_records && nl > cap_lm) || (feat_records && nf > cap_feat))
        return set_error(m->c, VX_ERR_CAPACITY, "need %d landmark / %d feature records, caps %d / %d", nl, nf, cap_lm,
                         cap_feat);
    if (lm_records && nl) std::memcpy(lm_records, C.lm.data(), (size_t)nl * sizeof(vx_cull_landmark));
    if (feat_records && nf) std::memcpy(feat_records, C.feat.data(), (size_t)nf * sizeof(vx_cull_feature));
    return VX_OK;
}

}  // extern "C"

static_assert(sizeof(vx_cull_options) == 40, "vx_cull_options layout (python CULL_OPTIONS_DTYPE)");
static_assert(sizeof(vx_cull_landmark) == 32, "vx_cull_landmark layout (python CULL_LANDMARK_DTYPE)");
static_assert(sizeof(vx_cull_feature) == 16, "vx_cull_feature layout (python CULL_FEATURE_DTYPE)");
