// reloc.hip — relocalisation: Tracking::TrackWithPnP (core/frontend/tracking.cpp:332-455) against the landmarks
// of up to 16 map keyframes as ONE correspondence set and ONE PnP (vx_relocalize_async / vx_relocalize_fetch).
// It is what HandleTrackingBad / HandleTrackingLost (tracking.cpp:477-499) leave as a TODO: both call
// map_->removeAll() and re-initialise.  The semantics are stated once, in include/vx_slam.h.
//
//   Match(kf_c, curr) for all c    k_knn_rows_batch + k_knn_compact_batch (match_batch_enqueue_to), unchanged
//   k_reloc_pairs   grid = candidates     candidate c = workgroup c: k_track_pairs' stages 1-6 on table entry c
//                                         (track_pairs_body.inc, as k_rig_pairs)
//   k_reloc_pool    one workgroup         the open candidates' pairs, one per current feature, into the
//                                         contiguous arrays PnP reads; the PnP problem record
//   pnp_enqueue(P = 1)                    unchanged kernels (ransac.hip)
//   k_reloc_final   one workgroup         the record: PnP result, status, per-candidate counts, best candidate
//
// so the launch count does not depend on the number of candidates, and the only synchronisation is the fetch's.
//
// k_reloc_pool.  Of all pairs that name one current feature the smallest match distance wins, then the lower
// candidate, then the lower pair index.  That is the unsigned minimum of the 64-bit key
//     distance bits (32) | candidate (4) | pair index (28)
// (a match distance is a non-negative float, whose bit pattern orders as an unsigned integer), kept per current
// feature in LDS and filled with 64-bit LDS minimum operations.  The minimum of a set does not depend on the
// order its members arrive in, so no atomic decides a position: after a barrier the concatenated pair list is
// compacted in order, in chunks of kBlock pairs with a running offset (trk::block_rank), a pair kept iff the
// table holds its key.  Keys are unique (candidate and pair index), so exactly one pair per claimed feature
// passes.  One workgroup: the table is the workgroup's LDS, and the compaction is ordered.  There are no
// spin-waits and no hand-offs between workgroups; kernel boundaries and workgroup barriers are the only
// synchronisation.
// The table is dynamic LDS sized by the current frame's capacity; the host takes its limit from the kernel's
// own static LDS use (hipFuncGetAttributes) against the 160 KiB of a CU: (163840 - 144) / 8 = 20462 rows.  A
// larger frame is refused (VX_ERR_CAPACITY); there is no global-memory second path.
// The pooled arrays, the provenance arrays and the mask go straight to their final places (the mask and the
// provenance arrays into the packed block the fetch copies: P = 1, so nothing has to be sliced afterwards).
//
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950; VGPRs / SGPRs / static LDS / scratch):
//   k_reloc_pairs 61 / 88 / 256 B / 0     k_reloc_pool 46 / 68 / 144 B (+ 8 B per row) / 0     k_reloc_final 16 / 30 / 128 B / 0
#include <algorithm>
#include <cstddef>
#include <cstring>

#include "vx_internal.hpp"
#include "dmap.hpp"
#include "track_bodies.hpp"

namespace vx {
namespace {

using trk::kBlock;
using trk::kWaves;

constexpr int kP = VX_MAX_RELOC_CANDIDATES;
constexpr int kPairBits = 28;                // the key's pair index field; 4 bits of candidate above it
constexpr size_t kCuLds = 160 * 1024;
static_assert(kP <= 16 && kP <= VX_MAX_MATCH_PAIRS && kP <= trk::kProbMax && kP <= kWaves, "candidate field / batch sizes");

// candidate = workgroup: k_track_pairs' stages on the candidate's own table entry
__global__ void __launch_bounds__(kBlock) k_reloc_pairs(const trk::TrackArgs* __restrict__ tab) {
    const trk::TrackArgs& a = tab[blockIdx.x];
#include "track_pairs_body.inc"
}

__device__ __forceinline__ unsigned long long pool_key(float distance, int cand, int pair) {
    return ((unsigned long long)__float_as_uint(distance) << 32) | ((unsigned long long)cand << kPairBits) |
           (unsigned long long)pair;
}

struct PoolArgs {
    int n_cand;
    const int* n_curr;       // the current frame's row count, clamped to cap_curr: the table's rows
    int cap_curr;
    int min_inliers;
    vx_pnp_options pnp;
    double intr[4];
    // the pooled problem and where each pair came from (cap_pool entries each)
    float* obj;
    float* img;
    uint8_t* pool_cand;
    int* pool_match;
    int* pool_train;
    uint8_t* mask;           // zeroed here, written by k_pnp_refine
    vx_reloc_result* res;    // n_pool
    vx_track_result* pool;   // the pool as TrackWithPnP's record: n_good_matches = the candidates' largest, n_pairs = n_pool
    int* offsets;            // 2
    double* intr_out;        // 4
    vx_pnp_options* opt_out;
};

// pair g of the concatenation: its candidate, pair index, match index, current feature and key
struct PoolPair {
    int cand, pair, match, train;
    unsigned long long key;
};
__device__ __forceinline__ PoolPair pool_pair(const trk::TrackArgs* __restrict__ tab, const int* s_off, int g) {
    PoolPair p;
    int c = 0;
    while (g >= s_off[c + 1]) ++c;  // (g < s_off[n_cand]; a closed candidate's range is empty)
    const trk::TrackArgs& t = tab[c];
    p.cand = c;
    p.pair = g - s_off[c];
    p.match = t.pair_match[p.pair];
    const vx_match m = t.matches[p.match];
    p.train = m.train_idx;
    p.key = pool_key(m.distance, c, p.pair);
    return p;
}

__global__ void __launch_bounds__(kBlock) k_reloc_pool(const trk::TrackArgs* __restrict__ tab, PoolArgs a) {
    extern __shared__ unsigned long long s_key[];  // one key per current feature
    __shared__ int s_cnt[kWaves];
    __shared__ int s_off[kP + 1];  // where candidate c's pairs begin in the concatenation
    const int tid = threadIdx.x;
    const int rows = min(max(*a.n_curr, 0), a.cap_curr);
    for (int i = tid; i < rows; i += kBlock) s_key[i] = ~0ull;
    if (tid == 0) {
        int o = 0;
        for (int c = 0; c < a.n_cand; ++c) {
            const vx_track_result* r = tab[c].res;
            s_off[c] = o;
            if (r->n_good_matches >= tab[c].min_matches) o += min(max(r->n_pairs, 0), tab[c].cap_matches);  // open (:357)
        }
        s_off[a.n_cand] = o;
    }
    __syncthreads();
    const int total = s_off[a.n_cand];
    // the table: per current feature the minimum key of the pairs that name it (order-free)
    for (int g = tid; g < total; g += kBlock) {
        const PoolPair p = pool_pair(tab, s_off, g);
        if ((unsigned)p.train < (unsigned)rows) atomicMin(&s_key[p.train], p.key);
    }
    __syncthreads();
    // the survivors, in concatenation order
    int n_pool = 0;
    for (int base = 0; base < total; base += kBlock) {
        const int g = base + tid;
        bool keep = false;
        PoolPair p{};
        if (g < total) {
            p = pool_pair(tab, s_off, g);
            keep = (unsigned)p.train < (unsigned)rows && s_key[p.train] == p.key;
        }
        int chunk;
        const int r = trk::block_rank(keep, s_cnt, &chunk);
        if (keep) {
            const trk::TrackArgs& t = tab[p.cand];
            const int k = n_pool + r;  // < min(rows, total): one survivor per claimed feature
            a.obj[3 * k] = t.obj[3 * p.pair];
            a.obj[3 * k + 1] = t.obj[3 * p.pair + 1];
            a.obj[3 * k + 2] = t.obj[3 * p.pair + 2];
            a.img[2 * k] = t.img[2 * p.pair];
            a.img[2 * k + 1] = t.img[2 * p.pair + 1];
            a.pool_cand[k] = (uint8_t)p.cand;
            a.pool_match[k] = p.match;
            a.pool_train[k] = p.train;
            a.mask[k] = 0;
        }
        n_pool += chunk;
    }
    if (tid == 0) {
        int n_good = tab[0].res->n_good_matches;  // (a candidate is open iff the largest count is: one min_matches)
        for (int c = 1; c < a.n_cand; ++c) n_good = max(n_good, tab[c].res->n_good_matches);
        a.pool->status = 0;
        a.pool->n_matches = 0;
        a.pool->n_good_matches = n_good;
        a.pool->n_pairs = n_pool;
        a.pool->n_bad_index = 0;
        a.pool->min_distance = 0.f;
        a.pool->parallax = 0.0;
        a.res->n_pool = n_pool;
        a.offsets[0] = 0;
        a.offsets[1] = n_pool >= a.min_inliers ? n_pool : 0;  // (:402) on the pool; no open candidate: n_pool = 0
        for (int k = 0; k < 4; ++k) a.intr_out[k] = a.intr[k];
        vx_pnp_options o = a.pnp;
        if (o.max_iterations < 0) o.max_iterations = min(100, 2 * n_pool);  // (:421)
        *a.opt_out = o;
    }
}

struct FinalArgs {
    int n_cand;
    int min_matches, min_inliers;
    const int* offsets;            // the pool's problem record: {0, n_pool} when PnP ran, {0, 0} otherwise
    const vx_track_result* pool;   // the pool as TrackWithPnP's record: k_reloc_pool's counts, k_pnp_refine's result
    const uint8_t* pool_cand;
    const uint8_t* mask;
    vx_reloc_result* res;          // n_pool is the pool kernel's
};

// wave c = candidate c: its survivors and its inliers counted over the pool (integer sums); then lane c of wave 0
// writes candidate c's entry, wave 1 the PnP record and thread 0 the head
__global__ void __launch_bounds__(kBlock) k_reloc_final(const trk::TrackArgs* __restrict__ tab, FinalArgs a) {
    __shared__ int s_kept[kP], s_inl[kP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_pool = a.res->n_pool;
    int kept = 0, inl = 0;
    if (wave < a.n_cand)
        for (int i = lane; i < n_pool; i += 64) {
            const bool mine = a.pool_cand[i] == wave;
            kept += mine ? 1 : 0;
            inl += mine && a.mask[i] ? 1 : 0;
        }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        kept += __shfl_xor(kept, off);
        inl += __shfl_xor(inl, off);
    }
    if (lane == 0 && wave < kP) {
        s_kept[wave] = kept;
        s_inl[wave] = inl;
    }
    __syncthreads();
    if (tid < kP) {  // candidate tid's entry; zeros from n_cand up
        const bool on = tid < a.n_cand;
        const vx_track_result* r = tab[on ? tid : 0].res;
        vx_reloc_candidate_result* e = &a.res->cand[tid];
        e->n_matches = on ? r->n_matches : 0;
        e->n_good_matches = on ? r->n_good_matches : 0;
        e->n_pairs = on ? r->n_pairs : 0;
        e->n_bad_index = on ? r->n_bad_index : 0;
        e->open = on && r->n_good_matches >= a.min_matches ? 1 : 0;
        e->n_kept = on ? s_kept[tid] : 0;
        e->n_inliers = on ? s_inl[tid] : 0;
        e->min_distance = on ? r->min_distance : 0.f;
        e->parallax = on ? r->parallax : 0.0;
    }
    // the PnP record, word by word: k_pnp_refine's when the problem ran, zeros otherwise
    const bool ran = a.offsets[1] > 0;
    if (tid >= 64 && tid < 64 + (int)(sizeof(vx_pnp_result) / 4))
        reinterpret_cast<uint32_t*>(&a.res->pnp)[tid - 64] = ran ? reinterpret_cast<const uint32_t*>(&a.pool->pnp)[tid - 64] : 0u;
    if (tid != 0) return;
    // TrackWithPnP's gates (:357, :402, :425, :441) on the pool's record (k_reloc_pool's counts, k_pnp_refine's result)
    const int status = trk::pnp_status(*a.pool, a.min_matches, a.min_inliers);
    int best = -1;
    double parallax = 0.0;
    if (status == VX_TRACK_OK) {
        best = 0;
        for (int c = 1; c < a.n_cand; ++c)
            if (s_inl[c] > s_inl[best]) best = c;  // ties: the lower index
        parallax = tab[best].res->parallax;
    }
    a.res->status = status;
    a.res->n_cand = a.n_cand;
    a.res->best_cand = best;
    a.res->parallax = parallax;
}

// the packed result block: vx_reloc_result | pool_cand[cap] | pool_match[cap] | pool_train[cap] | mask[cap],
// each part on a 16-byte boundary
struct Packed {
    int cap;
    size_t cand() const { return align16(sizeof(vx_reloc_result)); }
    size_t match() const { return cand() + align16((size_t)cap); }
    size_t train() const { return match() + align16((size_t)cap * 4); }
    size_t mask() const { return train() + align16((size_t)cap * 4); }
    size_t bytes() const { return mask() + align16((size_t)cap); }
};

// a running 256-byte aligned sub-allocation of one device buffer
struct Carve {
    size_t at = 0;
    size_t take(size_t bytes) {
        const size_t o = at;
        at += (bytes + 255) & ~(size_t)255;
        return o;
    }
};

// k_reloc_pool's table limit: the CU's LDS less the kernel's static use, in keys
int table_limit(vx_ctx* c, int* rows) {
    if (!c->rl_limit) {
        hipFuncAttributes fa{};
        VX_HIP(c, hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&k_reloc_pool)));
        int dev_max = 0;
        VX_HIP(c, hipDeviceGetAttribute(&dev_max, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device));
        const size_t lds = std::min((size_t)std::max(dev_max, 0), kCuLds);
        if (fa.sharedSizeBytes + 8 > lds) return set_error(c, VX_ERR_HIP, "k_reloc_pool: no LDS left for its table");
        c->rl_limit = (int)((lds - fa.sharedSizeBytes) / 8);
    }
    *rows = c->rl_limit;
    return VX_OK;
}

}  // namespace
}  // namespace vx

using namespace vx;

extern "C" {

int vx_relocalize_table_limit(vx_ctx* c, int32_t* rows) {
    if (!c) return VX_ERR_INVALID;
    if (!rows) return set_error(c, VX_ERR_INVALID, "vx_relocalize_table_limit: null argument");
    VX_HIP(c, hipSetDevice(c->device));
    int n = 0, rc;
    if ((rc = table_limit(c, &n))) return rc;
    *rows = n;
    return VX_OK;
}

int vx_relocalize_async(vx_ctx* c, vx_dmap* m, int n_cand, const vx_reloc_candidate* cands, const vx_frame* curr,
                        float ratio, const double* intr4, const vx_track_options* opt) {
    if (!c) return VX_ERR_INVALID;
    const char* call = "vx_relocalize_async";
    if (n_cand < 1 || n_cand > kP) return set_error(c, VX_ERR_INVALID, "%s: %d candidates outside [1, %d]", call, n_cand, kP);
    if (!m || !m->c || !cands || !curr || !curr->block.p || !intr4 || !opt)
        return set_error(c, VX_ERR_INVALID, "%s: null argument", call);
    if (m->c->device != c->device) return set_error(c, VX_ERR_INVALID, "%s: map and context on different devices", call);
    if (curr->device != c->device) return set_error(c, VX_ERR_INVALID, "%s: frame and context on different devices", call);
    int row[kP];
    for (int i = 0; i < n_cand; ++i) {
        const vx_frame* f = cands[i].frame;
        if (!f || !f->block.p) return set_error(c, VX_ERR_INVALID, "%s: candidate %d without a frame", call, i);
        if (f->device != c->device) return set_error(c, VX_ERR_INVALID, "%s: candidate %d: frame and context on different devices", call, i);
        const auto kf = m->kf_index.find(cands[i].kf_id);
        if (kf == m->kf_index.end())
            return set_error(c, VX_ERR_INVALID, "%s: candidate %d: keyframe %llu is not in the map", call, i,
                             (unsigned long long)cands[i].kf_id);
        for (int j = 0; j < i; ++j)
            if (cands[j].kf_id == cands[i].kf_id)
                return set_error(c, VX_ERR_INVALID, "%s: keyframe %llu named by candidates %d and %d", call,
                                 (unsigned long long)cands[i].kf_id, j, i);
        // the key's pair index field (a candidate has at most as many pairs as its frame has rows)
        if ((int64_t)f->cap >= ((int64_t)1 << kPairBits))
            return set_error(c, VX_ERR_CAPACITY, "%s: candidate %d: %d rows do not fit the key's pair index", call, i, f->cap);
        row[i] = kf->second;
    }
    int rc;
    if ((rc = trk::check_focal(c, call, intr4))) return rc;
    if ((rc = trk::check_pnp_options(c, call, opt->pnp))) return rc;
    VX_HIP(c, hipSetDevice(c->device));
    int limit = 0;
    if ((rc = table_limit(c, &limit))) return rc;
    if (curr->cap > limit)
        return set_error(c, VX_ERR_CAPACITY, "%s: current frame of %d rows, the LDS table holds %d", call, curr->cap, limit);
    // (a call refused above leaves the previous call's result in place)
    c->rl_valid = false;
    c->rl_n = 0;
    // as vx_track_pnp_async: the id table up to date on the map's stream, which this stream then follows
    if ((rc = ht_sync(m->c, m))) return set_error(c, rc, "landmark id table: %s", vx_last_error(m->c));
    if ((rc = vx_stream_wait_ctx(c, m->c))) return rc;

    // ---- capacities
    int cap[kP], pc[kP];
    int64_t seg[kP + 1];
    int q_cap = 1;
    seg[0] = 0;
    for (int i = 0; i < n_cand; ++i) {
        cap[i] = cands[i].frame->cap;
        pc[i] = std::max(cap[i], 1);
        seg[i + 1] = seg[i] + pc[i];
        q_cap = std::max(q_cap, cap[i]);
    }
    const int t_cap = std::max(curr->cap, 1);
    const int64_t slots = seg[n_cand];
    const int cap_pool = (int)std::min<int64_t>(slots, t_cap);  // one survivor per current feature at most
    const Packed pk{cap_pool};

    // ---- buffers
    Carve cm;  // rl_match
    const size_t o_best = cm.take((size_t)n_cand * q_cap * sizeof(unsigned));
    const size_t o_list = cm.take((size_t)n_cand * q_cap * sizeof(vx_match));
    const size_t o_count = cm.take(kP * 16);  // candidate i's count: int32[4] at i * 16
    Carve cw;  // rl_work
    const size_t o_good = cw.take((size_t)slots * sizeof(int));
    const size_t o_sega = cw.take((size_t)slots * 3 * sizeof(float));
    const size_t o_segb = cw.take((size_t)slots * 2 * sizeof(float));
    const size_t o_obj = cw.take((size_t)cap_pool * 3 * sizeof(float));
    const size_t o_img = cw.take((size_t)cap_pool * 2 * sizeof(float));
    const size_t o_prob = cw.take(trk::prob_bytes<trk::TrackArgs>());   // the candidates' own records (their options)
    const size_t o_prob1 = cw.take(trk::prob1_bytes<PoolArgs>());       // the pool's: what PnP reads
    const size_t o_res = cw.take(sizeof(vx_track_result));   // the pool's record; PnP writes its .pnp
    size_t o_tk[kP];
    for (int i = 0; i < n_cand; ++i) o_tk[i] = cw.take(trk::packed_bytes<vx_track_result>(pc[i]));
    VX_HIP(c, c->rl_match.ensure(cm.at));
    VX_HIP(c, c->rl_work.ensure(cw.at));
    VX_HIP(c, c->rl_out.ensure(pk.bytes()));
    uint8_t* dm = c->rl_match.as<uint8_t>();
    uint8_t* dw = c->rl_work.as<uint8_t>();
    uint8_t* dout = c->rl_out.as<uint8_t>();
    unsigned* best = reinterpret_cast<unsigned*>(dm + o_best);
    vx_match* list = reinterpret_cast<vx_match*>(dm + o_list);
    int32_t* count = reinterpret_cast<int32_t*>(dm + o_count);
    int* good = reinterpret_cast<int*>(dw + o_good);
    float* sega = reinterpret_cast<float*>(dw + o_sega);
    float* segb = reinterpret_cast<float*>(dw + o_segb);
    vx_track_result* pool_rec = reinterpret_cast<vx_track_result*>(dw + o_res);

    // ---- the argument table, staged and uploaded in one copy
    VX_HIP(c, c->rl_tab.begin(kP * sizeof(trk::TrackArgs)));
    trk::TrackArgs* tab = static_cast<trk::TrackArgs*>(c->rl_tab.host.p);
    std::memset(tab, 0, (size_t)n_cand * sizeof(trk::TrackArgs));
    const uint8_t *mq[kP], *mt[kP];
    const int *mnq[kP], *mnt[kP];
    for (int i = 0; i < n_cand; ++i) {
        const vx_frame* f = cands[i].frame;
        mq[i] = f->desc();
        mnq[i] = f->count();
        mt[i] = curr->desc();
        mnt[i] = curr->count();
        vx_ctx::RelocCand& h = c->rl_cand[i];
        h.list = list + (size_t)i * q_cap;
        h.count = count + 4 * i;
        h.cap = cap[i];
        trk::TrackArgs& a = tab[i];
        a.matches = h.list;
        a.n_matches = h.count;
        a.cap_matches = cap[i];
        a.curr_xy = reinterpret_cast<const uint8_t*>(&curr->kp()->x);
        a.stride = (int64_t)sizeof(vx_keypoint);
        a.n_curr = curr->count();
        trk::map_side(a, m, row[i]);
        trk::set_options(a, *opt, intr4);
        a.good = good + seg[i];
        a.obj = sega + 3 * seg[i];
        a.img = segb + 2 * seg[i];
        trk::packed_outputs(a, dw + o_tk[i], pc[i]);
        trk::prob_pointers(a, dw + o_prob, i);
    }
    VX_HIP(c, c->rl_tab.upload((size_t)n_cand * sizeof(trk::TrackArgs), c->stream));
    const trk::TrackArgs* dtab = c->rl_tab.dev.as<trk::TrackArgs>();

    // ---- Match(kf_c, curr) and the pair lists (:340-400), candidate = grid row / workgroup
    if ((rc = match_batch_enqueue_to(c, n_cand, mq, mnq, mt, mnt, q_cap, t_cap, ratio, best, list, count))) return rc;
    VX_HIP(c, launch(c, kStRelocPairs, k_reloc_pairs, dim3(n_cand), dim3(kBlock), 0, c->stream, dtab));
    // ---- the pool
    PoolArgs p{};
    p.n_cand = n_cand;
    p.n_curr = curr->count();
    p.cap_curr = curr->cap;
    p.min_inliers = opt->min_inliers;
    p.pnp = opt->pnp;
    for (int k = 0; k < 4; ++k) p.intr[k] = intr4[k];
    p.obj = reinterpret_cast<float*>(dw + o_obj);
    p.img = reinterpret_cast<float*>(dw + o_img);
    p.pool_cand = dout + pk.cand();
    p.pool_match = reinterpret_cast<int*>(dout + pk.match());
    p.pool_train = reinterpret_cast<int*>(dout + pk.train());
    p.mask = dout + pk.mask();
    p.res = reinterpret_cast<vx_reloc_result*>(dout);
    p.pool = pool_rec;
    trk::prob1_pointers(p, dw + o_prob1);
    static std::atomic<uint64_t> lds_done{0};
    VX_HIP(c, lds_attr_once(c->device, reinterpret_cast<const void*>(&k_reloc_pool), limit * 8, lds_done));
    const uint32_t table_bytes = (uint32_t)t_cap * 8;  // t_cap <= limit
    VX_HIP(c, launch(c, kStRelocPool, k_reloc_pool, dim3(1), dim3(kBlock), table_bytes, c->stream, dtab, p));
    // ---- one PnP on the pool (:414-423)
    PnpDeviceArgs pd{};
    pd.offsets = p.offsets;
    pd.intr = p.intr_out;
    pd.opt = p.opt_out;
    pd.obj = p.obj;
    pd.img = p.img;
    pd.out = &pool_rec->pnp;
    pd.mask = p.mask;
    if ((rc = pnp_enqueue(c, 1, trk::pnp_hyp_bound(opt->pnp), pd, c->rl_hyp))) return rc;
    // ---- the record
    FinalArgs f{};
    f.n_cand = n_cand;
    f.min_matches = opt->min_matches;
    f.min_inliers = opt->min_inliers;
    f.offsets = p.offsets;
    f.pool = pool_rec;
    f.pool_cand = p.pool_cand;
    f.mask = p.mask;
    f.res = p.res;
    VX_HIP(c, launch(c, kStRelocFinal, k_reloc_final, dim3(1), dim3(kBlock), 0, c->stream, dtab, f));
    c->rl_n = n_cand;
    c->rl_cap = cap_pool;
    c->rl_valid = true;
    return VX_OK;
}

int vx_relocalize_fetch(vx_ctx* c, vx_reloc_result* out, uint8_t* pool_cand, int32_t* pool_match, int32_t* pool_train,
                        uint8_t* mask, int cap_pool) {
    if (!c || !out) return c ? set_error(c, VX_ERR_INVALID, "vx_relocalize_fetch: null result") : VX_ERR_INVALID;
    if (!c->rl_valid) return set_error(c, VX_ERR_STATE, "no vx_relocalize_async enqueued");
    VX_HIP(c, hipSetDevice(c->device));
    const Packed pk{c->rl_cap};
    VX_HIP(c, c->rl_host.ensure(pk.bytes()));
    VX_HIP(c, hipMemcpyAsync(c->rl_host.p, c->rl_out.p, pk.bytes(), hipMemcpyDeviceToHost, c->stream));
    VX_HIP(c, hipStreamSynchronize(c->stream));
    if (c->prof) prof_collect(c);
    const uint8_t* h = static_cast<const uint8_t*>(c->rl_host.p);
    std::memcpy(out, h, sizeof *out);
    const int np = std::min(std::max(out->n_pool, 0), c->rl_cap);
    if ((pool_cand || pool_match || pool_train || mask) && np > cap_pool)
        return set_error(c, VX_ERR_CAPACITY, "need %d pooled pairs, cap %d", np, cap_pool);
    if (pool_cand && np) std::memcpy(pool_cand, h + pk.cand(), (size_t)np);
    if (pool_match && np) std::memcpy(pool_match, h + pk.match(), (size_t)np * 4);
    if (pool_train && np) std::memcpy(pool_train, h + pk.train(), (size_t)np * 4);
    if (mask && np) std::memcpy(mask, h + pk.mask(), (size_t)np);
    return VX_OK;
}

int vx_relocalize_matches(vx_ctx* c, int cand, const vx_match** d_matches, const int32_t** d_n, int32_t* cap) {
    if (!c) return VX_ERR_INVALID;
    if (!c->rl_valid) return set_error(c, VX_ERR_STATE, "no vx_relocalize_async enqueued");
    if (cand < 0 || cand >= c->rl_n)
        return set_error(c, VX_ERR_INVALID, "vx_relocalize_matches: candidate %d outside [0, %d)", cand, c->rl_n);
    const vx_ctx::RelocCand& k = c->rl_cand[cand];
    if (d_matches) *d_matches = k.list;
    if (d_n) *d_n = k.count;
    if (cap) *cap = k.cap;
    return VX_OK;
}

}  // extern "C"

static_assert(sizeof(vx_reloc_candidate) == 16, "vx_reloc_candidate layout (python RELOC_CANDIDATE_DTYPE)");
static_assert(sizeof(vx_reloc_candidate_result) == 40, "vx_reloc_candidate_result layout (python RELOC_CANDIDATE_RESULT_DTYPE)");
static_assert(sizeof(vx_reloc_result) == 808 && offsetof(vx_reloc_result, pnp) == 24 && offsetof(vx_reloc_result, cand) == 168,
              "vx_reloc_result layout (python RELOC_RESULT_DTYPE)");
