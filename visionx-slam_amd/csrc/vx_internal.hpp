// vx_internal.hpp — context, device buffers, error plumbing and stage profiling shared by the
// ORB, matching and bundle-adjustment translation units of libvxslam.so.
#pragma once

#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <string>
#include <vector>

#include "vx_slam.h"

#ifndef VX_NO_RCCL
#include <rccl/rccl.h>
#endif

namespace vx {

// $VX_PLAN_TIMING: host timestamps of a plan build's stages on stderr (ms since the build began)
struct PlanClock {
    bool on = std::getenv("VX_PLAN_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void mark(const char* what) const {
        if (on)
            std::fprintf(stderr, "[vx plan] %-28s %.3f ms\n", what,
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
};

constexpr int kMaxLevels = 12;

// Profiling stages (vx_prof_*).
enum Stage : int {
    kStGray = 0,
    kStResize,
    kStFast,
    kStSelect,
    kStBlur,          // (unused: the blur is computed inside k_fast)
    kStDescribe,
    kStMatchPartial,
    kStMatchMerge,
    kStBaReset,
    kStBaPose,
    kStBaPoseSum,
    kStBaAllreduce,
    kStBaSolve,
    kStBaLandmark,
    kStPyramid,
    kStSbaLandmark,
    kStSbaBlocks,
    kStSbaSolve,
    kStSbaUpdate,
    kStSbaAllreduce,
    kStLmDepth,
    kStLmTriangulate,
    kStLmCompact,
    kStPnpHyp,
    kStPnpRefine,
    kStEmHyp,
    kStEmSelect,
    kStBaIter,        // fused LocalBA iteration (k_ba_iter)
    kStBaPrologue,    // iteration 0's pose stage of the fused path
    kStBaWin,         // the whole LocalBA window in one persistent launch (k_ba_win)
    kStTrackPairs,    // TrackWithPnP's filter + pair gather (k_track_pairs)
    kStKfFeat,        // CreateKeyFrame on the resident map: feature rows + depth (k_kf_feat)
    kStKfMatch,       // its triangulation gate per match (k_kf_match)
    kStKfCommit,      // its ordered compactions and the map edit (k_kf_commit)
    kStTrackEPairs,   // TrackLastFrame's filter + 2D-2D pair gather (k_track_epairs)
    kStTrackEPose,    // its T_cl * T_lw (k_track_epose)
    kStInitSums,      // InitWithFirstFrame's gray sum / sum of squares (k_init_sums)
    kStInitGate,      // its occupancy grid, meanStdDev and gates (k_init_gate)
    kStFrameCapture,  // a slot's rows into a device-resident frame (k_frame_capture)
    kStTrackGate,     // Track()'s PnP -> essential fallback decision (k_track_gate)
    kStTrackFinal,    // its result head and packed block (k_track_final)
    kStRigPairs,      // Track() for a rig: k_track_pairs' stages, camera = workgroup (k_rig_pairs)
    kStRigPack,       // the cameras' pair segments into the contiguous RANSAC arrays (k_rig_pack)
    kStRigGate,       // the fallback decision per camera (k_rig_gate)
    kStRigEPairs,     // k_track_epairs' stages, camera = workgroup (k_rig_epairs)
    kStRigEPose,      // T_cl * T_lw per camera (k_rig_epose)
    kStRigFinal,      // the cameras' heads and packed blocks (k_rig_final)
    kStFrameCaptureBatch,  // a batch bank's frames into resident frames (k_frame_capture_batch)
    kStRigKfFeat,     // CreateKeyFrame for a rig: feature rows + depth, camera = grid row (k_rig_kf_feat)
    kStRigKfMatch,    // its triangulation gate per match (k_rig_kf_match)
    kStRigKfCount,    // the cameras' landmark counts (k_rig_kf_count)
    kStRigKfCommit,   // the cameras' ordered compactions and the map edit (k_rig_kf_commit)
    kStRelocPairs,    // relocalisation: k_track_pairs' stages, candidate = workgroup (k_reloc_pairs)
    kStRelocPool,     // the candidates' pairs pooled, one per current feature (k_reloc_pool)
    kStRelocFinal,    // the record: status, per-candidate counts, best candidate (k_reloc_final)
    kStCount
};

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    // grow-only; returns hipSuccess or the allocation error
    hipError_t ensure(size_t want) {
        if (want <= bytes) return hipSuccess;
        release();
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) bytes = want;
        return e;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
};

struct PinnedBuf {
    void* p = nullptr;
    size_t bytes = 0;
    ~PinnedBuf() {
        if (p) (void)hipHostFree(p);
    }
    // cached = true: host-cached (non-coherent) pages for a staging block the CPU fills with many
    // scattered writes; the default (coherent) pages are uncached on the host side
    hipError_t ensure(size_t want, bool cached = false) {
        if (want <= bytes) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
        hipError_t e = hipHostMalloc(&p, want, cached ? hipHostMallocNonCoherent : hipHostMallocDefault);
        if (e == hipSuccess) bytes = want;
        return e;
    }
};

inline size_t align64(size_t x) { return (x + 63) & ~(size_t)63; }
__host__ __device__ inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }  // (kernels use it too)

// A host block staged in pinned memory and uploaded into a device block of its own in one copy, the
// staging guarded by an event: begin() waits until the previous upload has left the staging (the one
// place an entry that uses it can block) or creates the event, and ensures both blocks; the caller
// fills host.p; upload() copies and records the event.
struct StagedUpload {
    PinnedBuf host;
    DevBuf dev;
    hipEvent_t event = nullptr;
    ~StagedUpload() {
        if (event) (void)hipEventDestroy(event);
    }
    hipError_t begin(size_t bytes) {
        hipError_t e = event ? hipEventSynchronize(event) : hipEventCreateWithFlags(&event, hipEventDisableTiming);
        if (e == hipSuccess) e = host.ensure(bytes);
        if (e == hipSuccess) e = dev.ensure(bytes);
        return e;
    }
    hipError_t upload(size_t bytes, hipStream_t stream) {
        const hipError_t e = hipMemcpyAsync(dev.p, host.p, bytes, hipMemcpyHostToDevice, stream);
        return e == hipSuccess ? hipEventRecord(event, stream) : e;
    }
};

// Track()'s packed block (track_frame.hip, track_rig.hip) by its three capacities.  Declared here because
// the context holds them by value; the members, the one statement of the layout, are in track_bodies.hpp.
namespace trk {
struct FrameBlock {
    int cap0 = 0, cap1 = 0, cap_kp = 0;  // pair capacities of the two paths, keypoint rows
    size_t pm(int which) const;          // offset of pair_match0 / pair_match1
    size_t mask(int which) const;        // ... of mask0 / mask1
    size_t kp() const;                   // ... of the keypoint rows
    size_t bytes(bool with_keypoints) const;
};
}  // namespace trk

// Host-computed geometry of one ORB configuration (image size + params).  Mirrors the layer
// layout of ORB_Impl::detectAndCompute (levels stored unpadded, back to back).
struct OrbGeometry {
    int W = 0, H = 0;
    vx_orb_params p{};
    int L = 0;
    int lw[kMaxLevels], lh[kMaxLevels];
    int64_t off[kMaxLevels];        // byte offset of level l in the pyramid buffer
    float scale[kMaxLevels], inv_scale[kMaxLevels];
    int quota[kMaxLevels];
    int64_t pyr_bytes = 0;
    // resize tables for levels 1..L-1: int4 {ofs, c0, c1, 0} per destination column / row
    int64_t xtab[kMaxLevels], ytab[kMaxLevels];
    int64_t tab_entries = 0;
    // fused pyramid (k_pyramid): level-0 tiles, per (tile column | tile row, level) int4
    // {need_lo, need_hi, own_lo, own_hi} at tabs[pr_x] / tabs[pr_y], LDS bytes per ping-pong buffer
    bool pyr_fused = false;
    int pr_ntx = 0, pr_nty = 0;
    int pr_tile = 64, pr_block = 1024;
    int64_t pr_x = 0, pr_y = 0;
    int pr_buf = 0;
    int pr_area0 = 0;               // max level-0 need area (pixels)
    int pr_w0 = 0, pr_h0 = 0;       // max level-0 need width / height
    int pr_tabn = 0;                // max packed coefficient entries per tile
    int n_cu = 256;                 // compute units of the device (batched pyramid choice)
    // FAST tiles (64 x 16 pixels per workgroup) and output cells (row x tile column)
    int ntx[kMaxLevels], nty[kMaxLevels];
    int tile_base[kMaxLevels];     // first tile (workgroup) of level l
    int total_tiles = 0;
    int64_t cell_base[kMaxLevels]; // first cell of level l
    int64_t cells_total = 0;
    int level_cap[kMaxLevels];     // max strict-NMS corners of level l
    int64_t stage_base[kMaxLevels];// selection staging (4 * level_cap + 4 records) of level l
    int64_t stage_total = 0;
    int max_w = 0;
    int out_cap = 0;               // keypoint capacity of one slot
};

struct Slot {
    DevBuf kp, desc, count;  // vx_keypoint[cap], uint8[cap*32], int32[4] {n, overflow, ..}
    int cap = 0;
    bool valid = false;
};

struct ProfEvent {
    hipEvent_t a, b;
    int stage;
};

// Launch sequences of the async entry points captured into hipGraphs and replayed with one
// hipGraphLaunch (the per-frame pipeline is otherwise bound by host-side launch cost: ~18 kernel
// launches per frame).  Keyed by everything the captured sequence bakes in (device pointers,
// sizes, a geometry / plan serial); least-recently-used entries are evicted.
struct GraphCache {
    struct Entry {
        std::vector<uint64_t> key;
        hipGraphExec_t exec = nullptr;
        uint64_t last = 0;
    };
    std::vector<Entry> entries;
    uint64_t tick = 0;
    int captured = 0, launched = 0;
};

}  // namespace vx

struct vx_ba_plan;

// a frame's features on the device (frame.hip): count[4] | vx_keypoint[cap] | uint8[cap * 32]
struct vx_frame {
    int device = 0;
    int cap = 0;
    vx::DevBuf block;
    size_t off_kp = 16, off_desc = 0, bytes = 0;
    int32_t* count() const { return block.as<int32_t>(); }
    vx_keypoint* kp() const { return reinterpret_cast<vx_keypoint*>(block.as<uint8_t>() + off_kp); }
    uint8_t* desc() const { return block.as<uint8_t>() + off_desc; }
};

struct vx_event {
    int device = 0;
    hipEvent_t ev = nullptr;
};

struct vx_ctx {
    int device = 0;
    int n_cus = 0;  // compute units of the device (lazily queried)
    float grid_share = 1.0f;  // vx_set_grid_share: CUs the single-round grids (k_pyramid) size for
    hipStream_t stream = nullptr;
    hipEvent_t order_event = nullptr;  // vx_stream_wait_ctx: recorded on this stream
    std::string err;

    // ---- ORB
    vx::OrbGeometry geo;
    bool geo_valid = false;
    int kp_order = VX_ORDER_STL;  // vx_orb_set_order: keypoint order inside a level
    int orb_debug = 0;            // vx_orb_set_debug flags (test hooks)
    int scratch_slot = -1;        // slot whose single-frame extraction last wrote the shared ORB scratch
                                  // (pyramid, blur, candidates, stages); -1 after a batch
    vx::DevBuf orb_dbg;           // their device record (k_select_stl)
    vx::DevBuf img_in, pyr, blur, tabs, cand, band_count, hist, stage, level_count;
    vx::Slot slots[VX_MAX_SLOTS];
    vx::Slot batch[VX_BATCH_BANKS];  // vx_orb_extract_batch_async outputs, frame-major
    int batch_n[VX_BATCH_BANKS] = {0};

    // ---- matching
    vx::DevBuf mq, mt, mq_n, partial, matches, match_count;
    vx::PinnedBuf host_stage;
    int match_cap = 0;
    bool match_valid = false;
    vx::DevBuf mb_best, mb_matches, mb_count;  // vx_match_batch_async: per-pair results
    vx::DevBuf mb_in;                           // vx_match_knn2_ratio_batch: uploaded rows + counts
    vx::PinnedBuf mb_host;
    int mb_valid = 0, mb_cap = 0;

    // ---- landmark creation (landmarks.hip): inputs, per-item flags / points, compacted outputs
    vx::DevBuf lm_in0, lm_in1, lm_in2, lm_in3, lm_in4, lm_depth, lm_valid, lm_pw, lm_index, lm_out, lm_count, lm_aux;

    // ---- PnP RANSAC (ransac.hip): packed inputs (pinned staging + device), hypothesis records,
    // packed outputs (results + inlier mask)
    vx::PinnedBuf rs_host, rs_host_out;
    vx::DevBuf rs_in, rs_hyp, rs_out;  // (shared by vx_essential_ransac, essential.hip)

    // ---- TrackWithPnP on the device (track.hip): buffers of its own, so the RANSAC entry points
    // above may run between vx_track_pnp_async and its fetch
    vx::DevBuf tk_good, tk_obj, tk_img, tk_prob, tk_hyp, tk_out;  // kept-match list, pairs, PnP record, packed result
    vx::PinnedBuf tk_host;
    vx::StagedUpload tk_in;      // vx_track_pnp_host_async: descriptors + positions staged for one upload
    int tk_cap = 0;              // match capacity of the enqueued call (sizes the packed result)
    int tk_min_matches = 0, tk_min_inliers = 0;
    bool tk_valid = false;

    // ---- TrackLastFrame on the device (track_ess.hip): buffers of its own again, so a PnP track, an
    // essential track and the RANSAC entry points may all be in flight together
    vx::DevBuf te_good, te_p1, te_p2, te_prob, te_hyp, te_out;  // kept-match list, pairs, essential record, packed result
    vx::PinnedBuf te_host;
    vx::StagedUpload te_in;      // vx_track_essential_host_async: descriptors + positions staged for one upload
    int te_cap = 0;              // match capacity of the enqueued call (sizes the packed result)
    int te_min_matches = 0, te_min_inliers = 0;
    bool te_valid = false;

    // ---- InitWithFirstFrame's gates on the device (init_gate.hip)
    vx::DevBuf ig_part, ig_out;  // per-workgroup {sum, sum_sq} slots, the result record
    vx::PinnedBuf ig_host;       // the fetched record
    vx::StagedUpload ig_in;      // vx_init_gate_host_async: count + positions + image rows staged for one upload
    bool ig_valid = false;

    // ---- device-resident frames (frame.hip): the pinned staging of vx_frame_extract_host_async (image
    // rows) and vx_frame_upload_async (the frame block), and the pinned block vx_frame_fetch copies into
    vx::PinnedBuf fr_in_host, fr_host;
    hipEvent_t fr_in_event = nullptr;  // (recorded after the upload: the staging is reused once it has passed)

    // ---- Tracking::Track() on the device (track_frame.hip): both match lists, the gate record, the
    // packed result (device + pinned); the pair / RANSAC scratch is tk_* and te_*
    vx::DevBuf tf_matches[2], tf_count, tf_gate, tf_out;  // tf_count: int32[8], list i's count at [4 * i]
    vx::PinnedBuf tf_host;
    int tf_cap[2] = {0, 0};      // match capacities of the enqueued call (0: that match was not enqueued)
    vx::trk::FrameBlock tf_blk;  // the packed block's pair capacities and keypoint rows
    bool tf_list1_own = true;    // false: list 1 is list 0's rows under a gated count (last_kf == last)
    bool tf_valid = false, tf_fetched = false;

    // ---- Track() for a rig (track_rig.hip): buffers of its own throughout, so a single-camera track
    // (tk_*, te_*, tf_*) may be in flight on the same context
    vx::StagedUpload tr_tab;     // the per-camera argument table, staged for one upload
    vx::DevBuf tr_match;         // match scratch, both lists of every camera, their counts, the gate records
    vx::DevBuf tr_zero;          // int32[4] of zeros: the query count of a camera without a last keyframe (never written)
    vx::DevBuf tr_work;          // kept-match lists, pair segments, contiguous RANSAC arrays + masks, problem
                                 // records, RANSAC results, the cameras' packed PnP / essential blocks
    vx::DevBuf tr_hyp[2];        // hypothesis scratch of the two RANSACs
    vx::DevBuf tr_out;           // the packed result, camera blocks at vx_track_rig_layout's offsets
    vx::PinnedBuf tr_host;
    struct RigCam {
        int cap[2] = {0, 0};       // match capacities (0: list 0 not enqueued: no last keyframe)
        vx::trk::FrameBlock blk;   // the camera's block: pair capacities of the two paths, keypoint rows
        const vx_match* list[2] = {nullptr, nullptr};
        const int32_t* count[2] = {nullptr, nullptr};
        int64_t offset = 0;        // of the camera's block in tr_out / tr_host
    } tr_cam[VX_MAX_RIG_CAMERAS];
    int tr_n = 0;                // cameras of the enqueued call
    int64_t tr_bytes = 0;        // of the packed result
    bool tr_valid = false, tr_fetched = false, tr_fetched_kp = false;

    // ---- relocalisation (reloc.hip): buffers of its own throughout, so any track, match or RANSAC call may be
    // in flight on the same context
    vx::StagedUpload rl_tab;     // the per-candidate argument table, staged for one upload
    vx::DevBuf rl_match;         // match scratch, every candidate's list and count
    vx::DevBuf rl_work;          // kept-match lists, pair segments, the candidates' packed PnP blocks and problem
                                 // records, the pooled arrays, the pool's problem record, the PnP result
    vx::DevBuf rl_hyp;           // hypothesis scratch
    vx::DevBuf rl_out;           // the packed result: record | pool_cand | pool_match | pool_train | mask
    vx::PinnedBuf rl_host;
    struct RelocCand {
        const vx_match* list = nullptr;
        const int32_t* count = nullptr;
        int cap = 0;
    } rl_cand[VX_MAX_RELOC_CANDIDATES];
    int rl_n = 0;                // candidates of the enqueued call
    int rl_cap = 0;              // pool capacity of the enqueued call (sizes the packed result)
    int rl_limit = 0;            // k_reloc_pool's LDS table limit on this device (0: not asked yet)
    bool rl_valid = false;

    // ---- device-side LocalBA plan build scratch (ba_window.hip)
    struct PlanScratch {
        vx::DevBuf wptr, wlm, wfl, cam, wid, wuv, lid, bad, optr, okf, ofi, pos, hkey, hval, f_lm, f_pv, f_first,
            l_ref, l_opt, l_slot, l_first, counts, scan_a, scan_b, scan_c, inv, cnt, tmp;
        vx::DevBuf fb, fb_groups, fb_tmp;  // device build of the fused layout (ba_fused_build.hip)
        vx::PinnedBuf fb_host;             // its two small read-backs
        vx::PinnedBuf rb_host, up_host;    // build_core's read-back and its table uploads
        vx::PinnedBuf win_host;            // the resident-map build's window tables, one upload ...
        vx::DevBuf win;                    // ... into one device block
    } plan_scratch;
    vx_dmap* snap_map = nullptr;  // vx_ba_optimize_map's scratch map: the view loaded for the lean build (ba_lean.hip)
    // LocalBA plans of this context: parked buffer sets of destroyed plans (adopted by the next
    // vx_ba_plan_create) and the live plans (detached when the context goes first)
    std::vector<vx_ba_plan*> plan_husks, plan_live;

    // ---- hipGraph replay of the async entry points ($VX_GRAPHS=0 disables)
    vx::GraphCache graphs;
    bool use_graphs = true;
    uint64_t geo_gen = 0;  // bumped whenever the ORB geometry (and its buffers) is rebuilt

    // ---- profiling
    bool prof = false;
    uint64_t prof_mask = 0;
    std::vector<vx::ProfEvent> pending;
    std::vector<hipEvent_t> event_pool;
    double prof_ms[vx::kStCount] = {0};
    int64_t prof_n[vx::kStCount] = {0};

    // ---- multi-GPU
#ifndef VX_NO_RCCL
    ncclComm_t comm = nullptr;
#endif
    int nranks = 1, rank = 0;
};

namespace vx {

int set_error(vx_ctx* c, int code, const char* fmt, ...);
// frees the parked plan buffers and detaches the live plans of c (vx_destroy; ba.hip)
void plan_pool_release(vx_ctx* c);
int hip_fail(vx_ctx* c, hipError_t e, const char* what);

// Event bracket around launches of one stage (no-op when profiling is off).
struct ProfScope {
    vx_ctx* c;
    int stage;
    hipStream_t s;
    hipEvent_t a = nullptr;
    ProfScope(vx_ctx* c_, int st, hipStream_t on = nullptr);  // default: the context stream
    ~ProfScope();
};
void prof_collect(vx_ctx* c);

// Per-dispatch timing for a single-kernel stage: the events handed to hipExtLaunchKernelGGL carry
// the dispatch's own start / end timestamps (the duration rocprofv3 reports), not a bracket that
// also spans the stream's dispatch boundaries.  Both null when the stage is not being profiled.
struct KTiming {
    hipEvent_t a = nullptr, b = nullptr;
};
KTiming prof_kernel_events(vx_ctx* c, int stage);
void prof_kernel_done(vx_ctx* c, int stage, KTiming t);

template <class F, class... Args>
inline hipError_t launch(vx_ctx* c, int stage, F kernel, dim3 grid, dim3 block, uint32_t shm, hipStream_t s,
                         Args... args) {
    const KTiming t = prof_kernel_events(c, stage);
    if (t.a) {
        hipExtLaunchKernelGGL(kernel, grid, block, shm, s, t.a, t.b, 0, args...);
        prof_kernel_done(c, stage, t);
    } else {
        hipLaunchKernelGGL(kernel, grid, block, shm, s, args...);
    }
    return hipGetLastError();
}

int orb_prepare(vx_ctx* c, const vx_orb_params* p, int w, int h);

// kNN-2 + ratio matching of device descriptor sets (match.hip) into a caller's list: `out` holds
// q_cap vx_match rows, out_count one int32; c->partial is the only context buffer it uses.  Enqueued
// on c->stream, nothing synchronised.  vx_match_* pass the context's own list (c->matches).
int match_enqueue_to(vx_ctx* c, const uint8_t* dq, const int* dnq, int nq_host, const uint8_t* dt, const int* dnt,
                     int nt_host, int q_cap, int t_cap, float ratio, vx_match* out, int* out_count);
// The batched form (k_knn_rows_batch + k_knn_compact_batch: pair = grid y / workgroup) into a caller's
// buffers: n_pairs in [1, VX_MAX_MATCH_PAIRS] pairs under ONE q_cap / t_cap (every pair's device
// counts are clamped to them); `best` holds n_pairs * q_cap keys of scratch, pair p's matches go to
// out + p * q_cap and its count to out_count[4 p].  No context buffer is used.  Per pair the list is
// match_enqueue_to's, byte for byte.  vx_match_batch_async passes the context's own buffers (c->mb_*).
int match_batch_enqueue_to(vx_ctx* c, int n_pairs, const uint8_t* const* dq, const int* const* dnq,
                           const uint8_t* const* dt, const int* const* dnt, int q_cap, int t_cap, float ratio,
                           unsigned* best, vx_match* out, int* out_count);

// PnP RANSAC on problems already in device memory (ransac.hip): k_pnp_hyp over (hmax, P) and
// k_pnp_refine over P enqueued on c->stream, nothing synchronised.  Problem p owns correspondences
// [offsets[p], offsets[p + 1]) and runs min(opt[p].max_iterations, 4096, hmax) hypotheses (hmax is the
// grid and the stride of the hypothesis records: the kernels clamp to it) — every input, the counts
// included, is read on the device.  `hyp` is the hypothesis scratch (grown to P * hmax
// records).  vx_pnp_ransac_batch and vx_track_pnp_async both end here.
struct PnpDeviceArgs {
    const int* offsets;           // P + 1
    const double* intr;           // 4 per problem
    const vx_pnp_options* opt;    // per problem
    const float* obj;             // 3 per correspondence
    const float* img;             // 2 per correspondence
    vx_pnp_result* out;           // per problem
    uint8_t* mask;                // per correspondence
};
int pnp_enqueue(vx_ctx* c, int P, int hmax, const PnpDeviceArgs& d, DevBuf& hyp);

// Essential-matrix RANSAC + recoverPose on problems already in device memory (essential.hip), the
// counterpart of pnp_enqueue: k_em_hyp over (hmax, P) (in two launches with k_em_gate between when
// the grid exceeds what is resident at once), k_em_pick over P, k_em_cheir and k_em_final over
// (n_bound / 256, P), enqueued on c->stream, nothing synchronised.  Problem p owns matches
// [offsets[p], offsets[p + 1]) — read on the device; n_bound is the host-side bound of the largest
// problem that sizes the per-match grids — and runs min(opt[p].max_iterations, 4096, hmax) hypotheses.
// `hyp` is the hypothesis scratch.  vx_essential_ransac_batch and vx_track_essential_async both end here.
struct EmDeviceArgs {
    const int* offsets;                // P + 1
    const double* intr;                // 4 per problem
    const vx_essential_options* opt;   // per problem
    const float* p1;                   // 2 per match (pts_last)
    const float* p2;                   // 2 per match (pts_curr)
    vx_essential_result* out;          // per problem
    uint8_t* mask;                     // per match
};
int ess_enqueue(vx_ctx* c, int P, int hmax, int n_bound, const EmDeviceArgs& d, DevBuf& hyp);

// Runs `enqueue` (which only enqueues work on c->stream) through the context's graph cache: the
// first call with a key runs eagerly (so every buffer it needs gets allocated outside a capture),
// the second captures the sequence into a hipGraph, later ones replay it.  Profiling (events
// around launches) and the intra-frame fork bypass the cache.
int graph_run(vx_ctx* c, const std::vector<uint64_t>& key, int (*enqueue)(vx_ctx*, void*), void* arg);
// A graph owned by a long-lived object (a BA plan): captured on its second run, replayed after,
// destroyed with its owner (independently of the context's cache).
struct OwnedGraph {
    hipGraphExec_t exec = nullptr;
    bool seen = false;
    OwnedGraph() = default;
    OwnedGraph(const OwnedGraph&) = delete;
    OwnedGraph& operator=(const OwnedGraph&) = delete;
    ~OwnedGraph();
    void reset();  // forget the captured sequence (the next run is eager, then captured again)
};
int graph_run_owned(vx_ctx* c, OwnedGraph& g, int (*enqueue)(vx_ctx*, void*), void* arg);

// A kernel's >64 KB dynamic-LDS attribute, set once per DEVICE (hipFuncSetAttribute applies to the
// current device only; a function-local static would set it on whichever device came first).
// `done` is a per-call-site bit set of the devices already configured.
inline hipError_t lds_attr_once(int device, const void* fn, int bytes, std::atomic<uint64_t>& done) {
    const uint64_t bit = (device >= 0 && device < 64) ? (1ull << device) : 0;
    if (bit && (done.load(std::memory_order_acquire) & bit)) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess && bit) done.fetch_or(bit, std::memory_order_release);
    return e;
}

}  // namespace vx

#define VX_HIP(ctx, call)                                       \
    do {                                                        \
        hipError_t e__ = (call);                                \
        if (e__ != hipSuccess) return vx::hip_fail(ctx, e__, #call); \
    } while (0)

#define VX_LAUNCH_CHECK(ctx, what)                              \
    do {                                                        \
        hipError_t e__ = hipGetLastError();                     \
        if (e__ != hipSuccess) return vx::hip_fail(ctx, e__, what); \
    } while (0)
