/*
 * vx_slam.h — C ABI of the MI355X-native (gfx950) VisionX-SLAM hot path.
 *
 * One shared library (visionx-slam_amd/lib/libvxslam.so) exports these entry points.  They
 * are plain C: pointers, sizes and status codes, no C++/torch types, no exceptions across the
 * boundary.  Every call returns VX_OK (0) or a negative VX_ERR_*; vx_last_error() gives text.
 *
 * Reference interfaces replaced (paths relative to QinZiwen/VisionX-SLAM):
 *   vx_orb_extract        <- FeatureExtractor::Extract(Frame&)   core/feature/feature_extractor.h:15
 *                            ORBExtractor::Extract               core/feature/orb_extractor.cpp:9-27
 *                            ORBExtractor(n=1000, 1.2f, 8)       core/feature/orb_extractor.h:11-13
 *   vx_orb_extract_batch* <- ORBExtractor::Extract once per camera of a multi-camera time step
 *                            (orb_extractor.cpp:9-27; BASELINE config C5's 8 streams), B frames per launch
 *   vx_match_knn2_ratio   <- FeatureMatcher::Match(last, curr, matches)
 *                                                                core/feature/feature_matcher.h:11-12
 *                            ORBMatcher::Match + Options         core/feature/orb_matcher.cpp:11-43,
 *                                                                orb_matcher.h:11-14
 *   vx_match_*batch*      <- ORBMatcher::Match once per camera pair (orb_matcher.cpp:11-43), up to
 *                            VX_MAX_MATCH_PAIRS pairs per launch
 *   vx_ba_optimize_map    <- LocalBA::Optimize(map, ref_kf)      core/backend/local_ba.h:23,
 *                                                                local_ba.cpp:66-249
 *                            LocalBA::Options                    core/backend/local_ba.h:12-19
 *   vx_depth_landmarks    <- Tracking::CreateLandmarksFromDepth  core/frontend/tracking.cpp:586-650
 *   vx_triangulate        <- Tracking::TriangulateWithLastKeyFrame + TriangulatePoint
 *                                                                core/frontend/tracking.cpp:856-945
 *   vx_pnp_ransac         <- cv::solvePnPRansac in Tracking::TrackWithPnP
 *                                                                core/frontend/tracking.cpp:414-423
 *   vx_track_pnp_*        <- Tracking::TrackWithPnP after Match(): distance filter, 3D-2D pairs over
 *                            Map::GetLandmark, solvePnPRansac, ComputeParallax
 *                                                                core/frontend/tracking.cpp:332-455
 *   vx_essential_ransac   <- cv::findEssentialMat + cv::recoverPose in
 *                            Tracking::EstimatePoseByEssential   core/frontend/tracking.cpp:503-547
 *   vx_track_essential_*  <- Tracking::TrackLastFrame after Match() (and InitWithSecondFrame's head):
 *                            distance filter, 2D-2D pairs, findEssentialMat + recoverPose,
 *                            T_cl * T_lw, ComputeParallax       core/frontend/tracking.cpp:281-330
 *   vx_init_gate_*        <- Tracking::InitWithFirstFrame's gates: feature count, CheckFeatureDistribution,
 *                            CheckImageQuality                   core/frontend/tracking.cpp:93-139, :177-204
 *   vx_frame_*            <- what a Frame keeps of ORBExtractor::Extract (keypoints_, descriptors_), on the
 *                            device for the life of the frame    core/feature/orb_extractor.cpp:13-24
 *   vx_track_frame_*      <- Tracking::Track: TrackWithPnP, else TrackLastFrame, decided on the device
 *                                                                core/frontend/tracking.cpp:267-279
 *   vx_dmap_*             <- visionx::Map (map.h:13-35) kept resident on the device, updated like
 *                            Map::InsertKeyFrame / InsertLandmark / Landmark::AddObservation
 *   vx_dmap_create_keyframe* <- Tracking::CreateKeyFrame's insertion: CreateLandmarksFromDepth,
 *                            TriangulateWithLastKeyFrame, Map::InsertKeyFrame on the resident map
 *                                                                core/frontend/tracking.cpp:577-584
 *   vx_dmap_create_keyframes_rig <- the same for every camera of a rig time step in one call
 *   vx_ba_plan_create_dmap <- the gather of local_ba.cpp:42-108 from the resident map
 *   vx_sba_*              (no reference counterpart: north_star's Schur-complement dense solve)
 *
 * The host-side C++ adapters that keep the reference call surface (same class names and
 * signatures) are in visionx-slam_amd/host/; the bindings a reference maintainer adds are in
 * INTEGRATION.md.
 *
 * Threading: a vx_ctx is not thread-safe; use one per calling thread (the reference calls the
 * hot path from its single tracking thread, core/system/system.cpp:39-52).  Synchronous calls
 * return after results are in caller memory.  *_async calls enqueue on the context's HIP stream
 * and work on device-resident data; vx_synchronize() / the *_fetch calls complete them.
 */
#ifndef VX_SLAM_H
#define VX_SLAM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VX_OK 0
#define VX_ERR_INVALID (-1)   /* bad argument */
#define VX_ERR_HIP (-2)       /* HIP runtime failure (message in vx_last_error) */
#define VX_ERR_CAPACITY (-3)  /* caller buffer too small; *n_out holds the required count */
#define VX_ERR_COMM (-4)      /* RCCL failure */
#define VX_ERR_STATE (-5)     /* call sequence error (e.g. fetch before extract) */

#define VX_MAX_SLOTS 4        /* device-resident keypoint/descriptor slots per context */
#define VX_BATCH_BANKS 2      /* batched-extraction output banks per context */
#define VX_MAX_BATCH 64       /* frames per batched extraction call */
#define VX_MAX_MATCH_PAIRS 16 /* descriptor-set pairs per batched matching call */

typedef struct vx_ctx vx_ctx;

/* cv::KeyPoint fields the reference keeps (orb_extractor.cpp:19-24 keeps pt and response;
 * octave and angle are exported too so callers can reproduce cv::KeyPoint). */
typedef struct {
    float x, y;        /* level-0 pixel coordinates */
    float response;    /* Harris response (HARRIS_SCORE) */
    float angle;       /* degrees [0, 360), intensity centroid */
    int32_t octave;    /* pyramid level */
} vx_keypoint;

/* cv::DMatch with imgIdx = 0 */
typedef struct {
    int32_t query_idx, train_idx;
    float distance;
} vx_match;

/* cv::ORB::create(n_features, scale_factor, n_levels) with OpenCV's remaining defaults
 * (edgeThreshold 31, firstLevel 0, WTA_K 2, HARRIS_SCORE, patchSize 31, fastThreshold 20). */
typedef struct {
    int32_t n_features;      /* 1000 (orb_extractor.h:11) */
    float scale_factor;      /* 1.2f */
    int32_t n_levels;        /* 8   */
    int32_t fast_threshold;  /* 20  */
    int32_t edge_threshold;  /* 31  */
} vx_orb_params;

/* ---------------------------------------------------------------- context */
int vx_version(void);
int vx_create(int device, vx_ctx** out);
/* vx_create with a stream priority (0 normal, 1 the device's greatest) and an optional CU mask
 * (bit i = compute unit i may run this context's workgroups; mask_words 32-bit words, NULL / 0 =
 * every CU).  Disjoint masks keep a latency-critical chain (the LocalBA context of a pipeline)
 * from queueing behind concurrently running bulk work (extraction) — see bench.py --ba-cus. */
int vx_create_ex(int device, int priority, const uint32_t* cu_mask, int mask_words, vx_ctx** out);
/* compute units of a device (the width of a CU mask) */
int vx_device_cus(int device);
void vx_destroy(vx_ctx* ctx);
/* Page-locked, host-cached memory (hipHostMalloc): a vx_map_view whose arrays live in it is uploaded
 * by DMA straight from the caller's arrays (pageable arrays are staged through the runtime's
 * bounce buffers first).  visionx::FlatMap keeps its large arrays in it.  NULL on failure. */
void* vx_host_alloc(size_t bytes);
void vx_host_free(void* p);
const char* vx_last_error(const vx_ctx* ctx);
void* vx_stream(vx_ctx* ctx);          /* the context's hipStream_t */
int vx_synchronize(vx_ctx* ctx);
/* Device-side ordering between two contexts of the same device: work enqueued on `ctx` after
 * this call starts only after everything enqueued on `after` so far has finished (event record on
 * after's stream + stream wait; the host does not block).  This is how a backend context (the
 * LocalBA of keyframe t, which needs tracking(t)) overlaps the frontend context's Extract/Match
 * of frame t+1 — the concurrency ORB-SLAM-style systems get from a separate mapping thread. */
int vx_stream_wait_ctx(vx_ctx* ctx, vx_ctx* after);
/* Device events for finer cross-context ordering (a pipeline that must wait for one specific
 * earlier step of another context, not for everything enqueued on it so far). */
typedef struct vx_event vx_event;
int vx_event_create(vx_ctx* ctx, vx_event** out);
int vx_event_record(vx_ctx* ctx, vx_event* ev); /* marks everything enqueued on ctx so far */
int vx_event_wait(vx_ctx* ctx, vx_event* ev);   /* later work on ctx waits for the marked work */
void vx_event_destroy(vx_event* ev);
/* hipGraph replay: the *_async entry points (and vx_ba_plan_run_async / vx_sba_plan_run_async) run
 * eagerly the first time a launch configuration is seen, capture it into a hipGraph the second
 * time and replay it with one hipGraphLaunch afterwards ($VX_GRAPHS=0 or enable = 0 disables;
 * profiling bypasses it).  Counts of captured graphs and graph launches so far. */
int vx_graph_enable(vx_ctx* ctx, int enable);
int vx_graph_counts(const vx_ctx* ctx, int* captured, int* launched);
/* Fraction (0, 1] of the device's compute units this context's one-round grids (the fused
 * pyramid of vx_orb_extract*) are sized for (default 1).  A frontend context whose extraction
 * runs beside other contexts' work (the LocalBA of the previous keyframe) gets a smaller grid
 * that leaves CUs free: 1/4 in the 3-context pipeline of bench.py.  Results are
 * identical for every share; the call drops the context's captured graphs. */
int vx_set_grid_share(vx_ctx* ctx, float share);
void vx_orb_default_params(vx_orb_params* p);
/* Copies the compiled-in rBRIEF pattern (bit_pattern_31_, 256 x {x1,y1,x2,y2}). */
int vx_orb_pattern(int32_t* out_1024);

/* ---------------------------------------------------------------- ORB extraction
 * img: 8UC1 gray or 8UC3/8UC4 BGR(A) rows of row_stride bytes.  Keypoints are emitted level by
 * level (octave ascending) and, inside a level, in the order OpenCV's KeyPointsFilter::retainBest
 * leaves them when built against libstdc++: std::nth_element + std::partition by FAST score, then
 * again by Harris response (VX_ORDER_STL, the default) — the order ORBExtractor::Extract numbers
 * Frame::Features() in (orb_extractor.cpp:13-24).  VX_ORDER_RASTER (opt-in, vx_orb_set_order)
 * keeps the same keypoint set per level in raster order.  out_desc gets N rows of 32 bytes.
 * Returns VX_ERR_CAPACITY (with *n_out = N) if N > cap. */
#define VX_ORDER_STL 0
#define VX_ORDER_RASTER 1
/* Keypoint order of every later extraction on ctx (drops the context's captured graphs). */
int vx_orb_set_order(vx_ctx* ctx, int order);
int vx_orb_get_order(const vx_ctx* ctx);
/* Test hooks for per-stage parity; single-frame extraction into slot 0
 * (vx_orb_extract) only.  VX_ORB_DEBUG_FAST_NO_BORDER makes k_fast keep every FAST + NMS corner
 * of [3, W-3) x [3, H-3) (the list before runByImageBorder; the later stages are then NOT the
 * reference's); VX_ORB_DEBUG_STAGES records the selection's stages.  vx_orb_debug_read(level,
 * what): 0 the gray / INTER_LINEAR_EXACT level (lw*lh bytes), 1 its GaussianBlur, 2 the level's
 * candidates in raster order (16-byte records {x | y << 16, FAST score, float Harris, 0}),
 * 3 retainBest(2q)'s output order (int32 indices into the candidates), 4 retainBest(q)'s output
 * (16-byte records, the order k_describe emits).  *n_out = elements (bytes for 0/1). */
#define VX_ORB_DEBUG_FAST_NO_BORDER 1
#define VX_ORB_DEBUG_STAGES 2
int vx_orb_set_debug(vx_ctx* ctx, int flags);
int vx_orb_debug_read(vx_ctx* ctx, int level, int what, void* out, int64_t cap_bytes, int64_t* n_out);
/* Test hook: KeyPointsFilter::retainBest(keys, npts) through the device selection code (one
 * workgroup): elements u32 (key <= 255, the FAST-score path) or wide = u64 (the Harris path),
 * in LDS or in global memory; out_idx = kept key indices in output order. */
int vx_test_retain_best(vx_ctx* ctx, const uint32_t* keys, int n, int npts, int wide, int use_lds,
                        int32_t* out_idx, int* n_out);
int vx_orb_extract(vx_ctx* ctx, const vx_orb_params* params, const uint8_t* img, int width,
                   int height, int channels, int64_t row_stride, vx_keypoint* out_kp,
                   uint8_t* out_desc, int cap, int* n_out);
/* Device-resident variant: d_img is device memory; results stay in `slot`. */
int vx_orb_extract_async(vx_ctx* ctx, const vx_orb_params* params, const uint8_t* d_img,
                         int width, int height, int channels, int64_t row_stride, int slot);
int vx_orb_fetch(vx_ctx* ctx, int slot, vx_keypoint* out_kp, uint8_t* out_desc, int cap,
                 int* n_out);
/* Device pointers of a slot's descriptor rows and its device-side count, and its row capacity
 * (for interop and for vx_match_device_async from another context).  Stable until the ORB
 * geometry (image size / params) of the context changes. */
int vx_orb_slot_device(vx_ctx* ctx, int slot, const uint8_t** d_desc, const int32_t** d_count,
                       int32_t* cap);

/* Batched extraction (SURVEY.md 8(d) batched figures; the C5 multi-camera rig): n_frames images
 * of one size, frame f at d_imgs + f * frame_stride (device memory), extracted by ONE launch per
 * kernel (frame = grid z) instead of one extraction per frame — same results as vx_orb_extract
 * for every frame.  Each frame's keypoints / descriptors stay in output bank `bank` (two banks,
 * so a camera's batch t can be matched against its batch t-1) at index f: vx_orb_batch_fetch
 * copies them out, vx_orb_batch_device hands their device rows to vx_match_*_async. */
int vx_orb_extract_batch_async(vx_ctx* ctx, const vx_orb_params* params, const uint8_t* d_imgs,
                               int n_frames, int64_t frame_stride, int width, int height, int channels,
                               int64_t row_stride, int bank);
/* Host-image variant: imgs[f] are host rows of row_stride bytes (all frames one size), uploaded
 * into the context, then extracted as one batch into `bank`. */
int vx_orb_extract_batch(vx_ctx* ctx, const vx_orb_params* params, const uint8_t* const* imgs,
                         int n_frames, int width, int height, int channels, int64_t row_stride,
                         int bank);
int vx_orb_batch_fetch(vx_ctx* ctx, int bank, int frame, vx_keypoint* out_kp, uint8_t* out_desc,
                       int cap, int* n_out);
int vx_orb_batch_device(vx_ctx* ctx, int bank, int frame, const uint8_t** d_desc,
                        const int32_t** d_count, int32_t* cap);

/* ---------------------------------------------------------------- matching
 * knnMatch(query = last frame, train = current frame, k = 2) + ratio test
 * (m1.distance < ratio * m2.distance), matches in ascending query index. */
int vx_match_knn2_ratio(vx_ctx* ctx, const uint8_t* query_desc, int n_query,
                        const uint8_t* train_desc, int n_train, float ratio, vx_match* out,
                        int cap, int* n_out);
/* Device-resident variant matching two extraction slots (counts read on device). */
int vx_match_slots_async(vx_ctx* ctx, int query_slot, int train_slot, float ratio);
/* Device-resident variant over any device descriptor sets whose row counts are device-side
 * (e.g. another context's slots, vx_orb_slot_device); cap_* bound the rows.  Enqueued on ctx's
 * stream: order it after the producer with vx_event_wait / vx_stream_wait_ctx. */
int vx_match_device_async(vx_ctx* ctx, const uint8_t* d_query, const int32_t* d_n_query, int cap_query,
                          const uint8_t* d_train, const int32_t* d_n_train, int cap_train, float ratio);
int vx_match_fetch(vx_ctx* ctx, vx_match* out, int cap, int* n_out);
/* Batched matching: n_pairs (<= VX_MAX_MATCH_PAIRS) independent kNN-2 + ratio problems in one
 * launch pair (pair = grid y), query set i = d_query[i] (d_n_query[i] rows on the device, at most
 * cap_query), train set i likewise — e.g. each camera's frame t against its frame t-1 from two
 * batch banks.  The pointer arrays are host arrays of device pointers.  Results per pair:
 * vx_match_batch_fetch(ctx, i, ...), identical to vx_match_device_async on that pair alone. */
int vx_match_batch_async(vx_ctx* ctx, int n_pairs, const uint8_t* const* d_query,
                         const int32_t* const* d_n_query, int cap_query, const uint8_t* const* d_train,
                         const int32_t* const* d_n_train, int cap_train, float ratio);
/* Host-descriptor variant: pair i = query q[i] (nq[i] rows of 32 B) against train t[i] (nt[i]
 * rows), uploaded in one copy; a pair with an empty side yields 0 matches (orb_matcher.cpp:18-20). */
int vx_match_knn2_ratio_batch(vx_ctx* ctx, int n_pairs, const uint8_t* const* q, const int32_t* nq,
                              const uint8_t* const* t, const int32_t* nt, float ratio);
int vx_match_batch_fetch(vx_ctx* ctx, int pair, vx_match* out, int cap, int* n_out);

/* ---------------------------------------------------------------- local bundle adjustment
 * A flattened snapshot of visionx::Map (map.h:13-34): keyframes with their Feature vectors
 * (frame.h:16-23) and landmarks with their observation maps (landmark.h:12-68).  Keyframes may
 * be in any order (the reference's std::map sorts them by id).  kf_pose and lm_pos are updated
 * in place, exactly as Frame::SetPose / Landmark::SetPosition would be. */
typedef struct {
    int32_t n_kf;
    const uint64_t* kf_id;
    double* kf_pose;             /* 7 per KF: qx qy qz qw tx ty tz (T_cw, world -> camera) */
    const double* kf_intr;       /* 4 per KF: fx fy cx cy */
    const uint8_t* kf_has_cam;   /* Frame::GetCamera() != nullptr */
    const int64_t* kf_feat_ptr;  /* n_kf + 1, CSR into the feature arrays */
    const double* feat_uv;       /* 2 per feature */
    const uint64_t* feat_lm_id;  /* Feature::landmark_id_ */
    const uint8_t* feat_flags;   /* bit0 has_landmark, bit1 is_outlier */
    int32_t n_lm;
    const uint64_t* lm_id;       /* distinct ids in any order (not necessarily sorted: lookups hash them) */
    double* lm_pos;              /* 3 per landmark */
    const uint8_t* lm_bad;
    const int64_t* lm_obs_ptr;   /* n_lm + 1, CSR of (kf id, feature index) observations */
    const uint64_t* obs_kf_id;
    const uint64_t* obs_feat_idx;
} vx_map_view;

typedef struct {                 /* LocalBA::Options, local_ba.h:12-19 */
    int32_t window_size;         /* 5 */
    int32_t max_iterations;      /* 5 */
    int32_t min_pose_observations;   /* 20 */
    int32_t min_point_observations;  /* 2 */
    double huber_delta;          /* 5.0 */
    double max_reproj_error;     /* 5.0 */
} vx_ba_options;

typedef struct {
    int32_t iterations;          /* outer iterations executed (including the one that broke) */
    int32_t n_window_kf, n_landmarks;
    double cost[16];             /* pose-stage total_cost per iteration */
    int32_t obs[16];             /* pose-stage total_obs per iteration */
    double gate_margin;          /* unused by the GPU path (set to -1) */
    int32_t status;              /* 0 optimised, 1 early return (no KF pair / no landmark) */
} vx_ba_stats;

void vx_ba_default_options(vx_ba_options* o);
/* Reproducibility: unsharded windows sum each keyframe's normal-equation row with FP64 float
 * atomics by default (arrival order), so two runs of the same input agree to rounding (~1e-8
 * relative in the positions after five iterations; residuals move < 1e-7 px), not bit for bit.
 * Set $VX_BA_ATOMIC_ROWS=0 before the plan is built for per-workgroup partial slots summed in a fixed
 * order: bitwise-repeatable runs, ~7 % slower LocalBA.  Sharded plans always use
 * the slots. */
int vx_ba_optimize_map(vx_ctx* ctx, vx_map_view* map, uint64_t ref_kf_id, int has_ref,
                       const vx_ba_options* opt, vx_ba_stats* stats);

/* Staged form: plan = window selection + device CSR upload (host work of local_ba.cpp:66-108);
 * run = the iterations on the device from the plan's initial state (repeatable);
 * fetch = download + scatter back into `map` (may be NULL to only read stats).
 * shard_count > 1 keeps only this rank's landmark shard (landmark id hash) and all-reduces the
 * per-keyframe normal equations over the communicator set by vx_comm_init. */
typedef struct vx_ba_plan vx_ba_plan;
int vx_ba_plan_create(vx_ctx* ctx, const vx_map_view* map, uint64_t ref_kf_id, int has_ref,
                      const vx_ba_options* opt, int shard_rank, int shard_count,
                      vx_ba_plan** out);
/* flags: VX_PLAN_HOST_BUILD builds the plan with the host reference restatement of
 * local_ba.cpp:42-108 (hash maps, one core) instead of the device build (default: window join,
 * slot assignment and both CSRs as HIP kernels).  Both give the same plan. */
#define VX_PLAN_HOST_BUILD 1
/* VX_PLAN_GLOBAL_POSES runs the large-window kernels (poses solved once into global memory, one
 * thread per landmark) at any window size; by default they run only beyond 448 keyframes, where
 * the per-workgroup LDS copy of every keyframe's pose no longer fits.  Same results. */
#define VX_PLAN_GLOBAL_POSES 2
int vx_ba_plan_create_ex(vx_ctx* ctx, const vx_map_view* map, uint64_t ref_kf_id, int has_ref,
                         const vx_ba_options* opt, int shard_rank, int shard_count, int flags,
                         vx_ba_plan** out);
int vx_ba_plan_run_async(vx_ctx* ctx, vx_ba_plan* plan);
int vx_ba_plan_fetch(vx_ctx* ctx, vx_ba_plan* plan, vx_map_view* map, vx_ba_stats* stats);
void vx_ba_plan_destroy(vx_ba_plan* plan);
/* sizes of the device problem: out8 = {n_kf, n_lm (local shard), n_pose_obs, n_lm_obs, n_opt,
 * n_split (pose-stage workgroups per keyframe), n_lm_blocks (landmark-stage workgroups),
 * max_lm_obs (most landmark-stage observations of one landmark)} */
int vx_ba_plan_info(const vx_ba_plan* plan, int64_t* out8);
/* kernel layout of the plan: out4 = {1 if it has the fused one-launch-per-iteration layout
 * (k_ba_iter) else 0, threads per fused workgroup, fused workgroups, most partial slots of one
 * keyframe}.  A sharded plan runs the fused kernel only when every rank has the layout (decided by
 * one all-reduce on its first run). */
int vx_ba_plan_layout(const vx_ba_plan* plan, int64_t* out4);
/* 1 when the plan's runs are ONE persistent launch per window (k_ba_win: unsharded float-atomic
 * plans whose workgroups fit on the device at once; $VX_BA_PERSIST=0 disables it), 0 when they are
 * one launch per iteration.  A persistent run whose bounded waits ran out (its workgroups could not
 * all be resident, e.g. another persistent window held the compute units) is re-run by
 * vx_ba_plan_fetch with the per-iteration launches, which the plan keeps from then on. */
int vx_ba_plan_persistent(const vx_ba_plan* plan);
/* Test hook: the fused layout's index tables (workgroup headers, landmark slots and runs,
 * landmark-stage records, keyframe entries, landmark- and pose-stage observation sources, pose
 * codes) copied back to back into dst; *bytes = their total size (dst NULL: the size only).  The
 * device build of the layout must equal the host packing (VX_PLAN_HOST_BUILD) byte for byte. */
int vx_ba_plan_fused_tables(vx_ctx* ctx, const vx_ba_plan* plan, void* dst, size_t cap, size_t* bytes);
/* Test hook: runs the n shard plans plans[r] (shard r of n, built from one window, all on ctx) the
 * way n ranks would run them, on one device: per iteration every shard's pose stage, then the
 * element-wise sum of their partial blocks in rank order written back to every shard in place of
 * the ncclAllReduce, then every shard's landmark stage (the kernel set chosen from the maxima over
 * the shards, as the all-reduced choice of a real sharded run).  Fetch each plan afterwards. */
int vx_ba_shard_emulate_run(vx_ctx* ctx, vx_ba_plan* const* plans, int n);
/* Host-only dry run of vx_ba_plan_create (needs no device): out8 = {status, n_window_kf,
 * n_landmarks (all shards), n_kf, n_opt (local optimisable), n_lm (local table), n_pose_obs,
 * n_lm_obs}; lm_map_idx / kf_map_idx (optional) receive the local tables as map indices. */
int vx_ba_plan_inspect(const vx_map_view* map, uint64_t ref_kf_id, int has_ref,
                       const vx_ba_options* opt, int shard_rank, int shard_count, int64_t* out8,
                       int32_t* lm_map_idx, int cap_lm, int32_t* kf_map_idx, int cap_kf);
/* Landmark -> shard assignment used by sharded plans (splitmix64(id) mod shard_count). */
uint32_t vx_ba_shard_of(uint64_t lm_id, int shard_count);

/* ---------------------------------------------------------------- device-resident map
 * A persistent mirror of visionx::Map on the device: keyframes with their
 * features, landmarks, observations, updated incrementally as Tracking / the Map change them
 * (Map::InsertKeyFrame, Map::InsertLandmark, Landmark::AddObservation, Feature::landmark_id_,
 * Landmark::SetBad, Frame::SetPose), so a LocalBA plan is built from device memory — no map
 * snapshot crosses PCIe per keyframe — and its result is scattered back into the device map
 * without a host round trip.  Keyframes / landmarks keep their insertion order (the map index
 * order of an equivalent vx_map_view); a landmark's observations keep their insertion order.
 * Capacities grow on demand. */
typedef struct vx_dmap vx_dmap;
int vx_dmap_create(vx_ctx* ctx, vx_dmap** out);
void vx_dmap_destroy(vx_dmap* map);
/* Map::InsertKeyFrame: kf_id unique; pose7 T_cw; intr4 fx fy cx cy (ignored unless has_cam);
 * features as in vx_map_view (uv 2 each, landmark ids, flags bit0 has_landmark bit1 is_outlier) */
int vx_dmap_add_keyframe(vx_dmap* map, uint64_t kf_id, const double* pose7, const double* intr4, int has_cam,
                         int n_feat, const double* feat_uv, const uint64_t* feat_lm_id, const uint8_t* feat_flags);
/* Map::InsertLandmark: ids unique; pos 3 each; bad may be NULL (all good) */
int vx_dmap_add_landmarks(vx_dmap* map, int n, const uint64_t* lm_id, const double* pos3, const uint8_t* bad);
/* Landmark::AddObservation(kf_id, feat_idx) on existing landmarks (VX_ERR_INVALID for unknown ids).
 * Like observations_[keyframe_id] = feature_idx (landmark.h:32-35), a (landmark, keyframe) pair
 * already present keeps its place and takes the new feature index; a landmark never holds two
 * observations from one keyframe.  Each new pair takes an observation id for the map's life (8 B of
 * device memory per pair ever added; compaction reclaims rows, not ids). */
int vx_dmap_add_observations(vx_dmap* map, int n, const uint64_t* lm_id, const uint64_t* kf_id,
                             const uint64_t* feat_idx);
/* Landmark::RemoveObservation(kf_id) (landmark.h:37-40): the pair stops counting towards
 * ObservationCount and leaves the landmark's list; an absent pair is a no-op (unordered_map::erase).
 * VX_ERR_INVALID for an unknown landmark id. */
int vx_dmap_remove_observations(vx_dmap* map, int n, const uint64_t* lm_id, const uint64_t* kf_id);
/* Map::RemoveKeyFrame(id) (map.cpp:15-18): the keyframe leaves the map (SelectKeyFrames no longer
 * sees it; observations naming it fail the window check like GetFrame() == nullptr).  Its feature
 * rows stay as dead storage.  The id may be inserted again later.  VX_ERR_INVALID if absent.
 * Tracking::RemoveKeyFrame (tracking.cpp:752-773) = vx_dmap_remove_observations for the frame's
 * landmark features + vx_dmap_set_features (0, no landmark, outlier) + this call. */
int vx_dmap_remove_keyframe(vx_dmap* map, uint64_t kf_id);
/* Map::RemoveLandmark(id) (map.cpp:20-23): GetLandmark() == nullptr afterwards (pose stage and
 * landmark set skip it).  Absent ids are a no-op, as std::unordered_map::erase. */
int vx_dmap_remove_landmarks(vx_dmap* map, int n, const uint64_t* lm_id);
/* Feature::landmark_id_ / has_landmark / is_outlier of features of keyframe kf_id */
int vx_dmap_set_features(vx_dmap* map, uint64_t kf_id, int n, const int32_t* feat_idx, const uint64_t* lm_id,
                         const uint8_t* flags);
int vx_dmap_set_landmark_bad(vx_dmap* map, int n, const uint64_t* lm_id, const uint8_t* bad);
int vx_dmap_set_poses(vx_dmap* map, int n, const uint64_t* kf_id, const double* pose7);
/* out4 = {keyframe rows, feature rows, landmark rows, observation rows}: storage rows in insertion
 * order, removed ones included (vx_dmap_download returns that many) */
int vx_dmap_counts(const vx_dmap* map, int64_t* out4);
/* out4 = {keyframes, landmarks, observations, 0} currently in the map (removed ones excluded) */
int vx_dmap_live_counts(const vx_dmap* map, int64_t* out4);
/* current poses (7 per keyframe row) / positions (3 per landmark row) in insertion order (rows of
 * removed keyframes / landmarks included); either may be NULL */
int vx_dmap_download(vx_dmap* map, double* kf_pose, double* lm_pos);
/* LocalBA plan from the resident map (the plan vx_ba_plan_create builds from the equivalent
 * vx_map_view snapshot); run with vx_ba_plan_run_async as usual */
int vx_ba_plan_create_dmap(vx_ctx* ctx, vx_dmap* map, uint64_t ref_kf_id, int has_ref, const vx_ba_options* opt,
                           int shard_rank, int shard_count, vx_ba_plan** out);
/* enqueue the scatter of a run's window poses and optimised landmark positions into the map (stream
 * ordered after the run; no host synchronisation) */
int vx_ba_plan_apply_dmap(vx_ctx* ctx, vx_ba_plan* plan, vx_dmap* map);
/* LocalBA::Optimize(map, ref_kf) (local_ba.cpp:66-249) on the resident map in ONE call: window
 * selection over the host id mirror, then plan build, iterations and the scatter of the results into
 * the map's rows as one stream-ordered sequence over buffers sized by capacity, with the counts kept
 * on the device — the call synchronises once, at its end, to fill `stats` (ba_lean.hip).  Windows of
 * more than 255 keyframes (or $VX_LEAN=0) take the general build (vx_ba_plan_create_dmap + run +
 * apply) inside the same call.  Same status / iteration / observation counts as vx_ba_optimize_map on
 * the equivalent snapshot; poses and positions within the BA tolerance. */
int vx_ba_optimize_dmap(vx_ctx* ctx, vx_dmap* map, uint64_t ref_kf_id, int has_ref, const vx_ba_options* opt,
                        vx_ba_stats* stats);
/* What the last vx_ba_optimize_dmap changed (for a host Map mirror: Frame::SetPose /
 * Landmark::SetPosition, local_ba.cpp:173,237): *n_kf window keyframe rows (insertion order rows of
 * the map) with their poses (7 each) and *n_lm optimised landmark rows with their positions (3 each);
 * both 0 when nothing was optimised.  Any output pointer may be NULL; VX_ERR_CAPACITY if a count
 * exceeds its cap (the counts are set either way). */
int vx_ba_dmap_results(vx_ctx* ctx, vx_dmap* map, int cap_kf, int64_t* kf_rows, double* kf_pose7, int cap_lm,
                       int64_t* lm_rows, double* lm_pos3, int* n_kf, int* n_lm);
/* on != 0: every following vx_ba_optimize_dmap also copies its results (both pose buffers, the
 * optimised positions and their rows, sized by the call's capacities) into pinned host memory before
 * its one synchronisation, so vx_ba_dmap_results then only copies on the host — no device call, no
 * second synchronisation (what a drop-in that writes every result back wants; default off). */
int vx_dmap_prefetch_results(vx_dmap* map, int on);
/* The same results without a copy, with prefetching on: pointers into the pinned block the last
 * vx_ba_optimize_dmap filled, valid until the next vx_ba_optimize_dmap / vx_dmap_* call on the map —
 * *n_kf keyframe rows (int32) with their poses (8 doubles each: qx qy qz qw tx ty tz, pad), *n_lm
 * landmark rows (int32) with their positions (4 doubles each: x y z, pad); both counts 0 (pointers
 * NULL) when nothing was optimised.  VX_ERR_STATE when the results were not prefetched (prefetching
 * off, or a run that fell back to a built plan): use vx_ba_dmap_results then. */
int vx_ba_dmap_results_view(vx_ctx* ctx, vx_dmap* map, const int32_t** kf_rows, const double** kf_pose8,
                            const int32_t** lm_rows, const double** lm_pos4, int* n_kf, int* n_lm);

/* ---------------------------------------------------------------- Schur-complement joint BA
 * NOT a reference entry point: the reference's LocalBA alternates per-keyframe and per-landmark
 * steps (local_ba.cpp:116-238).  BASELINE.json's north_star (and configs C5) ask for the
 * Schur-complement reduction of the landmark blocks into the dense 6N x 6N pose system and a
 * dense pose solve; this is that solver, on the same window / landmark set / observations /
 * residual / Jacobians / Huber weight / gates as LocalBA (local_ba.cpp:15-108, projection.h:11-31),
 * as one damped Gauss-Newton (Levenberg-Marquardt) system with b = +J^T W e, the oldest
 * `fixed_keyframes` window keyframes held fixed.  Same map snapshot and plan life cycle as
 * vx_ba_plan_*; shard_count > 1 shards landmarks and all-reduces the reduced system over RCCL.
 * Parity is against its CPU restatement (oracle/sba_oracle.cpp), see DESIGN.md §10. */
typedef struct {
    int32_t window_size;             /* keyframes in the window (SelectKeyFrames) */
    int32_t max_iterations;          /* assemblies: initial + accepted + rejected steps, <= 64 */
    int32_t min_point_observations;  /* landmark filter (local_ba.cpp:100-102) */
    int32_t fixed_keyframes;         /* oldest window keyframes held fixed (gauge, 2: also the scale) */
    double huber_delta;              /* 5.0 */
    double max_reproj_error;         /* 5.0 */
    double lambda_init;              /* Marquardt damping H_ii += lambda * H_ii (1e-4) */
    double rel_tol;                  /* stop after an accepted step lowering the cost by < rel_tol */
} vx_sba_options;

typedef struct {
    int32_t iterations;          /* assemblies executed */
    int32_t accepted;            /* accepted steps */
    int32_t n_window_kf, n_landmarks;
    double cost[16];             /* Huber cost at each assembly */
    int32_t obs[16];             /* valid observations at each assembly */
    int32_t step[16];            /* 2 initial, 1 accepted, 0 rejected, 3 re-assembled after a reject */
    double lambda;               /* damping after the last iteration */
    double initial_cost, final_cost;
    int32_t status;              /* 0 optimised, 1 early return (no KF pair / no landmark) */
} vx_sba_stats;

typedef struct vx_sba_plan vx_sba_plan;
void vx_sba_default_options(vx_sba_options* o);
int vx_sba_plan_create(vx_ctx* ctx, const vx_map_view* map, uint64_t ref_kf_id, int has_ref,
                       const vx_sba_options* opt, int shard_rank, int shard_count, vx_sba_plan** out);
int vx_sba_plan_run_async(vx_ctx* ctx, vx_sba_plan* plan);
int vx_sba_plan_fetch(vx_ctx* ctx, vx_sba_plan* plan, vx_map_view* map, vx_sba_stats* stats);
void vx_sba_plan_destroy(vx_sba_plan* plan);
/* out8 = {n_kf, n_opt (local landmarks), n_obs, n_pairs, n_blocks, n (= 6 n_kf), nonzero 16x16
 * tiles of the Cholesky factors (symbolic factorisation, rhs row included), n_components} */
int vx_sba_plan_info(const vx_sba_plan* plan, int64_t* out8);
/* The dense pose solve's symbolic work (all components; the rhs row's tiles left out): out4 =
 * {nonzero tiles of L, trailing-update tile products (16x16x16 each), diagonal tiles (one POTRF
 * each), off-diagonal panel tiles (one TRSM each)} -> algorithmic FP64 flops of one factorisation
 * 2*16^3 * updates + 16^3 * panel + 16^3/3 * diagonal (bench.py's MFMA roofline for config C5). */
int vx_sba_plan_factor_work(const vx_sba_plan* plan, int64_t* out4);
/* The reduced system of the LAST assembly of the last run (S row-major n x n, lower triangle
 * meaningful, damping included; rhs n), for verification against the restatement. */
int vx_sba_plan_system(vx_ctx* ctx, vx_sba_plan* plan, double* S, double* rhs, int n);
/* Test hook: the pose step dx (n = 6 n_kf, window order, (upsilon, omega) per keyframe) of the last
 * iteration of the last run that solved, i.e. the dense pose solve's output.  Sign: S dx = +rhs with
 * S and rhs as vx_sba_plan_system reports them for the assembly that was factored (rhs = g_T -
 * sum Y g_p with b = +J^T W e); k_sba_update applies it as T <- exp(dx) T and dp = V^-1 (g_p - W^T dx).
 * Fixed keyframes keep 0.  Iterations that do not solve (a rejected step's successor, the last one)
 * leave dx alone, so with max_iterations = 2 it is the solve of the first assembly damped with
 * lambda_init.  *fail = 1 if a component's Cholesky met a non-positive pivot in any iteration of the
 * run.  Errors as vx_sba_plan_system (empty plan, wrong n, plan not run). */
int vx_sba_plan_step(vx_ctx* ctx, vx_sba_plan* plan, double* dx, int n, int32_t* fail);
/* The same plan from the device-resident map (vx_dmap): window, landmark set and observation set as
 * for the equivalent snapshot, the observation / pair / block tables sorted on the device (two small
 * read-backs: the counts, then the block list for the host's covisibility components and symbolic
 * factorisation).  Unsharded.  Fetch statistics with vx_sba_plan_fetch(map = NULL); the result goes
 * into the map's rows with vx_sba_plan_apply_dmap (stream ordered, no host synchronisation). */
int vx_sba_plan_create_dmap(vx_ctx* ctx, vx_dmap* map, uint64_t ref_kf_id, int has_ref, const vx_sba_options* opt,
                            vx_sba_plan** out);
/* Rebuild a plan made by vx_sba_plan_create_dmap in place for the map's current state and ref_kf_id,
 * with the plan's options: its device buffers and host staging are reused (grown when the window
 * needs more), so a drop-in that keeps one plan per backend pays no allocation or release per
 * Backend::Optimize() (the reference builds its problem per call, core/backend/local_ba.cpp:42-108).
 * The plan's captured run graph is dropped (the next run is eager).  On error the plan is left
 * unusable (status set, no run) until a successful rebuild. */
int vx_sba_plan_rebuild_dmap(vx_ctx* ctx, vx_dmap* map, uint64_t ref_kf_id, int has_ref, vx_sba_plan* plan);
int vx_sba_plan_apply_dmap(vx_ctx* ctx, vx_sba_plan* plan, vx_dmap* map);
/* Test hook, the Schur counterpart of vx_ba_shard_emulate_run: the n shard plans of one window
 * (vx_sba_plan_create with shard_rank r of n, all on ctx; every shard's block structure is the whole
 * window's) run as n ranks would on one device — per iteration every shard's landmark stage and
 * blocks, then their reduced systems summed element-wise in rank order into every shard in place of
 * the ncclAllReduce, then every shard's (identical) factorisation, back-substitution and update.
 * Fetch each plan afterwards. */
int vx_sba_shard_emulate_run(vx_ctx* ctx, vx_sba_plan* const* plans, int n);
int vx_sba_optimize_map(vx_ctx* ctx, vx_map_view* map, uint64_t ref_kf_id, int has_ref,
                        const vx_sba_options* opt, vx_sba_stats* stats);

/* ---------------------------------------------------------------- landmark creation
 * The two loops Tracking::CreateKeyFrame runs on every new keyframe right before LocalBA
 * (core/frontend/tracking.cpp:577-580).  Both return the created landmarks in input order (the
 * order landmark_id_++ numbers them): out_index[i] = rank of item i among the created ones or -1,
 * out_pw[3 * rank ..] = its world position; *n_created = count.  The caller creates the Landmark
 * objects, adds the observations and sets Feature::landmark_id_ / has_landmark / is_outlier
 * exactly as the reference loop body does. */
#define VX_DEPTH_U16 0   /* CV_16U, metres * 5000 (TUM; kDepthScale, tracking.cpp:601) */
#define VX_DEPTH_F32 1   /* CV_32F metres */
#define VX_DEPTH_F64 2   /* CV_64F metres */

/* <- Tracking::CreateLandmarksFromDepth(frame) (tracking.cpp:586-650): features without a
 * landmark, depth at (int)(x + 0.5), (int)(y + 0.5), 0.1 <= d <= 10 m, pw = T_cw^-1 * pixelToCamera.
 * feat_uv: 2 per feature (Feature::position); intr4: fx fy cx cy; pose7: T_cw (qx qy qz qw tx ty tz).
 * depth == NULL (Depth().empty()) creates nothing. */
int vx_depth_landmarks(vx_ctx* ctx, const double* feat_uv, const uint8_t* feat_has_lm, int n_feat,
                       const void* depth, int depth_type, int rows, int cols, int64_t row_stride,
                       const double* intr4, const double* pose7, int32_t* out_index, double* out_pw,
                       int* n_created);
/* <- Tracking::TriangulateWithLastKeyFrame(last, curr) + TriangulatePoint (tracking.cpp:856-945)
 * over the matches Match(last, curr) returned (query = last frame, train = current frame; query
 * indices unique): parallax >= min_angle_deg, 4x4 DLT null vector, reprojection <= max_reproj_error
 * in both views; a train feature triangulated by an earlier match is skipped (the reference sets
 * has_landmark as it goes).  Options: Tracking::Options (tracking.h:43-44), 5.0 px / 1.0 deg. */
int vx_triangulate(vx_ctx* ctx, const double* uv1, const uint8_t* has1, int n1, const double* intr1,
                   const double* pose1, const double* uv2, const uint8_t* has2, int n2,
                   const double* intr2, const double* pose2, const vx_match* matches, int n_matches,
                   double min_angle_deg, double max_reproj_error, int32_t* out_index, double* out_pw,
                   int* n_created);

/* ---------------------------------------------------------------- geometry RANSAC (ransac.hip)
 * <- cv::solvePnPRansac(pts_3d, pts_2d, K, noArray(), rvec, tvec, false, iterations,
 *    max_reproj_error, 0.99, inliers) in Tracking::TrackWithPnP (tracking.cpp:414-423).
 * All hypotheses are generated and scored at once on the device; the sequential RANSAC loop's
 * adaptive stop rule (RANSACUpdateNumIters) is then replayed over them in order, so the selected
 * model is the one a sequential run over the same hypothesis stream keeps.  Minimal solver: P3P
 * (Grunert) on 3 points, the 4th of the sample picks among its up to 4 solutions; hypotheses come
 * from a counter-based splitmix64 stream (OpenCV's cv::RNG stream and its EPnP kernel are not
 * reproduced: parity against OpenCV is unpinned).  Inliers: point in front of the
 * camera and squared reprojection error <= reproj_error^2.  The kept model is refined on its
 * inliers by Levenberg-Marquardt (the SOLVEPNP_ITERATIVE refinement solvePnPRansac runs). */
typedef struct {
    int32_t max_iterations;    /* iterationsCount (tracking.cpp:420: min(100, 2 * n)), <= 4096 */
    int32_t refine_iterations; /* LM iterations on the inliers (0: keep the RANSAC model) */
    double reproj_error;       /* reprojectionError, px (Tracking::Options::max_reproj_error 2.0) */
    double confidence;         /* 0.99 (tracking.cpp:423) */
    uint64_t seed;             /* hypothesis stream */
} vx_pnp_options;
typedef struct {
    int32_t ok;                /* solvePnPRansac's return value */
    int32_t n_inliers;         /* inliers.rows */
    int32_t best_hypothesis;   /* index of the kept hypothesis, -1 when !ok */
    int32_t hypotheses_run;    /* hypotheses the adaptive stop rule let the loop evaluate */
    int32_t refine_iterations; /* LM iterations performed */
    int32_t reserved;
    double rvec[3], tvec[3];   /* T_cw as cv::Rodrigues vector + translation */
    double pose[7];            /* the same T_cw as Sophus storage: qx qy qz qw tx ty tz */
    double cost0, cost;        /* sum of squared reprojection errors over the inliers, before / after LM */
} vx_pnp_result;
/* tracking.cpp:420-423 defaults for n correspondences: min(100, 2n) iterations, 2.0 px, 0.99, 20 LM */
void vx_pnp_default_options(int n_points, vx_pnp_options* out);
/* obj_pts: 3 floats per correspondence (cv::Point3f), img_pts: 2 floats (cv::Point2f), intr4: fx fy
 * cx cy (no distortion, as the reference passes cv::Mat()).  inlier_mask (n bytes) may be NULL. */
int vx_pnp_ransac(vx_ctx* ctx, const float* obj_pts, const float* img_pts, int n, const double* intr4,
                  const vx_pnp_options* opt, uint8_t* inlier_mask, vx_pnp_result* out);
/* Independent problems in one pass (e.g. the C5 rig's 8 camera streams): problem p owns
 * correspondences [offsets[p], offsets[p+1]), intrinsics intr4[4p..], options opt[p]; inlier_mask
 * covers all offsets[n_problems] correspondences; out[p] per problem. */
int vx_pnp_ransac_batch(vx_ctx* ctx, int n_problems, const int32_t* offsets, const float* obj_pts,
                        const float* img_pts, const double* intr4, const vx_pnp_options* opt,
                        uint8_t* inlier_mask, vx_pnp_result* out);

/* ---------------------------------------------------------------- TrackWithPnP on the device (track.hip)
 * <- Tracking::TrackWithPnP after Match(last_keyframe, curr) (tracking.cpp:332-455): the distance
 *    filter (:342-355), the 3D-2D pair build over Map::GetLandmark (:364-400), solvePnPRansac
 *    (:414-423) and ComputeParallax (:449, :548-560) as ONE stream-ordered sequence over data that is
 *    already on the device — the match list, the current frame's keypoints, the resident map — with
 *    one synchronisation, in the fetch. */
typedef struct {
    int32_t min_matches;        /* Tracking::Options::min_matches 50 (tracking.cpp:357) */
    int32_t min_inliers;        /* Tracking::Options::min_inliers 30 (tracking.cpp:402, :425) */
    vx_pnp_options pnp;         /* max_iterations < 0: min(100, 2 * n_pairs), computed on the device
                                   (tracking.cpp:421); reproj 2.0, conf 0.99, 20 LM, seed 0x5EED */
} vx_track_options;

#define VX_TRACK_OK 0
#define VX_TRACK_FEW_MATCHES 1   /* filtered matches < min_matches          (tracking.cpp:357) */
#define VX_TRACK_FEW_PAIRS 2     /* 3D-2D pairs < min_inliers               (tracking.cpp:402) */
#define VX_TRACK_PNP_FAILED 3    /* !ok || inliers < min_inliers            (tracking.cpp:425) */
#define VX_TRACK_BAD_ROTATION 4  /* non-finite R                            (tracking.cpp:441) */

typedef struct {
    int32_t status, n_matches, n_good_matches, n_pairs;
    int32_t n_bad_index;        /* kept matches whose query / train index lies outside the two feature sets
                                   (skipped, never read; the reference would index out of bounds) */
    float min_distance;         /* min(100.0f, smallest distance), tracking.cpp:345-348 */
    double parallax;            /* ComputeParallax(last_kf, curr, good matches) (tracking.cpp:548-560): the sum
                                   over the kept matches with valid indices / n_good_matches; 0 when FEW_MATCHES */
    vx_pnp_result pnp;          /* as vx_pnp_ransac on the gathered pairs (ok = 0 when the call returned early) */
} vx_track_result;

/* tracking.h:27-29 + tracking.cpp:420-423: 50 / 30 / {-1 (auto), 20, 2.0, 0.99, 0x5EED} */
void vx_track_default_options(vx_track_options* o);
/* Device pointer of a slot's vx_keypoint rows (their count: vx_orb_slot_device's d_count).  &kp[0].x
 * with a stride of sizeof(vx_keypoint) = 20 bytes is a valid d_curr_xy below. */
int vx_orb_slot_keypoints(vx_ctx* ctx, int slot, const vx_keypoint** d_kp);
/* <- tracking.cpp:342-423, :449.  last_kf_id: a live keyframe of `map` (the query side of the matches;
 * VX_ERR_INVALID otherwise).  Current frame positions: row i = two floats at d_curr_xy + i *
 * curr_stride_bytes (20 for a slot's vx_keypoint rows, 8 for packed float2), *d_n_curr rows (device).
 * d_matches / d_n_matches: a device match list of at most cap_matches entries; d_matches == NULL: the
 * result of ctx's last vx_match_slots_async / vx_match_device_async (cap_matches ignored; VX_ERR_STATE
 * if nothing was matched).  intr4 (host): fx fy cx cy of the current frame, non-zero focal lengths;
 * opt->pnp.max_iterations <= 4096.  Enqueued on ctx's stream, which first waits (vx_stream_wait_ctx)
 * for the map context's stream when ctx is another context; no host synchronisation.  Uses buffers of
 * its own: vx_pnp_ransac / vx_essential_ransac may run before the fetch.
 * The ordering is one way: nothing makes a later edit of `map` (vx_dmap_*, a LocalBA write-back, a
 * call that grows its arrays or its id table) wait for this call's kernels on another context, so
 * fetch — or order the map's context after ctx with vx_stream_wait_ctx — before editing the map.
 * The call also brings the map's landmark id table up to date (host-side bookkeeping of the map
 * included), so, like every vx_dmap_* call, it must not run concurrently with another call on the
 * same map from another thread. */
int vx_track_pnp_async(vx_ctx* ctx, vx_dmap* map, uint64_t last_kf_id,
                       const float* d_curr_xy, int64_t curr_stride_bytes, const int32_t* d_n_curr,
                       const vx_match* d_matches, const int32_t* d_n_matches, int cap_matches,
                       const double* intr4, const vx_track_options* opt);
/* One device-to-host copy (result | pair_match | inlier_mask) and one synchronisation; `status` is
 * then set from the counts in the order of tracking.cpp:357, :402, :425, :441.  pair_match[k] = index
 * in the match list of pair k (ascending), inlier_mask[k] = solvePnPRansac's inlier flag of pair k;
 * either may be NULL.  VX_ERR_CAPACITY (with *out filled) if an array is given and n_pairs > cap_pairs. */
int vx_track_pnp_fetch(vx_ctx* ctx, vx_track_result* out, int32_t* pair_match, uint8_t* inlier_mask,
                       int cap_pairs);
/* Host-input form (what visionx::PnPTracker calls): the last keyframe's and the current frame's
 * descriptor rows (32 B each) and the current frame's positions (n_train float2) are staged and
 * uploaded in ONE copy, matched on the device as vx_match_knn2_ratio would (query = last keyframe,
 * `ratio`), and the match list goes straight into vx_track_pnp_async.  Completed by
 * vx_track_pnp_fetch; the matches themselves by vx_match_fetch, if wanted.  "async" as in: nothing
 * is waited for after the enqueue; the call may block at its start until the PREVIOUS call's upload
 * has left the pinned staging block it reuses (it has, once that call was fetched). */
int vx_track_pnp_host_async(vx_ctx* ctx, vx_dmap* map, uint64_t last_kf_id, const uint8_t* query_desc, int n_query,
                            const uint8_t* train_desc, int n_train, const float* curr_xy, float ratio,
                            const double* intr4, const vx_track_options* opt);
/* threads of the pair-gather workgroup (its compaction chunk; for tests of the chunk boundaries) */
int vx_track_block(void);

/* ---------------------------------------------------------------- map culling on the resident map (cull.hip)
 * <- Tracking::CullLandmarks (tracking.cpp:652-750), Tracking::CullKeyFrames (:775-840) and
 *    Tracking::RemoveKeyFrame (:752-773), what Tracking::CreateKeyFrame runs before LocalBA
 *    (:76-84): the decision (a reprojection of every observation of every landmark; a redundancy count
 *    over every keyframe's features) and the edit of the map's device arrays run in kernels, the
 *    culled lists come back with one synchronisation and the map's host mirrors follow them.  The map
 *    afterwards is the map the same decisions leave through vx_dmap_set_landmark_bad /
 *    vx_dmap_set_features / vx_dmap_remove_landmarks / vx_dmap_remove_observations /
 *    vx_dmap_remove_keyframe. */
typedef struct {                          /* Tracking::Options, "Map culling" (tracking.h:33-40) */
    int32_t min_landmark_observations;    /* 2 */
    int32_t min_landmarks_for_culling;    /* 200 */
    int32_t min_keyframes_for_culling;    /* 3 */
    int32_t max_keyframes;                /* 30 */
    int32_t kf_min_shared_observations;   /* 3 */
    int32_t reserved;
    double kf_redundant_ratio;            /* 0.9 */
    double landmark_max_reproj_error;     /* 5.0 */
} vx_cull_options;
void vx_cull_default_options(vx_cull_options* o);

/* why a landmark left, in the order CullLandmarks tests (tracking.cpp:666-722) */
#define VX_CULL_ALREADY_BAD 1       /* IsBad()                                         (:666) */
#define VX_CULL_FEW_OBSERVATIONS 2  /* ObservationCount() < min_landmark_observations  (:670) */
#define VX_CULL_NO_PROJECTION 3     /* no observation passed the checks of :681-701    (:713) */
#define VX_CULL_LARGE_ERROR 4       /* an error > 2 * landmark_max_reproj_error        (:707) */
#define VX_CULL_MEAN_ERROR 5        /* err_sum / cnt > landmark_max_reproj_error       (:719) */

typedef struct {
    uint64_t lm_id;
    int32_t row;                /* the landmark's row in the map (insertion order) */
    int32_t reason;             /* VX_CULL_* */
    int32_t n_projected;        /* observations projected when the decision fell (insertion order; the walk
                                   stops at the first large error, :709); 0 for ALREADY_BAD / FEW_OBSERVATIONS */
    int32_t reserved;
    double mean_err;            /* err_sum / cnt for MEAN_ERROR (summed in insertion order), else 0 */
} vx_cull_landmark;
typedef struct {                /* a feature reset to landmark_id_ = 0, has_landmark = false, is_outlier = true */
    uint64_t kf_id;
    int32_t kf_row;             /* the keyframe's row in the map */
    int32_t feat_idx;
} vx_cull_feature;

/* <- Tracking::CullLandmarks (tracking.cpp:652-750).  Nothing happens below min_landmarks_for_culling
 * live landmarks (:656).  Otherwise every live landmark is tested as :666-722 do (an observation's
 * keyframe is looked up among the live keyframes; is_outlier is not consulted) and the culled ones are
 * removed as :729-747 do: each observed feature whose landmark_id_ is the landmark's is reset (no
 * has_landmark check there), then Map::RemoveLandmark.  *n_landmarks landmarks left, *n_features
 * features were reset (either may be NULL); the lists: vx_dmap_cull_results.  Runs on ctx's stream (it
 * waits for the map context's stream first when ctx is another context) and synchronises once. */
int vx_dmap_cull_landmarks(vx_ctx* ctx, vx_dmap* map, const vx_cull_options* opt, int* n_landmarks, int* n_features);
/* The counts of Tracking::CullKeyFrames' loop (tracking.cpp:804-820) for every live keyframe in
 * ascending id: total[i] = its features with has_landmark, redundant[i] = those whose landmark is in
 * the map, not bad and has ObservationCount() >= kf_min_shared_observations.  No edit.  *n = live
 * keyframes; VX_ERR_CAPACITY (with *n set) when cap is smaller.  One synchronisation. */
int vx_dmap_keyframe_redundancy(vx_ctx* ctx, vx_dmap* map, const vx_cull_options* opt, int cap, uint64_t* kf_id,
                                int32_t* total, int32_t* redundant, int* n);
/* <- Tracking::CullKeyFrames (tracking.cpp:775-840).  Nothing happens at or below
 * min_keyframes_for_culling live keyframes (:781).  protect_ids: last_keyframe_, init_frame_ and the
 * current frame (:797-802; ids not in the map are ignored).  The first keyframe in ascending id with
 * ratio = double(redundant) / double(total) > kf_redundant_ratio && (exceeded || ratio > 0.95) (:826-827,
 * compared on the host in that expression) is removed as Tracking::RemoveKeyFrame does (:752-773:
 * RemoveObservation + reset for each of its has_landmark features whose landmark is in the map, the
 * others left as they are, then Map::RemoveKeyFrame), and CullLandmarks runs once more (:838, under
 * its own gate).  *removed 0 / 1, *removed_kf_id and *ratio of the removed keyframe, *n_landmarks /
 * *n_features as vx_dmap_cull_landmarks (the keyframe's own reset features included); outputs may be
 * NULL.  Two synchronisations when a keyframe is removed (the counts, then the lists), else one. */
int vx_dmap_cull_keyframes(vx_ctx* ctx, vx_dmap* map, const vx_cull_options* opt, const uint64_t* protect_ids,
                           int n_protect, int* removed, uint64_t* removed_kf_id, double* ratio, int* n_landmarks,
                           int* n_features);
/* The lists of the map's last vx_dmap_cull_landmarks / vx_dmap_cull_keyframes (host memory owned by
 * the map, filled before that call's last synchronisation, valid until the next vx_dmap_* edit; may be
 * read again, e.g. with larger arrays): *n_lm landmark records in ascending landmark row; *n_feat
 * feature records, the culled landmarks' in (landmark row, observation insertion order), then the
 * removed keyframe's own features in feature order.  Arrays may be NULL; VX_ERR_CAPACITY when an array
 * is given and its count exceeds its cap (the counts are set either way). */
int vx_dmap_cull_results(vx_dmap* map, int cap_lm, vx_cull_landmark* lm_records, int cap_feat,
                         vx_cull_feature* feat_records, int* n_lm, int* n_feat);
/* threads of a landmark-scan workgroup (for tests of its boundaries) and the keyframe count up to
 * which the scan keeps its keyframe table in LDS (above it the table is read from global memory) */
int vx_cull_block(void);
int vx_cull_lds_keyframes(void);

/* ---------------------------------------------------------------- keyframe creation on the resident map (keyframe.hip)
 * <- Tracking::CreateKeyFrame (tracking.cpp:577-584): CreateLandmarksFromDepth(curr) (:586-650), then
 *    TriangulateWithLastKeyFrame(last, curr) (:856-945, whose has_landmark test on the current side sees
 *    the depth landmarks just made), then Map::InsertKeyFrame (:581) — as one stream-ordered sequence
 *    over the resident map with one synchronisation.  The last keyframe's feature positions, flags,
 *    pose and intrinsics are read from the map's rows (after a LocalBA its pose is current only
 *    there), never passed in.  After a successful call the map is the map this sequence leaves:
 *      vx_dmap_add_landmarks     ids first_landmark_id + rank in creation order, bad = 0
 *      vx_dmap_add_observations  creation order: a depth landmark adds (kf_id, i); a triangulated one
 *                                (last_kf_id, queryIdx) then (kf_id, trainIdx) (:916-917)
 *      vx_dmap_set_features      last_kf_id's triangulated query features: id, has_landmark, not outlier
 *      vx_dmap_add_keyframe      kf_id with the final links (unlinked features: id 0, flags 0)
 *    device rows and host mirrors alike.  Creation order: the depth landmarks in feature order, then
 *    the triangulated ones in match order (the first passing match per train feature wins). */
typedef struct {
    double tri_min_angle_deg;      /* 1.0  triangulation_min_angle_deg (tracking.h:43) */
    double tri_max_reproj_error;   /* 5.0  triangulation_max_reproj_error (tracking.h:44) */
} vx_keyframe_options;
void vx_keyframe_default_options(vx_keyframe_options* o);

/* error_bits of vx_keyframe_result: why a call returned VX_ERR_INVALID and left the map as it was */
#define VX_KF_ERR_MATCH_RANGE 1   /* a match index outside either feature set (found on the device) */
#define VX_KF_ERR_DUP_QUERY 2     /* a repeated query index (found on the device) */
#define VX_KF_ERR_KF_LIVE 4       /* kf_id is already a live keyframe */
#define VX_KF_ERR_NO_LAST 8       /* last_kf_id is not a live keyframe */
#define VX_KF_ERR_NO_CAMERA 16    /* intr4 == NULL, or the last keyframe was inserted without a camera */
#define VX_KF_ERR_ID_RANGE 32     /* an id of [first_landmark_id, first_landmark_id + cap_feat) is in the map */

typedef struct {
    int32_t n_feat;                /* features of the new keyframe (the device-side count, clamped to cap_feat) */
    int32_t n_depth;               /* landmarks CreateLandmarksFromDepth made */
    int32_t n_triangulated;        /* landmarks TriangulateWithLastKeyFrame made */
    int32_t n_matches;             /* matches read (clamped to cap_matches; 0 without a last keyframe) */
    uint64_t first_landmark_id;
    uint64_t next_landmark_id;     /* first_landmark_id + n_depth + n_triangulated: the caller's landmark_id_ */
    int32_t error_bits;            /* VX_KF_ERR_* */
    int32_t reserved;
} vx_keyframe_result;

typedef struct {                   /* one created landmark */
    uint64_t lm_id;
    int32_t row;                   /* its row in the map */
    int32_t kind;                  /* 0 depth, 1 triangulated */
    int32_t feat_curr;             /* feature of the new keyframe */
    int32_t feat_last;             /* feature of the last keyframe (-1 for depth) */
    double pw[3];
} vx_keyframe_landmark;

/* The device-input form.  kf_id / pose7 (x y z w | t, T_cw) / intr4: the new keyframe.  Feature
 * positions: row i = two floats at d_xy + i * stride_bytes (20 for the vx_keypoint rows of an extraction
 * slot, vx_orb_slot_keypoints; 8 for packed float2), *d_n_feat rows (at most cap_feat), widened to
 * double exactly as Feature::position is made from cv::KeyPoint::pt.  has_last == 0 skips the
 * triangulation (the first frame of InitWithSecondFrame).  The match list Match(last, curr) (query =
 * last keyframe feature, train = new feature): d_matches == NULL = the result of ctx's last
 * vx_match_*_async (VX_ERR_STATE if none), else *d_n_matches rows (at most cap_matches).  d_depth:
 * device image of `rows` rows of `cols` VX_DEPTH_* elements, row_stride bytes apart; NULL =
 * Depth().empty().  Before enqueueing, every array of the map is grown for the worst case (cap_feat
 * features and landmarks, 2 cap_feat observations); after that no count comes from the host.  Runs on
 * ctx's stream (which first waits for the map context's stream when ctx is another context) and
 * synchronises once.  VX_ERR_INVALID with result->error_bits set leaves the map exactly as it was
 * (rows beyond the map's counts are scratch). */
int vx_dmap_create_keyframe(vx_ctx* ctx, vx_dmap* map, uint64_t kf_id, const double* pose7, const double* intr4,
                            const float* d_xy, int64_t stride_bytes, const int32_t* d_n_feat, int cap_feat,
                            int has_last, uint64_t last_kf_id, const vx_match* d_matches,
                            const int32_t* d_n_matches, int cap_matches, const void* d_depth, int depth_type,
                            int rows, int cols, int64_t row_stride, uint64_t first_landmark_id,
                            const vx_keyframe_options* opt, vx_keyframe_result* result);
/* The host-input form (what visionx::KeyFrameLandmarks::CreateKeyFrame calls): feat_uv = n_feat rows
 * of two doubles (Feature::position), a host match list and a host depth image (NULL = empty), staged
 * into one pinned block and uploaded in one copy; then the same sequence. */
int vx_dmap_create_keyframe_host(vx_ctx* ctx, vx_dmap* map, uint64_t kf_id, const double* pose7, const double* intr4,
                                 const double* feat_uv, int n_feat, int has_last, uint64_t last_kf_id,
                                 const vx_match* matches, int n_matches, const void* depth, int depth_type,
                                 int rows, int cols, int64_t row_stride, uint64_t first_landmark_id,
                                 const vx_keyframe_options* opt, vx_keyframe_result* result);
/* The records of the map's last vx_dmap_create_keyframe*, one per created landmark in creation order
 * (host memory owned by the map; empty after a rejected call).  `records` may be NULL;
 * VX_ERR_CAPACITY (with *n set) when it is given and *n > cap. */
int vx_dmap_create_results(vx_dmap* map, int cap, vx_keyframe_landmark* records, int* n);
/* A live keyframe's feature rows read back from the device: uv (2 doubles), lm_id, flags per feature;
 * any array may be NULL.  *n = its feature count; VX_ERR_CAPACITY when an array is given and *n > cap. */
int vx_dmap_keyframe_features(vx_dmap* map, uint64_t kf_id, int cap, double* uv, uint64_t* lm_id, uint8_t* flags,
                              int* n);
/* threads of the commit workgroup (the chunk of its two ordered compactions; for tests of the boundaries) */
int vx_keyframe_block(void);

/* <- E = cv::findEssentialMat(pts_last, pts_curr, K, cv::RANSAC, 0.999, 1.0, mask);
 *    inliers = cv::recoverPose(E, pts_last, pts_curr, K, R, t, mask)
 *    in Tracking::EstimatePoseByEssential (tracking.cpp:503-547).
 * Same device strategy as vx_pnp_ransac: every hypothesis (5 correspondences from a splitmix64
 * stream) is solved by the five-point method (up to 10 E, all scored by Sampson error) at once, and
 * the sequential RANSAC loop is replayed over the per-model inlier counts; the kept E is decomposed
 * (E = U diag V^T; R1 = U W V^T, R2 = U W^T V^T, t = U e3) and the four (R, +-t) are scored by DLT
 * triangulation of the RANSAC inliers (positive depth below distance_thresh in both views), OpenCV's
 * tie order.  Parity against OpenCV is unpinned (its cv::RNG stream); DESIGN.md §14. */
typedef struct {
    int32_t max_iterations;    /* findEssentialMat maxIters (OpenCV default 1000), <= 4096 */
    int32_t reserved;
    double threshold;          /* px (tracking.cpp:521: 1.0); divided by (fx + fy) / 2 */
    double confidence;         /* prob (0.999) */
    double distance_thresh;    /* recoverPose's triangulated-depth limit (50) */
    uint64_t seed;             /* hypothesis stream */
} vx_essential_options;
typedef struct {
    int32_t ok;                /* !E.empty() */
    int32_t n_inliers;         /* recoverPose's return value: RANSAC inliers in front of both views */
    int32_t n_ransac_inliers;  /* findEssentialMat's mask count */
    int32_t best_hypothesis, best_model, hypotheses_run;
    int32_t pose_candidate;    /* 0: (R1, t) 1: (R2, t) 2: (R1, -t) 3: (R2, -t) */
    int32_t reserved;
    double E[9];               /* row-major, unit Frobenius norm, x_curr^T E x_last = 0 (normalised) */
    double R[9], t[3];         /* T_cl: x_curr = R x_last + t, |t| = 1 (recoverPose's R, t) */
} vx_essential_result;
void vx_essential_default_options(vx_essential_options* out);
/* pts_last / pts_curr: 2 floats per match (cv::Point2f, tracking.cpp:506-514); mask (n bytes, may
 * be NULL) = recoverPose's output mask. */
int vx_essential_ransac(vx_ctx* ctx, const float* pts_last, const float* pts_curr, int n, const double* intr4,
                        const vx_essential_options* opt, uint8_t* mask, vx_essential_result* out);
int vx_essential_ransac_batch(vx_ctx* ctx, int n_problems, const int32_t* offsets, const float* pts_last,
                              const float* pts_curr, const double* intr4, const vx_essential_options* opt,
                              uint8_t* mask, vx_essential_result* out);

/* ---------------------------------------------------------------- TrackLastFrame on the device (track_ess.hip)
 * <- Tracking::TrackLastFrame after Match(last_frame, curr) (tracking.cpp:281-330) and the same
 *    sequence at the head of Tracking::InitWithSecondFrame (:207-245): the distance filter (:291-304),
 *    the cv::Point2f pairs (:509-514), findEssentialMat + recoverPose (:521-528), T_cl * T_lw
 *    (:539-541) and ComputeParallax (:325, :548-560) as ONE stream-ordered sequence over data that is
 *    already on the device — the match list and both frames' keypoints — with one synchronisation, in
 *    the fetch.  No map is involved.
 *    T_cl * T_lw (Sophus::SE3d): q_cl from R by Shepperd's method (Eigen::Quaterniond(Matrix3d)),
 *    q = q_cl (x) q_lw (Hamilton product), q *= 2 / (1 + |q|^2) when |q|^2 != 1 (Sophus's first-order
 *    renormalisation), t = R(q_cl) t_lw + t_cl.  Parity with Sophus itself is unpinned. */
typedef struct {
    int32_t min_matches;        /* Tracking::Options::min_matches 50 (tracking.cpp:306) */
    int32_t min_inliers;        /* Tracking::Options::min_inliers 30 (tracking.cpp:317, :530) */
    vx_essential_options ess;   /* vx_essential_default_options */
} vx_track_essential_options;

#define VX_TRACK_ESSENTIAL_FAILED 5 /* !ess.ok || ess.n_inliers < min_inliers (tracking.cpp:317, :523, :530) */

typedef struct {
    int32_t status;             /* VX_TRACK_OK, VX_TRACK_FEW_MATCHES or VX_TRACK_ESSENTIAL_FAILED */
    int32_t n_matches, n_good_matches, n_pairs;
    int32_t n_bad_index;        /* kept matches whose query / train index lies outside the two feature sets
                                   (skipped, never read; the reference would index out of bounds) */
    float min_distance;         /* min(100.0f, smallest distance), tracking.cpp:294-297 */
    double parallax;            /* ComputeParallax(last, curr, kept matches) over the float positions: the sum
                                   over the kept matches with valid indices / n_good_matches; 0 when FEW_MATCHES */
    double pose[7];             /* T_cw = T_cl * T_lw (qx qy qz qw tx ty tz); zero when !ess.ok */
    vx_essential_result ess;    /* as vx_essential_ransac on the pairs (ok = 0 when the call returned early) */
} vx_track_essential_result;

/* tracking.h:27-28 + tracking.cpp:521: 50 / 30 / vx_essential_default_options */
void vx_track_essential_default_options(vx_track_essential_options* o);
/* <- tracking.cpp:291-325, :509-541.  Positions of both frames as vx_track_pnp_async takes the current
 * frame's: row i = two floats at d_*_xy + i * stride (20 for a slot's vx_keypoint rows, 8 for packed
 * float2), *d_n_* rows (device).  The match list (query = last frame, train = current frame) as in
 * vx_track_pnp_async: d_matches == NULL means the result of ctx's last vx_match_slots_async /
 * vx_match_device_async (VX_ERR_STATE if nothing was matched).  pose_last7 (host): T_lw as qx qy qz qw
 * tx ty tz, NULL = identity; intr4 (host): fx fy cx cy, non-zero focal lengths;
 * opt->ess.max_iterations <= 4096.  Enqueued on ctx's stream; no host synchronisation.  Uses buffers
 * of its own: a vx_track_pnp_* pair, vx_pnp_ransac or vx_essential_ransac may run before the fetch,
 * and a PnP track and an essential track may be in flight together. */
int vx_track_essential_async(vx_ctx* ctx, const float* d_last_xy, int64_t last_stride_bytes, const int32_t* d_n_last,
                             const float* d_curr_xy, int64_t curr_stride_bytes, const int32_t* d_n_curr,
                             const vx_match* d_matches, const int32_t* d_n_matches, int cap_matches,
                             const double* pose_last7, const double* intr4, const vx_track_essential_options* opt);
/* Host-input form (what visionx::EssentialTracker calls): both frames' descriptor rows (32 B each) and
 * float2 positions are staged and uploaded in ONE copy, matched on the device (query = last frame,
 * `ratio`) and fed straight into vx_track_essential_async.  May block at its start until the PREVIOUS
 * call's upload has left the pinned staging block it reuses, as vx_track_pnp_host_async. */
int vx_track_essential_host_async(vx_ctx* ctx, const uint8_t* last_desc, int n_last, const float* last_xy,
                                  const uint8_t* curr_desc, int n_curr, const float* curr_xy, float ratio,
                                  const double* pose_last7, const double* intr4,
                                  const vx_track_essential_options* opt);
/* One device-to-host copy (result | pair_match | mask) and one synchronisation; `status` is then set
 * in the order of tracking.cpp:306, :317.  pair_match[k] = index in the match list of pair k
 * (ascending), mask[k] = recoverPose's output mask of pair k; either may be NULL.  VX_ERR_CAPACITY
 * (with *out filled) if an array is given and n_pairs > cap_pairs. */
int vx_track_essential_fetch(vx_ctx* ctx, vx_track_essential_result* out, int32_t* pair_match, uint8_t* mask,
                             int cap_pairs);

/* ---------------------------------------------------------------- InitWithFirstFrame's gates on the device (init_gate.hip)
 * <- Tracking::InitWithFirstFrame (tracking.cpp:177-204): the feature count (:179),
 *    CheckFeatureDistribution's occupancy grid over the keypoints (:93-118) and CheckImageQuality's
 *    cvtColor(BGR2GRAY) + meanStdDev bounds (:120-139), as two launches over an image and keypoints
 *    that are already on the device, with one synchronisation, in the fetch.
 *    Gray is vx_orb_extract's fixed-point level 0; the sums are integers, so the record is bitwise
 *    repeatable.  mean = sum * (1.0 / N), stddev = sqrt(max(sum_sq * (1.0 / N) - mean * mean, 0)) with
 *    every operation rounded on its own (meanStdDev's arithmetic: the reciprocal, no fused multiply-add).
 *    Deviation: cvtColor asserts 3 or 4 channels, so the reference throws on a gray image; here a
 *    1-channel image is its own gray level, as in vx_orb_extract. */
typedef struct {              /* Tracking::InitWithFirstFrame, tracking.cpp:177-204 */
    int32_t min_features;     /* Tracking::Options::min_matches (:179), default 50 */
    int32_t grid_cols, grid_rows;   /* 5, 5 (:96-97); grid_cols * grid_rows in 1..32 */
    double min_grid_frac;     /* 0.5 (:117); at byte 16 */
    double min_mean, max_mean, min_stddev;   /* 30, 225, 20 (:129-135) */
} vx_init_gate_options;

/* status of vx_init_gate_result: the first gate that fails, in the reference's order */
#define VX_INIT_OK 0
#define VX_INIT_FEW_FEATURES 1        /* n_features < min_features                          (tracking.cpp:179) */
#define VX_INIT_POOR_DISTRIBUTION 2   /* valid_grids < cols * rows * min_grid_frac (double) (tracking.cpp:117) */
#define VX_INIT_POOR_IMAGE 3          /* mean < min_mean || mean > max_mean || stddev < min_stddev (:129-135) */

typedef struct {
    int32_t status;             /* VX_INIT_*; every field below is filled whichever gate failed */
    int32_t n_features;         /* min(*d_n_feat, cap_feat) */
    int32_t valid_grids;        /* occupied cells (:109-114) */
    uint32_t grid_mask;         /* bit col * grid_rows + row set: grid[col][row] (:105) */
    int64_t n_pixels;           /* width * height */
    uint64_t sum, sum_sq;       /* over the gray level-0 pixels */
    double mean, stddev;        /* meanStdDev (:126) */
} vx_init_gate_result;

/* tracking.h:27, tracking.cpp:96-97, :117, :129-135: 50 / 5 x 5 / 0.5 / 30, 225, 20 */
void vx_init_gate_default_options(vx_init_gate_options* o);
/* <- tracking.cpp:179-197.  d_img: the device image vx_orb_extract_async takes (channels 1, 3 (BGR) or
 * 4 (BGRA), row_stride >= width * channels, any base alignment); it is read itself, so the call does
 * not depend on what was last extracted on ctx.  Keypoints as vx_track_essential_async takes them:
 * row i = two floats at d_xy + i * xy_stride_bytes (20 for a slot's vx_keypoint rows from
 * vx_orb_slot_keypoints, 8 for packed float2), min(*d_n_feat, cap_feat) rows.  d_xy may be NULL when
 * cap_feat is 0.  Enqueued on ctx's stream; no host synchronisation.  VX_ERR_INVALID for a null
 * pointer, non-positive geometry, channels outside {1, 3, 4}, a short stride or grid_cols * grid_rows
 * outside 1..32. */
int vx_init_gate_async(vx_ctx* ctx, const uint8_t* d_img, int width, int height, int channels, int64_t row_stride,
                       const float* d_xy, int64_t xy_stride_bytes, const int32_t* d_n_feat, int cap_feat,
                       const vx_init_gate_options* opt);
/* Host-input form (what visionx::Tracking calls): the image rows and the positions are staged and
 * uploaded in ONE copy, then as vx_init_gate_async.  May block at its start until the PREVIOUS call's
 * upload has left the pinned staging block it reuses, as vx_track_essential_host_async. */
int vx_init_gate_host_async(vx_ctx* ctx, const uint8_t* img, int width, int height, int channels, int64_t row_stride,
                            const float* xy, int64_t xy_stride_bytes, int n_feat, const vx_init_gate_options* opt);
/* One device-to-host copy of the record and one synchronisation.  VX_ERR_STATE when nothing was enqueued. */
int vx_init_gate_fetch(vx_ctx* ctx, vx_init_gate_result* out);

/* ---------------------------------------------------------------- device-resident frames (frame.hip)
 * <- what a visionx::Frame keeps of ORBExtractor::Extract (orb_extractor.cpp:13-24: keypoints_ and
 *    descriptors_, frame.h:16-40) held on the device for as long as the frame lives.  An extraction
 *    slot belongs to its context and is overwritten by the next extraction into it; a vx_frame is a
 *    block of its own:
 *        int32 count[4] {n, overflow, 0, 0} | vx_keypoint rows[cap] | descriptor rows[cap] (32 B each)
 *    (the layout of a slot's count; the row arrays start on 16-byte boundaries).  n <= cap always:
 *    `overflow` is set when the source held more rows than cap, and the first cap of them are kept.
 *    The handle is bound to the device of the context it was created on and may be read by every
 *    context of that device (order the reader after the writer with vx_stream_wait_ctx /
 *    vx_event_wait).  Destroying a frame waits for the device (hipFree). */
typedef struct vx_frame vx_frame;
int vx_frame_create(vx_ctx* ctx, int cap, vx_frame** out);   /* cap >= 1 */
void vx_frame_destroy(vx_frame* frame);
/* <- orb_extractor.cpp:19-24 (the copy out of detectAndCompute's outputs).  One launch of
 * k_frame_capture on ctx's stream: min(n_slot, cap) keypoint and descriptor rows of `slot` (a valid
 * extraction slot of ctx) and its count into `frame`; overflow = n_slot > cap or the slot's own
 * overflow flag.  Nothing synchronises: the count is read on the device. */
int vx_frame_capture_async(vx_ctx* ctx, int slot, vx_frame* frame);
/* <- ORBExtractor::Extract (orb_extractor.cpp:8-25) into a frame: the host image (as vx_orb_extract
 * takes it) is staged in pinned memory and uploaded, extracted into slot VX_MAX_SLOTS - 1 of ctx and
 * captured.  The frame then holds vx_orb_extract's keypoints and descriptors, byte for byte.
 * Nothing is waited for after the enqueue; the call may block at its start until the PREVIOUS
 * vx_frame_extract_host_async / vx_frame_upload_async on ctx has left the pinned staging block. */
int vx_frame_extract_host_async(vx_ctx* ctx, vx_frame* frame, const vx_orb_params* params, const uint8_t* img,
                                int width, int height, int channels, int64_t row_stride);
/* Features that came from elsewhere (a replay extractor): n float2 positions and n 32-byte rows from
 * the host, staged and uploaded in ONE copy.  The keypoint rows' response, angle and octave are zero.
 * VX_ERR_CAPACITY when n > cap.  xy / desc may be NULL when n is 0. */
int vx_frame_upload_async(vx_ctx* ctx, vx_frame* frame, const float* xy, const uint8_t* desc, int n);
/* The pointers the device-input forms take: &kp[0].x with *stride_bytes = sizeof(vx_keypoint) = 20 is a
 * valid d_*_xy of vx_track_pnp_async / vx_track_essential_async / vx_init_gate_async /
 * vx_dmap_create_keyframe; d_desc / d_count / cap go to vx_match_device_async.  Any output may be
 * NULL.  Stable for the life of the frame. */
int vx_frame_device(const vx_frame* frame, const float** d_xy, int64_t* stride_bytes, const uint8_t** d_desc,
                    const int32_t** d_count, int32_t* cap);
/* One device-to-host copy (count | keypoint rows [| descriptor rows]) and one synchronisation of ctx's
 * stream.  kp and desc may each be NULL; with desc == NULL the descriptor rows are not copied.
 * VX_ERR_CAPACITY with *n_out set when n > cap, as vx_orb_fetch.  vx_frame_fetch_ex also returns the
 * frame's overflow flag (*overflow, may be NULL). */
int vx_frame_fetch(vx_ctx* ctx, const vx_frame* frame, vx_keypoint* kp, uint8_t* desc, int cap, int* n_out);
int vx_frame_fetch_ex(vx_ctx* ctx, const vx_frame* frame, vx_keypoint* kp, uint8_t* desc, int cap, int* n_out,
                      int* overflow);

/* ---------------------------------------------------------------- Tracking::Track() on the device (track_frame.hip)
 * <- Tracking::Track (tracking.cpp:267-279): TrackWithPnP against the last keyframe (:269-273) and,
 *    when it fails, TrackLastFrame against the last frame (:278), over device-resident frames as ONE
 *    stream-ordered sequence with one synchronisation, in the fetch — whichever path sets the pose:
 *
 *      Match(last_kf, curr) -> vx_track_pnp_async's chain -> k_track_gate
 *                           -> Match(last, curr) -> vx_track_essential_async's chain -> k_track_final
 *
 *    k_track_gate evaluates vx_track_pnp_fetch's status rule (tracking.cpp:357, :402, :425, :441) on the
 *    device and writes the query count the fallback's match and pair kernels read: the last frame's
 *    count when PnP failed (or there is no last keyframe), 0 when it succeeded.  With the gate closed
 *    the fallback's kernels run as empty launches: no RANSAC hypothesis runs, and the essential record
 *    is byte for byte what vx_track_essential_async leaves on an empty match list. */
#define VX_TRACK_PATH_NONE 0       /* Track() returned false: the pose was not set */
#define VX_TRACK_PATH_PNP 1        /* TrackWithPnP set it (tracking.cpp:443-447) */
#define VX_TRACK_PATH_ESSENTIAL 2  /* TrackLastFrame set it (tracking.cpp:539-541) */

typedef struct {
    int32_t path;               /* VX_TRACK_PATH_* */
    int32_t status;             /* VX_TRACK_OK, or the status of the last path that ran */
    int32_t n_inliers;          /* of `path`: pnp.pnp.n_inliers or ess.ess.n_inliers; 0 for PATH_NONE */
    int32_t n_keypoints;        /* the current frame's keypoint count */
    double parallax;            /* of `path`: pnp.parallax or ess.parallax; 0 for PATH_NONE */
    double pose[7];             /* of `path`: pnp.pnp.pose or ess.pose (T_cl * T_lw), copied; 0 for PATH_NONE */
    int32_t pnp_ran;            /* last_kf was given */
    int32_t ess_ran;            /* the gate was open and `last` was given */
    vx_track_result pnp;        /* as vx_track_pnp_fetch returns it (status included); zero when !pnp_ran */
    vx_track_essential_result ess; /* as vx_track_essential_fetch returns it: of the fallback when ess_ran,
                                      otherwise of an empty match list (n_matches 0, min_distance 100, ess.ok 0) */
} vx_track_frame_result;

/* <- tracking.cpp:267-330 + :332-455.  last_kf: the last keyframe's frame (its rows are the features of
 * keyframe last_kf_id of `map`), NULL: no last keyframe, straight to TrackLastFrame (:269).  last: the
 * last frame, NULL: the fallback fails (:282).  They may be the same handle (the second match is then
 * the first list's, gated); at least one must be given.  pose_last7 (host): T_lw of `last`, NULL =
 * identity (InitWithSecondFrame's head, :207-232, is this call with last_kf = NULL and pose_last7 =
 * NULL).  ratio: the matcher's nn_ratio for both matches.  Options and intr4 as in vx_track_pnp_async /
 * vx_track_essential_async.  VX_ERR_INVALID for a null argument, a frame of another device, a keyframe
 * that is not in the map or bad options.
 * Ordering: as vx_track_pnp_async towards the map (ctx's stream first waits for the map context's).
 * Frames written on another context: order ctx after it first (vx_stream_wait_ctx), never the host.
 * Buffers: the call owns both of its match lists and its packed result; the pair and RANSAC scratch
 * is vx_track_pnp_async's and vx_track_essential_async's (it runs those two calls on ctx, so their
 * own fetches afterwards see this call's paths).  Everything is stream-ordered and the result is
 * complete once k_track_final has run, so any call on ctx except another vx_track_frame_async may
 * run between the enqueue and the fetch (vx_pnp_ransac, vx_essential_ransac, vx_match_*, ...). */
int vx_track_frame_async(vx_ctx* ctx, vx_dmap* map, uint64_t last_kf_id, const vx_frame* last_kf,
                         const vx_frame* last, const vx_frame* curr, float ratio, const double* pose_last7,
                         const double* intr4, const vx_track_options* pnp_opt,
                         const vx_track_essential_options* ess_opt);
/* One device-to-host copy of one packed block (result | both paths' pair_match and mask arrays | the
 * current frame's keypoint rows when curr_kp is given) and one synchronisation.  curr_kp (may be NULL):
 * the current frame's keypoint rows, *n_kp their count; VX_ERR_CAPACITY (with *out and *n_kp filled)
 * when the count exceeds cap_kp.  The pair arrays: vx_track_frame_pairs, after the fetch. */
int vx_track_frame_fetch(vx_ctx* ctx, vx_track_frame_result* out, vx_keypoint* curr_kp, int cap_kp, int* n_kp);
/* The fetched block's pair arrays of path `which` (0: PnP, 1: essential): pair_match[k] and mask[k] as
 * vx_track_pnp_fetch / vx_track_essential_fetch return them (either may be NULL).  No device work.
 * VX_ERR_STATE before a fetch, VX_ERR_CAPACITY when that path's n_pairs > cap_pairs. */
int vx_track_frame_pairs(vx_ctx* ctx, int which, int32_t* pair_match, uint8_t* mask, int cap_pairs);
/* The device match list of the PnP match (which = 0: query = last_kf) or the fallback match (1: query =
 * last; empty when the gate was closed), e.g. for vx_dmap_create_keyframe (tracking.cpp:340 and :863
 * match the same two frames).  Valid until the next vx_track_frame_async on ctx.  VX_ERR_STATE when
 * that match was not enqueued (which = 0 without a last keyframe). */
int vx_track_frame_matches(vx_ctx* ctx, int which, const vx_match** d_matches, const int32_t** d_n, int32_t* cap);

/* <- Tracking::CreateKeyFrame (tracking.cpp:577-584) over a resident frame: vx_dmap_create_keyframe with
 * the frame's device positions (vx_frame_device) and a HOST depth image (NULL / rows 0: none), which is
 * staged and uploaded in one copy per keyframe.  d_matches: a device list (vx_track_frame_matches: the
 * track's own Match(last keyframe, current), tracking.cpp:340 and :863 being the same two frames), or
 * NULL for ctx's last vx_match_*_async result.  Everything else as vx_dmap_create_keyframe. */
int vx_dmap_create_keyframe_frame(vx_ctx* ctx, vx_dmap* map, uint64_t kf_id, const double* pose7, const double* intr4,
                                  const vx_frame* curr, int has_last, uint64_t last_kf_id, const vx_match* d_matches,
                                  const int32_t* d_n_matches, int cap_matches, const void* depth, int depth_type, int rows,
                                  int cols, int64_t row_stride, uint64_t first_landmark_id,
                                  const vx_keyframe_options* opt, vx_keyframe_result* result);

/* The frames 0 .. n_frames - 1 of batch bank `bank` (vx_orb_extract_batch_async) into n_frames handles
 * in ONE launch of k_frame_capture_batch on ctx's stream (frame = grid y).  Each handle then holds
 * what vx_frame_capture_async would have written from a slot with that frame's rows: count, overflow
 * flag and rows, clamped to the handle's capacity.  Nothing synchronises.  VX_ERR_STATE when the
 * bank holds fewer frames; VX_ERR_INVALID for a null / foreign-device / repeated handle. */
int vx_frame_capture_batch_async(vx_ctx* ctx, int bank, int n_frames, vx_frame* const* frames);

/* ---------------------------------------------------------------- Track() for a rig (track_rig.hip)
 * <- Tracking::Track (tracking.cpp:267-279) for ALL cameras of a rig time step over one shared map as
 *    ONE stream-ordered sequence and ONE synchronisation; every camera takes its own path (PnP,
 *    fallback or neither), decided on the device:
 *
 *      Match(last_kf_i, curr_i) for all i  -> k_rig_pairs -> k_rig_pack -> k_pnp_* (P = cameras) -> k_rig_gate
 *      Match(last_i, curr_i) under the gates -> k_rig_epairs -> k_rig_pack -> k_em_* (P = cameras)
 *                                            -> k_rig_epose -> k_rig_final
 *
 *    The number of launches does not depend on the number of cameras.  Camera i's results are byte
 *    for byte what vx_track_frame_async + vx_track_frame_fetch give for it alone. */
#define VX_MAX_RIG_CAMERAS 16            /* = VX_MAX_MATCH_PAIRS */
typedef struct {
    uint64_t last_kf_id;                 /* keyframe of `map` whose features are last_kf's rows */
    const vx_frame* last_kf;             /* NULL: this camera has no last keyframe (tracking.cpp:269) */
    const vx_frame* last;                /* NULL: this camera's fallback fails (:282) */
    const vx_frame* curr;
    const double* pose_last7;            /* host; NULL = identity */
    const double* intr4;                 /* host */
} vx_rig_camera;

/* One map, one ratio and one pair of option structs serve the whole rig; per camera the semantics,
 * argument checks and ordering rules are vx_track_frame_async's (a camera needs `curr` and at least one
 * of last_kf / last; last_kf == last is allowed: the fallback match is then run again under the gate,
 * which gives list 0's rows and count when the gate is open).  n_cams in [1, VX_MAX_RIG_CAMERAS].
 * Buffers: the call owns all of its buffers (match lists, pair and RANSAC scratch, packed result), so
 * vx_track_frame_async, vx_track_pnp_async, vx_track_essential_async and the RANSAC entry points may
 * run on ctx between the enqueue and the fetch, and a rig call between theirs.  May block at its start
 * until the PREVIOUS vx_track_rig_async's argument table has left the pinned staging it reuses. */
int vx_track_rig_async(vx_ctx* ctx, vx_dmap* map, int n_cams, const vx_rig_camera* cams, float ratio,
                       const vx_track_options* pnp_opt, const vx_track_essential_options* ess_opt);
/* One device-to-host copy of one packed block and one synchronisation for all cameras.  Camera i's part
 * has vx_track_frame_fetch's layout (result | pair_match0 | mask0 | pair_match1 | mask1 | keypoint rows)
 * at the offset vx_track_rig_layout returns for the call's capacities.  out: cap_cams records (NULL with
 * cap_cams 0: counts only), *n_cams (may be NULL) the number of cameras; VX_ERR_CAPACITY when cap_cams is
 * smaller.  with_keypoints = 0: the copy ends before the LAST camera's keypoint rows and
 * vx_track_rig_keypoints is not available afterwards. */
int vx_track_rig_fetch(vx_ctx* ctx, int with_keypoints, vx_track_frame_result* out, int cap_cams, int* n_cams);
/* As vx_track_frame_pairs for camera `cam` of the fetched block.  No device work. */
int vx_track_rig_pairs(vx_ctx* ctx, int cam, int which, int32_t* pair_match, uint8_t* mask, int cap_pairs);
/* Camera cam's current-frame keypoint rows, a host copy out of the fetched block.  VX_ERR_CAPACITY
 * (with *n set) when the count exceeds cap. */
int vx_track_rig_keypoints(vx_ctx* ctx, int cam, vx_keypoint* kp, int cap, int* n);
/* As vx_track_frame_matches for camera `cam`: the device list for vx_dmap_create_keyframe[_frame].
 * Valid until the next vx_track_rig_async on ctx. */
int vx_track_rig_matches(vx_ctx* ctx, int cam, int which, const vx_match** d_matches, const int32_t** d_n, int32_t* cap);
/* The packed block's layout (pure host function, no context): camera i's part, sized by its pair
 * capacities of the two paths and its keypoint capacity (each >= 0), starts at cam_offset[i] (16-byte
 * aligned, ascending, parts disjoint); *total_bytes is the end of the last part.  Inside a part the
 * offsets are vx_track_frame_fetch's.  VX_ERR_INVALID for n_cams outside [1, VX_MAX_RIG_CAMERAS], a
 * null array or a negative capacity. */
int vx_track_rig_layout(int n_cams, const int32_t* cap_pairs0, const int32_t* cap_pairs1, const int32_t* cap_kp,
                        int64_t* cam_offset, int64_t* total_bytes);
/* The fetched block itself (host memory, valid until the next fetch) and the capacities it was laid
 * out with (each array cap_cams entries, any may be NULL): what a binding slices with
 * vx_track_rig_layout.  VX_ERR_STATE before a fetch. */
int vx_track_rig_block(vx_ctx* ctx, const uint8_t** block, int64_t* bytes, int32_t* cap_pairs0, int32_t* cap_pairs1,
                       int32_t* cap_kp, int cap_cams);

/* ---------------------------------------------------------------- CreateKeyFrame for a rig (keyframe_rig.hip)
 * <- Tracking::CreateKeyFrame (tracking.cpp:577-584) for every camera of a rig time step that inserts a
 *    keyframe, over one shared map: ONE upload (argument table + all depth images), one memset, four
 *    launches (k_rig_kf_feat -> k_rig_kf_match -> k_rig_kf_count -> k_rig_kf_commit) and ONE
 *    synchronisation whatever the number of cameras.  The map, the results and the records are those of
 *    n_cams vx_dmap_create_keyframe_frame calls in camera order: camera i + 1's first_landmark_id is
 *    camera i's next_landmark_id, its rows follow camera i's.
 *
 *    All or nothing: when any camera's error word is set nothing is committed, every results[i]
 *    carries its own error_bits (0 for a camera without a fault) and the call returns VX_ERR_INVALID.
 *    Besides the single call's refusals, checked per camera, the call refuses what would make the
 *    cameras depend on one another: a kf_id or a last_kf_id named by two cameras (VX_KF_ERR_RIG_REPEAT
 *    on each of them), and a last_kf_id that is not live BEFORE the call, another camera's new kf_id
 *    included (VX_KF_ERR_NO_LAST).  The id range checked against the map is the call's,
 *    [first_landmark_id, first_landmark_id + the sum of the frames' capacities): VX_KF_ERR_ID_RANGE is
 *    set on every camera.  A has_last camera without a device match list is VX_ERR_INVALID (no bits). */
/* the rig call's own bit, 64, after the six of vx_keyframe_result above */
#define VX_KF_ERR_RIG_REPEAT (1 << 6) /* this camera's kf_id or last_kf_id is named by another camera of the call */
typedef struct {
    uint64_t kf_id;                      /* the new keyframe */
    const double* pose7;                 /* host: x y z w | t, T_cw */
    const double* intr4;                 /* host */
    const vx_frame* curr;                /* its resident frame */
    int32_t has_last;
    uint64_t last_kf_id;                 /* a live keyframe of the map no other camera of the call names */
    const vx_match* d_matches;           /* device (vx_track_rig_matches(cam, 0)); required when has_last */
    const int32_t* d_n_matches;
    int32_t cap_matches;
    const void* depth;                   /* HOST image, NULL = empty (Depth().empty(), tracking.cpp:591-594) */
    int32_t depth_type, rows, cols;
    int64_t row_stride;
} vx_rig_keyframe;
/* n_cams in [1, VX_MAX_RIG_CAMERAS]: the cameras that create a keyframe this step.  results: n_cams
 * records.  vx_dmap_create_results afterwards returns all cameras' records concatenated in camera order
 * (creation order); camera i's slice follows from the results' counts.  A context other than the map's
 * waits for the map's stream first.  May block at its start until the previous create call's upload has
 * left the pinned staging it reuses. */
int vx_dmap_create_keyframes_rig(vx_ctx* ctx, vx_dmap* map, int n_cams, const vx_rig_keyframe* cams,
                                 uint64_t first_landmark_id, const vx_keyframe_options* opt,
                                 vx_keyframe_result* results);

/* ---------------------------------------------------------------- relocalisation (reloc.hip)
 * <- Tracking::TrackWithPnP (tracking.cpp:332-455) against the landmarks of up to 16 keyframes at once: what
 *    HandleTrackingBad / HandleTrackingLost (tracking.cpp:477-499) leave as a TODO ("for now just
 *    re-initialise", after map_->removeAll()).  ONE correspondence set is built from all candidates and ONE
 *    PnP is solved on it, so a landmark the current frame does not see through one keyframe is found
 *    through another; one stream-ordered sequence, one synchronisation, a launch count that does not
 *    depend on the number of candidates:
 *
 *      Match(kf_c, curr) for all c -> k_reloc_pairs -> k_reloc_pool -> k_pnp_* (P = 1) -> k_reloc_final
 *
 *    Per candidate c (the caller's order): Match(kf_c, curr) with `ratio`, the distance filter (:342-355)
 *    and the pair list by the rules of :373-400 — exactly what vx_track_pnp_async builds.  A candidate is
 *    OPEN when n_good_matches >= min_matches (:357); closed candidates contribute nothing.
 *    Pool: the open candidates' pairs concatenated, candidate-major, in pair order inside a candidate.  Of
 *    all pairs that name the same current feature (train_idx) exactly one is kept: the smallest match
 *    distance wins, ties go to the lower candidate index, further ties to the lower pair index.  The
 *    survivors keep the concatenation order; pool_cand / pool_match (index into that candidate's match
 *    list) / pool_train give each survivor's origin.  Two different current features that claim the same
 *    landmark are left to RANSAC.
 *    Solve: n_pool < min_inliers is FEW_PAIRS and PnP does not run.  Otherwise solvePnPRansac as
 *    TrackWithPnP calls it: max_iterations < 0 = min(100, 2 * n_pool), resolved on the device; the seed,
 *    the LM refit and the gates (:425, :441) of vx_track_pnp_*.
 *    Consequence: with one candidate and no repeated train_idx the pooled arrays are TrackWithPnP's own,
 *    and the PnP record and the mask are vx_track_pnp_fetch's byte for byte. */
#define VX_MAX_RELOC_CANDIDATES 16          /* = VX_MAX_MATCH_PAIRS */
typedef struct {
    uint64_t kf_id;                      /* a live keyframe of `map` ... */
    const vx_frame* frame;               /* ... whose features are this frame's rows */
} vx_reloc_candidate;
typedef struct {
    int32_t n_matches, n_good_matches, n_pairs, n_bad_index;   /* as vx_track_pnp_fetch reports them for Match(kf_c, curr) */
    int32_t open;            /* n_good_matches >= min_matches (:357) */
    int32_t n_kept;          /* pairs of this candidate that survive the pool */
    int32_t n_inliers;       /* pooled inliers that came from this candidate */
    float   min_distance;
    double  parallax;        /* ComputeParallax(kf_c, curr, good matches), as vx_track_result.parallax */
} vx_reloc_candidate_result;
typedef struct {
    int32_t status;          /* VX_TRACK_OK | FEW_MATCHES (no candidate open) | FEW_PAIRS (n_pool < min_inliers) | PNP_FAILED | BAD_ROTATION */
    int32_t n_cand, n_pool, best_cand;      /* best_cand: most n_inliers, ties -> lower index; -1 unless OK */
    double  parallax;        /* cand[best_cand].parallax; 0 unless OK */
    vx_pnp_result pnp;       /* as vx_pnp_ransac on the pooled arrays; zeros when it did not run */
    vx_reloc_candidate_result cand[VX_MAX_RELOC_CANDIDATES];   /* entries n_cand and up are zero */
} vx_reloc_result;
/* n_cand in [1, VX_MAX_RELOC_CANDIDATES]; the candidates distinct live keyframes of `map`; every frame on
 * ctx's device: anything else is VX_ERR_INVALID and leaves the previous call's result in place.  k_reloc_pool
 * keeps one 64-bit key per current feature in LDS: a current frame whose capacity exceeds
 * vx_relocalize_table_limit (at least 4096 rows) is refused with VX_ERR_CAPACITY; there is no second path.
 * Ordering towards the map's context as in vx_track_pnp_async.  The call owns all of its buffers, so any
 * vx_track_*, vx_pnp_ransac or vx_match_* call may run on ctx between the enqueue and the fetch, and this
 * call between theirs.  May block at its start until the PREVIOUS call's argument table has left the pinned
 * staging it reuses. */
int vx_relocalize_async(vx_ctx* ctx, vx_dmap* map, int n_cand, const vx_reloc_candidate* cands, const vx_frame* curr,
                        float ratio, const double* intr4, const vx_track_options* opt);
/* One device-to-host copy of one packed block (record | pool_cand | pool_match | pool_train | mask) and one
 * synchronisation.  The four arrays hold n_pool entries each; any may be NULL.  VX_ERR_CAPACITY (with *out
 * filled) if an array is given and n_pool > cap_pool; VX_ERR_STATE when nothing was enqueued. */
int vx_relocalize_fetch(vx_ctx* ctx, vx_reloc_result* out, uint8_t* pool_cand, int32_t* pool_match, int32_t* pool_train,
                        uint8_t* mask, int cap_pool);
/* Candidate cand's device match list Match(kf_cand, curr), as vx_track_frame_matches: what
 * vx_dmap_create_keyframe_frame takes.  Valid until the next vx_relocalize_async on ctx. */
int vx_relocalize_matches(vx_ctx* ctx, int cand, const vx_match** d_matches, const int32_t** d_n, int32_t* cap);
/* The largest current-frame capacity vx_relocalize_async accepts on ctx's device: what is left of a
 * compute unit's 160 KiB of LDS beside k_reloc_pool's own use, in 8-byte keys. */
int vx_relocalize_table_limit(vx_ctx* ctx, int32_t* rows);

/* ---------------------------------------------------------------- recorded enqueue sequences
 * A list of the async calls above (event waits / records, vx_orb_extract_async,
 * vx_match_device_async, vx_ba_plan_run_async), recorded once with every argument and replayed by
 * vx_seq_run in the recorded order, exactly as the individual calls would run — for a pipelined
 * caller whose per-frame calls would otherwise each cross a language binding (bench.py: one step of
 * F frames = one vx_seq_run).  The recorded pointers (contexts, events, plans, device buffers) must
 * outlive the sequence.  vx_seq_run stops at the first failing call: its status is returned and
 * *failed_op (may be NULL) set to its index (-1 when every call succeeded). */
typedef struct vx_seq vx_seq;
int vx_seq_create(vx_seq** out);
void vx_seq_destroy(vx_seq* seq);
int vx_seq_wait(vx_seq* seq, vx_ctx* ctx, vx_event* ev);
int vx_seq_record(vx_seq* seq, vx_ctx* ctx, vx_event* ev);
int vx_seq_extract(vx_seq* seq, vx_ctx* ctx, const vx_orb_params* params, const uint8_t* d_img, int width,
                   int height, int channels, int64_t row_stride, int slot);
int vx_seq_match(vx_seq* seq, vx_ctx* ctx, const uint8_t* d_query, const int32_t* d_n_query, int cap_query,
                 const uint8_t* d_train, const int32_t* d_n_train, int cap_train, float ratio);
int vx_seq_ba_run(vx_seq* seq, vx_ctx* ctx, vx_ba_plan* plan);
int vx_seq_length(const vx_seq* seq);
int vx_seq_run(vx_seq* seq, int* failed_op);
/* threads > 1: vx_seq_run replays each context's calls on a host thread of its own (persistent
 * workers, one per context after the first), keeping on the host every cross-context order the
 * device semantics depend on (a wait after the record it follows in the sequence; a record after the
 * waits on the event's previous record).  1 (default): one thread, the recorded order. */
int vx_seq_set_threads(vx_seq* seq, int threads);

/* ---------------------------------------------------------------- multi-GPU (RCCL over xGMI) */
int vx_comm_unique_id(uint8_t* out_128);
int vx_comm_init(vx_ctx* ctx, const uint8_t* id_128, int nranks, int rank);
/* What RCCL itself reports for the context's communicator (ncclCommCount / ncclCommUserRank), so a
 * multi-GPU run can check it against WORLD_SIZE / RANK.  VX_ERR_STATE without a communicator. */
int vx_comm_info(vx_ctx* ctx, int* nranks, int* rank);

/* ---------------------------------------------------------------- profiling
 * When enabled, the library brackets its kernels with hipEvents on its own stream; read back
 * accumulated milliseconds and launch counts per stage (names via vx_prof_name).
 * stage_mask: 0 = off, -1 = every stage, otherwise bit s enables stage s only (so a timed run
 * can bracket just the kernel it reports without perturbing the others). */
int vx_prof_enable(vx_ctx* ctx, int stage_mask);
/* the same with a 64-bit mask (stages 32 and up; vx_prof_enable's int sign-extends, so its -1 is still all) */
int vx_prof_enable64(vx_ctx* ctx, uint64_t stage_mask);
int vx_prof_count(void);
const char* vx_prof_name(int stage);
int vx_prof_read(vx_ctx* ctx, double* ms, int64_t* launches, int reset);

#ifdef __cplusplus
}
#endif
#endif /* VX_SLAM_H */
