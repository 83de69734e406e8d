// tracking.h — Tracking::TrackWithPnP (core/frontend/tracking.cpp:332-455) over the MI355X C ABI as
// one device-resident sequence (vx_track_pnp_host_async + vx_track_pnp_fetch, csrc/track.hip):
//
//   matcher_->Match(last_keyframe_, current_frame_, matches)        (:340)
//   distance filter, min_matches gate                               (:342-361)
//   3D-2D pairs over map_->GetLandmark                              (:364-407)
//   cv::solvePnPRansac, min_inliers gate                            (:414-429)
//   cv::Rodrigues, rotation check, current_frame_->SetPose          (:432-447)
//   last_parallax_ = ComputeParallax(...), last_inliers_            (:449-450)
//
// with one upload (both descriptor sets + the current positions) and one synchronisation.
// The landmarks and the last keyframe's features are read from the resident map (DeviceMap), which
// the integration keeps current at the points Tracking edits the reference's Map (device_map.h).
#pragma once

#include <memory>
#include <vector>

#include "vx_slam.h"
#include "visionx/device_map.h"
#include "visionx/frame.h"

namespace visionx {

class PnPTracker {
public:
    struct Options {                     // Tracking::Options (tracking.h:27-29), ORBMatcher::Options
        int min_matches = 50;
        int min_inliers = 30;
        float max_reproj_error = 2.0f;
        float nn_ratio = 0.8f;           // orb_matcher.h:12
    };
    explicit PnPTracker(DeviceMap::Ptr map) : PnPTracker(std::move(map), Options()) {}
    PnPTracker(DeviceMap::Ptr map, const Options& options);

    // Tracking::TrackWithPnP with last_keyframe_ / current_frame_ as arguments: the reference's
    // return values (false for a null keyframe or camera, too few matches / pairs / inliers, a
    // non-finite rotation); on success current->SetPose(T_cw).  last_keyframe must be a keyframe of
    // the DeviceMap (std::runtime_error otherwise, with the library's message).
    bool TrackWithPnP(const Frame::Ptr& last_keyframe, const Frame::Ptr& current);

    int LastInliers() const { return last_inliers_; }        // last_inliers_  (:450; kept on failure)
    double LastParallax() const { return last_parallax_; }   // last_parallax_ (:449; kept on failure)
    const vx_track_result& LastResult() const { return last_; }  // every count of the last call

private:
    friend class FrameTracker;  // TrackResident sets last_ / last_inliers_ / last_parallax_ as TrackWithPnP does
    DeviceMap::Ptr map_;
    Options options_;
    vx_track_result last_{};
    int last_inliers_ = 0;
    double last_parallax_ = 0.0;
    std::vector<float> xy_;
};

// Tracking::TrackLastFrame (core/frontend/tracking.cpp:281-330) and the head of
// Tracking::InitWithSecondFrame (:207-245) as one device-resident sequence
// (vx_track_essential_host_async + vx_track_essential_fetch, csrc/track_ess.hip):
//
//   matcher_->Match(last_frame_, current_frame_, matches)           (:289)
//   distance filter, min_matches gate                               (:291-310)
//   cv::Point2f pairs, findEssentialMat + recoverPose               (:509-528)
//   min_inliers gate                                                (:317, :530)
//   curr->SetPose(Sophus::SE3d(R, t) * last->Pose())                (:539-541)
//   last_inliers_, last_parallax_ = ComputeParallax(...)            (:324-325)
//
// with one upload (both descriptor sets + both position sets) and one synchronisation.  No map is read.
class EssentialTracker {
public:
    struct Options {                     // Tracking::Options (tracking.h:27-28), ORBMatcher::Options
        int min_matches = 50;
        int min_inliers = 30;
        float nn_ratio = 0.8f;           // orb_matcher.h:12
    };
    // ctx: the context the calls are queued on (not owned); nullptr = the calling thread's own
    explicit EssentialTracker(vx_ctx* ctx = nullptr) : EssentialTracker(ctx, Options()) {}
    EssentialTracker(vx_ctx* ctx, const Options& options) : ctx_(ctx), options_(options) {}

    // Tracking::TrackLastFrame with last_frame_ / current_frame_ as arguments: the reference's return
    // values (false for a null frame or camera, too few matches, a failed essential estimate, too few
    // inliers); on success current->SetPose(T_cl * last->Pose()).  Feature positions are narrowed to
    // float as cv::Point2f does; std::invalid_argument if a coordinate is not float-representable
    // (the parallax, which the reference takes from the doubles, would differ).
    bool TrackLastFrame(const Frame::Ptr& last, const Frame::Ptr& current);
    // Tracking::InitWithSecondFrame up to its parallax gate (:207-245) with init_frame_ /
    // current_frame_ as arguments: the same sequence with T_lw = identity (init's pose is not read),
    // then `parallax < 1.0f * M_PI / 180.0f` -> false.  On success current->SetPose(T_cl) and
    // LastInliers / LastParallax are set (:259-260); landmark creation and the two insertions stay
    // with KeyFrameLandmarks::CreateKeyFrame.
    bool EstimateInitialPose(const Frame::Ptr& init, const Frame::Ptr& current);

    int LastInliers() const { return last_inliers_; }        // last_inliers_  (:324; kept on failure)
    double LastParallax() const { return last_parallax_; }   // last_parallax_ (:325; kept on failure)
    const vx_track_essential_result& LastResult() const { return last_; }  // every count of the last call

private:
    friend class FrameTracker;  // TrackResident sets last_ / last_inliers_ / last_parallax_ as TrackLastFrame does
    bool Run(const Frame::Ptr& last, const Frame::Ptr& current, const double* pose_last7);
    vx_ctx* ctx_;
    Options options_;
    vx_track_essential_result last_{};
    int last_inliers_ = 0;
    double last_parallax_ = 0.0;
    std::vector<float> xy_last_, xy_curr_;
};

// Tracking::Track() (core/frontend/tracking.cpp:267-279): TrackWithPnP against the last keyframe when
// there is one, and TrackLastFrame when that fails.  Sequential, as the reference: the fallback is
// enqueued only once the PnP result is known.
class FrameTracker {
public:
    struct Options {
        PnPTracker::Options pnp;
        EssentialTracker::Options essential;
    };
    explicit FrameTracker(DeviceMap::Ptr map) : FrameTracker(std::move(map), Options()) {}
    FrameTracker(DeviceMap::Ptr map, const Options& options);

    // last_keyframe may be null (no PnP attempt, :269); last_frame null -> false (:282-285)
    bool Track(const Frame::Ptr& last_keyframe, const Frame::Ptr& last_frame, const Frame::Ptr& current);

    // Track() over resident frames (frame.h: Frame::Resident(), filled by ORBExtractor::ExtractResident or
    // UploadResident): ONE vx_track_frame_async and one fetch whichever path sets the pose, the PnP ->
    // TrackLastFrame decision taken on the device (csrc/track_frame.hip).  Returns what Track returns
    // and sets the pose, UsedFallback(), LastInliers() and LastParallax() as Track sets them; the fetch
    // also fills current->Features() (position, response) from the keypoint rows it brings down.
    // Descriptors() stays empty (Materialize fetches them on demand).  Every frame given must have a
    // resident handle (std::invalid_argument otherwise).
    bool TrackResident(const Frame::Ptr& last_keyframe, const Frame::Ptr& last_frame, const Frame::Ptr& current);
    // EssentialTracker::EstimateInitialPose (tracking.cpp:207-245) over resident frames: the same call
    // with no last keyframe and T_lw = identity, then the parallax gate; sets Essential()'s LastInliers /
    // LastParallax as EstimateInitialPose does and fills current->Features().
    bool EstimateInitialPoseResident(const Frame::Ptr& init, const Frame::Ptr& current);
    // Track() for every camera of a rig time step over the one resident map: ONE vx_track_rig_async and one
    // fetch (csrc/track_rig.hip), each camera taking its own path on the device.  Per camera it returns
    // what TrackResident returns, sets the pose and fills current->Features() as TrackResident does, and
    // keeps UsedFallback / LastInliers / LastParallax per camera index (RigUsedFallback, ...; the last two
    // kept on failure, as the single trackers keep theirs).  At most VX_MAX_RIG_CAMERAS cameras
    // (std::invalid_argument beyond); a camera TrackResident would refuse without a device call (no
    // current frame, no camera model, neither a last keyframe nor a last frame) returns false and stays
    // out of the call.  The component trackers' own LastInliers / UsedFallback are not touched.
    struct RigCamera {
        Frame::Ptr last_keyframe, last_frame, current;
    };
    std::vector<bool> TrackRig(const std::vector<RigCamera>& cams);
    bool RigUsedFallback(size_t cam) const { return rig_.at(cam).used_fallback; }
    int RigLastInliers(size_t cam) const { const RigState& r = rig_.at(cam); return r.used_fallback ? r.ess_inliers : r.pnp_inliers; }
    double RigLastParallax(size_t cam) const { const RigState& r = rig_.at(cam); return r.used_fallback ? r.ess_parallax : r.pnp_parallax; }
    const vx_track_frame_result& RigResult(size_t cam) const { return rig_.at(cam).result; }
    // Relocalisation (csrc/reloc.hip; what tracking.cpp:477-499 leaves as a TODO): TrackWithPnP of `current`
    // against the landmarks of all `keyframes` at once, as ONE vx_relocalize_async and one fetch.  keyframes: 1 ..
    // VX_MAX_RELOC_CANDIDATES distinct keyframes of the resident map, each with a resident handle, in the order
    // they are to be tried (std::invalid_argument otherwise; an empty list, a null current frame or one without a
    // camera returns false without a device call).  On success it sets the pose, UsedFallback() = false,
    // LastInliers() (the pooled PnP's inliers) and LastParallax() (the best keyframe's, as TrackWithPnP computes
    // it) and RelocBestKeyFrame(): the candidate most pooled inliers came from, whose device match list
    // MatchList then finds, so that KeyFrameLandmarks::CreateKeyFrame(RelocBestKeyFrame(), current) reuses it.
    // Either way it fills current->Features() as TrackResident does (one more fetch, of the frame's rows).
    bool Relocalize(const std::vector<Frame::Ptr>& keyframes, const Frame::Ptr& current);
    const Frame::Ptr& RelocBestKeyFrame() const { return reloc_best_; }        // null after a failed Relocalize
    const vx_reloc_result& LastRelocResult() const { return reloc_; }
    // The device match list the last resident call (TrackResident, EstimateInitialPoseResident, TrackRig or
    // Relocalize: each keeps its own) holds for Match(query, train), by frame ids
    // (tracking.cpp:340 and :863, and :208 and :863, match the same two frames): false when it holds none.
    bool MatchList(uint64_t query_id, uint64_t train_id, const vx_match** d_matches, const int32_t** d_n, int32_t* cap) const;
    // Resident calls use ONE ratio for both matches (the matcher's nn_ratio, set by Tracking::UseResidentFrames);
    // TrackResident throws when the two component trackers' ratios differ.
    void SetRatio(float nn_ratio);
    float Ratio() const;
    const DeviceMap::Ptr& ResidentMap() const;
    const vx_track_frame_result& LastResidentResult() const { return resident_; }

    bool UsedFallback() const { return used_fallback_; }     // the last Track() ran TrackLastFrame
    int LastInliers() const { return used_fallback_ ? essential_.LastInliers() : pnp_.LastInliers(); }
    double LastParallax() const { return used_fallback_ ? essential_.LastParallax() : pnp_.LastParallax(); }
    PnPTracker& Pnp() { return pnp_; }
    EssentialTracker& Essential() { return essential_; }

private:
    PnPTracker pnp_;
    EssentialTracker essential_;
    bool used_fallback_ = false;
    void RunResident(const Frame::Ptr& last_keyframe, const Frame::Ptr& last_frame, const Frame::Ptr& current,
                     bool identity_last);
    vx_track_frame_result resident_{};
    std::vector<vx_keypoint> kp_;
    // (query frame id, train frame id) of the two device match lists of the last resident call
    uint64_t list_ids_[2][2] = {{0, 0}, {0, 0}};
    bool list_valid_[2] = {false, false};
    // per rig camera: its state across calls and the ids of its two device lists of the last TrackRig
    struct RigState {
        bool used_fallback = false;
        int pnp_inliers = 0, ess_inliers = 0;
        double pnp_parallax = 0.0, ess_parallax = 0.0;
        vx_track_frame_result result{};
        int slot = -1;  // the camera's index in the last vx_track_rig_async (-1: it stayed out)
        uint64_t list_ids[2][2] = {{0, 0}, {0, 0}};
        bool list_valid[2] = {false, false};
    };
    std::vector<RigState> rig_;
    // the last Relocalize: its record, its best keyframe and the (query, train) ids of that candidate's device list
    vx_reloc_result reloc_{};
    Frame::Ptr reloc_best_;
    uint64_t reloc_ids_[2] = {0, 0};
    int reloc_slot_ = -1;  // the best candidate's index in the last vx_relocalize_async (-1: no list)
};

}  // namespace visionx
