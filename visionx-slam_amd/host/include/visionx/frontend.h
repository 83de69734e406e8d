// frontend.h — visionx::Tracking (core/frontend/tracking.h:17-123, tracking.cpp:19-89, :177-204,
// :459-499, :562-575) over the MI355X C ABI: the reference's State, Options, constructor,
// ProcessFrame and GetState, with every body it calls replaced by the device-resident adapter of this
// directory, composed in the reference's order:
//
//   extractor_->Extract(*current_frame_)                                   (:42)
//   InitWithFirstFrame   the three gates: vx_init_gate_host_async + fetch  (:177-204)
//   InitWithSecondFrame  EssentialTracker::EstimateInitialPose, then two
//                        KeyFrameLandmarks::CreateKeyFrame calls           (:206-263; ids: init depth,
//                                                                           current depth, triangulated)
//   Track                FrameTracker::Track (PnP, then TrackLastFrame)    (:267-279)
//   CreateKeyFrame       KeyFrameLandmarks::CreateKeyFrame                 (:577-584)
//   CullLandmarks / CullKeyFrames   MapCulling                             (:78-81)
//   local_ba_->Optimize  LocalBA over the DeviceMap                        (:82-84)
//   HandleTrackingBad / Lost   Map::removeAll + DeviceMap::removeAll       (:477-499); with UseRelocalisation,
//                              FrameTracker::Relocalize against the map's latest keyframes first
//
// It owns the DeviceMap that mirrors `map`; the map handed to the constructor must be empty (or be
// mirrored by hand through ResidentMap()).  VisualizeFeatures is not ported.
#pragma once

#include <memory>
#include <vector>

#include "vx_slam.h"
#include "visionx/culling.h"
#include "visionx/device_map.h"
#include "visionx/feature.h"
#include "visionx/mapping.h"
#include "visionx/tracking.h"

namespace visionx {

class Tracking {
public:
    using Ptr = std::shared_ptr<Tracking>;
    using KeyFrame = Frame;

    enum class State { INIT = 0, TRACKING_GOOD, TRACKING_BAD, LOST };

    struct Options {  // tracking.h:24-54
        int min_matches = 50;
        int min_inliers = 30;
        int min_keyframe_inliers = 50;
        double min_parallax = 10.0;
        double max_reproj_error = 2.0;
        int min_keyframe_gap = 3;
        bool enable_culling = false;

        // ===== Map culling =====
        int min_landmark_observations = 2;
        int min_landmarks_for_culling = 200;
        int min_keyframes_for_culling = 3;
        int max_keyframes = 30;
        int kf_min_shared_observations = 3;
        double kf_redundant_ratio = 0.9;
        double landmark_max_reproj_error = 5.0;

        // ===== Triangulation =====
        double triangulation_max_reproj_error = 5.0;
        double triangulation_min_angle_deg = 1.0;

        // ===== Local BA =====
        bool enable_local_ba = true;
        int ba_window_size = 5;
        int ba_iterations = 5;
        int ba_min_pose_observations = 20;
        int ba_min_point_observations = 2;
        double ba_huber_delta = 5.0;
        double ba_max_reproj_error = 5.0;
    };

    Tracking(const Options& options, std::shared_ptr<FeatureExtractor> extractor,
             std::shared_ptr<FeatureMatcher> matcher, std::shared_ptr<Map> map);

    void ProcessFrame(Frame::Ptr frame);

    // Resident frames (opt-in, before the first frame): every frame's keypoints and
    // descriptors stay on the device for as long as the Frame lives, and ProcessFrame calls no
    // FeatureMatcher::Match at all:
    //   extraction   ORBExtractor::ExtractResident (no synchronisation); any other extractor must leave a
    //                resident handle on the frame itself (UploadResident) in its Extract
    //   InitWithFirstFrame   one vx_frame_fetch of the keypoints, then the host-input gate (the image is
    //                on the host anyway)
    //   InitWithSecondFrame  FrameTracker::EstimateInitialPoseResident; the two CreateKeyFrame calls reuse
    //                its match list
    //   Track        FrameTracker::TrackResident: one enqueue, one synchronisation whichever path it takes
    //   CreateKeyFrame  the track's own match list (KeyFrameLandmarks::UseTrackLists)
    // Throws std::logic_error after the first frame, and std::invalid_argument unless the matcher is an
    // ORBMatcher, whose nn_ratio is then the one ratio used everywhere.  Features() are filled as in the
    // default mode; Descriptors() stay empty (Materialize fetches them on demand).
    void UseResidentFrames(bool on);
    bool ResidentFrames() const { return resident_; }

    // Relocalisation (opt-in, before the first frame; requires UseResidentFrames(true)).  The
    // reference's HandleTrackingBad and HandleTrackingLost (tracking.cpp:477-499) carry a TODO, "for now just
    // re-initialise", and throw the whole map away.  With max_candidates > 0 both first relocalise
    // current_frame_ (FrameTracker::Relocalize: one enqueue, one fetch) against RelocCandidates(*map_,
    // max_candidates).  On success last_keyframe_ becomes the best keyframe, last_inliers_ / last_parallax_ are the
    // record's, and the frame goes on through :76-88 exactly as after a successful Track(); on failure the
    // reference's reset runs.  0 (default): off.  Throws std::logic_error after the first frame or without resident
    // frames, std::invalid_argument outside [0, VX_MAX_RELOC_CANDIDATES].
    void UseRelocalisation(int max_candidates);
    int Relocalisation() const { return reloc_candidates_; }
    // the candidates: the max_candidates keyframes of `map` with the highest ids whose frames hold a resident
    // handle, most recent first
    static std::vector<Frame::Ptr> RelocCandidates(const Map& map, int max_candidates);
    bool LastFrameRelocalised() const { return relocalised_; }               // the last ProcessFrame relocalised its frame

    State GetState() const { return state_; }

    // read-only views of the private members (tracking.h:105-122) and of the last calls
    int LastInliers() const { return last_inliers_; }
    double LastParallax() const { return last_parallax_; }
    const vx_init_gate_result& LastInitGate() const { return last_gate_; }  // the last InitWithFirstFrame's record
    const Frame::Ptr& LastKeyFrame() const { return last_keyframe_; }
    const Frame::Ptr& LastFrame() const { return last_frame_; }
    uint64_t Landmarks() const { return keyframes_.landmark_id_; }          // landmark_id_: the next landmark id
    const DeviceMap::Ptr& ResidentMap() const { return dmap_; }
    const LocalBA* LocalBa() const { return local_ba_.get(); }              // null without enable_local_ba
    const FrameTracker& Tracker() const { return tracker_; }               // UsedFallback(): the last Track() ran TrackLastFrame

private:
    bool InitWithFirstFrame();
    bool InitWithSecondFrame();
    bool Track();
    void UpdateTrackingState();
    void HandleTrackingFailure();
    bool HandleTrackingBad();   // true: current_frame_ was relocalised and goes on as a tracked frame
    bool HandleTrackingLost();
    bool Relocalise();
    void Reset();
    bool NeedNewKeyFrame() const;
    void CreateKeyFrame();

    State state_ = State::INIT;
    Options options_;

    Frame::Ptr init_frame_;
    Frame::Ptr current_frame_;
    Frame::Ptr last_frame_;
    Frame::Ptr last_keyframe_;

    int last_inliers_ = 0;
    double last_parallax_ = 0.0;

    std::shared_ptr<FeatureExtractor> extractor_;
    std::shared_ptr<FeatureMatcher> matcher_;
    std::shared_ptr<Map> map_;

    DeviceMap::Ptr dmap_;
    FrameTracker tracker_;
    KeyFrameLandmarks keyframes_;  // holds landmark_id_
    MapCulling culling_;
    std::unique_ptr<LocalBA> local_ba_;
    vx_init_gate_result last_gate_{};
    std::vector<float> xy_;
    bool resident_ = false;
    int reloc_candidates_ = 0;
    bool relocalised_ = false;
};

}  // namespace visionx
