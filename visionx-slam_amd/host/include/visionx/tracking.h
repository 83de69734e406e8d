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
    DeviceMap::Ptr map_;
    Options options_;
    vx_track_result last_{};
    int last_inliers_ = 0;
    double last_parallax_ = 0.0;
    std::vector<float> xy_;
};

}  // namespace visionx
