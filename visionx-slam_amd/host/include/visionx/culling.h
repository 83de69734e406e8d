// culling.h — Tracking::CullLandmarks, Tracking::CullKeyFrames and Tracking::RemoveKeyFrame
// (core/frontend/tracking.cpp:652-840) over the MI355X C ABI: the decision and the edit of the
// resident map run on the device (vx_dmap_cull_landmarks / vx_dmap_cull_keyframes, csrc/cull.hip),
// and the lists that come back are applied to the host objects the reference would have edited:
//
//   Landmark::SetBad, Feature::landmark_id_ / has_landmark / is_outlier      (:671, :741-743, :767-769)
//   Landmark::RemoveObservation                                              (:766)
//   Map::RemoveLandmark, Map::RemoveKeyFrame                                 (:746, :772)
//
// so the drop-in's host Map and the resident map stay equal.  What CreateKeyFrame calls before
// LocalBA (:76-84) with `enable_culling`.
#pragma once

#include <memory>
#include <vector>

#include "vx_slam.h"
#include "visionx/device_map.h"
#include "visionx/frame.h"

namespace visionx {

class MapCulling {
public:
    struct Options {  // Tracking::Options, "Map culling" (tracking.h:33-40)
        int min_landmark_observations = 2;
        int min_landmarks_for_culling = 200;
        int min_keyframes_for_culling = 3;
        int max_keyframes = 30;
        int kf_min_shared_observations = 3;
        double kf_redundant_ratio = 0.9;
        double landmark_max_reproj_error = 5.0;
    };
    MapCulling(DeviceMap::Ptr device_map, Map::Ptr map) : MapCulling(std::move(device_map), std::move(map), Options()) {}
    MapCulling(DeviceMap::Ptr device_map, Map::Ptr map, const Options& options);

    // Tracking::CullLandmarks; returns how many landmarks left the map
    int CullLandmarks();
    // Tracking::CullKeyFrames with Tracking's three protected frames as arguments (any may be null);
    // returns the removed keyframe, or null
    Frame::Ptr CullKeyFrames(const Frame::Ptr& last_keyframe, const Frame::Ptr& init_frame,
                             const Frame::Ptr& current_frame);
    // Tracking::RemoveKeyFrame of an arbitrary keyframe, through the resident map's edit calls
    void RemoveKeyFrame(const Frame::Ptr& keyframe);

    double LastRatio() const { return last_ratio_; }                           // removed_ratio (:829)
    const std::vector<vx_cull_landmark>& LastLandmarks() const { return lm_; }  // the last call's lists
    const std::vector<vx_cull_feature>& LastFeatures() const { return feat_; }

private:
    vx_cull_options Native() const;
    void Fetch();
    void ApplyLandmarks(size_t n_features);
    DeviceMap::Ptr dmap_;
    Map::Ptr map_;
    Options options_;
    double last_ratio_ = 0.0;
    std::vector<vx_cull_landmark> lm_;
    std::vector<vx_cull_feature> feat_;
};

}  // namespace visionx
