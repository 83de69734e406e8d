// mapping.h — the landmark-creation half of Tracking::CreateKeyFrame (core/frontend/tracking.cpp:
// 577-580), run on every new keyframe right before LocalBA, over the MI355X C ABI:
//
//   CreateLandmarksFromDepth     tracking.cpp:586-650   -> vx_depth_landmarks
//   TriangulateWithLastKeyFrame  tracking.cpp:856-929   -> Match() + vx_triangulate
//   (TriangulatePoint / ProjectionMatrix, tracking.cpp:843-854, 931-945, run inside the kernel)
//
// With a DeviceMap (UseDeviceMap) the whole block of tracking.cpp:577-581 — both functions and
// Map::InsertKeyFrame — is one call on the resident map:
//
//   CreateKeyFrame(last, curr)   tracking.cpp:577-581   -> Match() + vx_dmap_create_keyframe_host
//
// Same member names, option names / defaults (Tracking::Options, tracking.h:43-44) and side effects
// as the reference: landmarks get consecutive ids from landmark_id_, observations are added and
// the features' landmark_id_ / has_landmark / is_outlier are set in the reference's order.
#pragma once

#include <memory>
#include <utility>
#include <vector>

#include "visionx/feature.h"

namespace visionx {

class FrameTracker;  // tracking.h

class KeyFrameLandmarks {
public:
    struct Options {
        double triangulation_max_reproj_error = 5.0;  // tracking.h:43
        double triangulation_min_angle_deg = 1.0;     // tracking.h:44
    };
    KeyFrameLandmarks(Map::Ptr map, FeatureMatcher::Ptr matcher, const Options& options)
        : map_(std::move(map)), matcher_(std::move(matcher)), options_(options) {}

    void CreateLandmarksFromDepth(const Frame::Ptr& frame);
    void TriangulateWithLastKeyFrame(Frame::Ptr last_frame, Frame::Ptr curr_frame);

    // The resident map CreateKeyFrame works on (device_map.h); it must already mirror map_.
    void UseDeviceMap(std::shared_ptr<DeviceMap> dm) { dmap_ = std::move(dm); }
    // CreateLandmarksFromDepth(curr) + TriangulateWithLastKeyFrame(last, curr) + Map::InsertKeyFrame(curr)
    // (+ DeviceMap::InsertKeyFrame) as one vx_dmap_create_keyframe_host call: the decision and the
    // resident map's edit run on the device — the last keyframe's pose is the resident one, which
    // after a LocalBA may be ahead of last_frame->Pose() — and the reference's loop bodies then run
    // over the returned records on the host objects; nothing is forwarded to the device a second
    // time.  curr arrives without links (tracking.cpp:577); last_frame may be null (the first frame
    // of InitWithSecondFrame: no triangulation).  Returns the next landmark_id_.
    uint64_t CreateKeyFrame(Frame::Ptr last_frame, Frame::Ptr curr_frame);
    // Resident mode: with a tracker attached, CreateKeyFrame on frames that hold resident handles
    // (frame.h) is vx_dmap_create_keyframe_frame on the current frame's device positions and the
    // match list the tracker's last resident call holds for these two frames (checked by frame id);
    // only when it holds none are the two frames matched, on the device.  matcher_->Match is not
    // called; the depth image is uploaded, one copy per keyframe; the records and the host mirrors
    // are handled exactly as in the host-input form.  nullptr (default): the host-input form.
    void UseTrackLists(const FrameTracker* tracker) { tracks_ = tracker; }
    // CreateKeyFrame for every (last, curr) pair of a rig time step, in order.  With a tracker attached
    // (UseTrackLists), 1 .. VX_MAX_RIG_CAMERAS pairs, resident frames and the tracker's list for every
    // pair that has a last frame — the state right after FrameTracker::TrackRig — it is ONE
    // vx_dmap_create_keyframes_rig call (one upload, one synchronisation) followed by the reference's
    // loop bodies, Map::InsertKeyFrame and DeviceMap::Created per camera over that camera's slice of the
    // records.  In any other case it runs CreateKeyFrame pair by pair, which gives the same map, links
    // and ids.  The cameras' last frames must be distinct keyframes of the map (the rig call refuses a
    // shared one).  LastRecords() then holds all cameras' records.  Returns the next landmark_id_.
    uint64_t CreateKeyFrameRig(const std::vector<std::pair<Frame::Ptr, Frame::Ptr>>& last_curr);
    const std::vector<vx_keyframe_landmark>& LastRecords() const { return rec_; }

    uint64_t landmark_id_ = 0;  // Tracking::landmark_id_ (tracking.h): next landmark id

private:
    void ApplyRecords(const Frame::Ptr& last_frame, const Frame::Ptr& curr_frame, const vx_keyframe_landmark* rec,
                      size_t n);
    Map::Ptr map_;
    FeatureMatcher::Ptr matcher_;
    Options options_;
    std::vector<double> uv_, uv2_, pw_;
    std::vector<uint8_t> has_, has2_;
    std::vector<int32_t> idx_;
    std::vector<vx_match> m_;
    std::shared_ptr<DeviceMap> dmap_;
    std::vector<vx_keyframe_landmark> rec_;
    const FrameTracker* tracks_ = nullptr;
};

}  // namespace visionx
