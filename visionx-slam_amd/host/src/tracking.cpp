// tracking.cpp — visionx::PnPTracker over vx_track_pnp_host_async / vx_track_pnp_fetch (see tracking.h).
#include "visionx/tracking.h"

#include <stdexcept>
#include <string>

#include "visionx/feature.h"

namespace visionx {

PnPTracker::PnPTracker(DeviceMap::Ptr map, const Options& options) : map_(std::move(map)), options_(options) {
    if (!map_) throw std::invalid_argument("PnPTracker: null DeviceMap");
}

bool PnPTracker::TrackWithPnP(const Frame::Ptr& last_keyframe, const Frame::Ptr& current) {
    if (!last_keyframe || !current) return false;  // tracking.cpp:333-336
    map_->Flush();
    // (the reference asks for the camera after the pair gate, :410-414; a frame without one cannot
    // pass either way, and the device call needs K up front)
    const auto cam = current->GetCamera();
    if (!cam) return false;
    const double intr[4] = {cam->fx(), cam->fy(), cam->cx(), cam->cy()};
    const auto& feats = current->Features();
    const int n_train = current->Descriptors().rows, n_query = last_keyframe->Descriptors().rows;
    if ((size_t)n_train != feats.size()) throw std::invalid_argument("TrackWithPnP: descriptors / features mismatch");
    xy_.resize(2 * feats.size());
    for (size_t i = 0; i < feats.size(); ++i) {  // cv::Point2f(px.x(), px.y()) (:398-399)
        xy_[2 * i] = (float)feats[i].position.x;
        xy_[2 * i + 1] = (float)feats[i].position.y;
    }
    vx_track_options o;
    vx_track_default_options(&o);
    o.min_matches = options_.min_matches;
    o.min_inliers = options_.min_inliers;
    o.pnp.reproj_error = options_.max_reproj_error;
    // the matches and the pairs are queued on the map's context: its stream orders them after the
    // map edits without a cross-context wait
    vx_ctx* c = map_->context();
    int rc = vx_track_pnp_host_async(c, map_->handle(), last_keyframe->Id(), last_keyframe->Descriptors().ptr(), n_query,
                                     current->Descriptors().ptr(), n_train, xy_.data(), options_.nn_ratio, intr, &o);
    if (rc != VX_OK) throw std::runtime_error(std::string("vx_track_pnp_host_async: ") + vx_last_error(c));
    rc = vx_track_pnp_fetch(c, &last_, nullptr, nullptr, 0);
    if (rc != VX_OK) throw std::runtime_error(std::string("vx_track_pnp_fetch: ") + vx_last_error(c));
    if (last_.status != VX_TRACK_OK) return false;
    const double* p = last_.pnp.pose;
    SE3d T;
    T.qx = p[0]; T.qy = p[1]; T.qz = p[2]; T.qw = p[3];
    T.tx = p[4]; T.ty = p[5]; T.tz = p[6];
    current->SetPose(T);
    last_parallax_ = last_.parallax;
    last_inliers_ = last_.pnp.n_inliers;
    return true;
}

}  // namespace visionx
