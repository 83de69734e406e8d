// culling.cpp — visionx::MapCulling over vx_dmap_cull_* (see culling.h).
#include "visionx/culling.h"

#include <stdexcept>
#include <string>

namespace visionx {

namespace {
void Check(vx_ctx* ctx, int rc, const char* what) {
    if (rc != VX_OK && rc != VX_ERR_CAPACITY) throw std::runtime_error(std::string(what) + ": " + vx_last_error(ctx));
}
void Reset(Feature& f) {  // (:741-743, :767-769)
    f.landmark_id_ = 0;
    f.has_landmark = false;
    f.is_outlier = true;
}
}  // namespace

MapCulling::MapCulling(DeviceMap::Ptr device_map, Map::Ptr map, const Options& options)
    : dmap_(std::move(device_map)), map_(std::move(map)), options_(options) {}

vx_cull_options MapCulling::Native() const {
    vx_cull_options o;
    vx_cull_default_options(&o);
    o.min_landmark_observations = options_.min_landmark_observations;
    o.min_landmarks_for_culling = options_.min_landmarks_for_culling;
    o.min_keyframes_for_culling = options_.min_keyframes_for_culling;
    o.max_keyframes = options_.max_keyframes;
    o.kf_min_shared_observations = options_.kf_min_shared_observations;
    o.kf_redundant_ratio = options_.kf_redundant_ratio;
    o.landmark_max_reproj_error = options_.landmark_max_reproj_error;
    return o;
}

void MapCulling::Fetch() {
    int nl = 0, nf = 0;
    Check(dmap_->context(), vx_dmap_cull_results(dmap_->handle(), 0, nullptr, 0, nullptr, &nl, &nf), "vx_dmap_cull_results");
    lm_.resize((size_t)nl);
    feat_.resize((size_t)nf);
    Check(dmap_->context(), vx_dmap_cull_results(dmap_->handle(), nl, lm_.data(), nf, feat_.data(), &nl, &nf),
          "vx_dmap_cull_results");
}

// the culled landmarks' records onto the host objects: SetBad, the feature resets (the first
// n_features records), Map::RemoveLandmark
void MapCulling::ApplyLandmarks(size_t n_features) {
    for (const vx_cull_landmark& r : lm_) {
        const Landmark::Ptr& lm = dmap_->LandmarkAt(r.row);
        if (lm) lm->SetBad();
    }
    for (size_t i = 0; i < n_features; ++i) {
        const Frame::Ptr& kf = dmap_->FrameAt(feat_[i].kf_row);
        if (kf && (size_t)feat_[i].feat_idx < kf->Features().size()) Reset(kf->Features()[(size_t)feat_[i].feat_idx]);
    }
    for (const vx_cull_landmark& r : lm_) {
        if (map_) map_->RemoveLandmark(r.lm_id);
        dmap_->DroppedLandmark(r.row, r.lm_id);
    }
}

int MapCulling::CullLandmarks() {
    dmap_->Flush();
    const vx_cull_options o = Native();
    int nl = 0, nf = 0;
    Check(dmap_->context(), vx_dmap_cull_landmarks(dmap_->context(), dmap_->handle(), &o, &nl, &nf),
          "vx_dmap_cull_landmarks");
    Fetch();
    ApplyLandmarks(feat_.size());
    return nl;
}

Frame::Ptr MapCulling::CullKeyFrames(const Frame::Ptr& last_keyframe, const Frame::Ptr& init_frame,
                                     const Frame::Ptr& current_frame) {
    dmap_->Flush();
    const vx_cull_options o = Native();
    std::vector<uint64_t> protect;
    for (const Frame::Ptr* f : {&last_keyframe, &init_frame, &current_frame})
        if (*f) protect.push_back((*f)->Id());
    int removed = 0, nl = 0, nf = 0;
    uint64_t kid = 0;
    last_ratio_ = 0.0;
    Check(dmap_->context(),
          vx_dmap_cull_keyframes(dmap_->context(), dmap_->handle(), &o, protect.data(), (int)protect.size(), &removed, &kid,
                                 &last_ratio_, &nl, &nf),
          "vx_dmap_cull_keyframes");
    Fetch();
    if (!removed) return nullptr;
    // Tracking::RemoveKeyFrame first: the removed keyframe's own records close the feature list
    size_t own = feat_.size();
    while (own > 0 && feat_[own - 1].kf_id == kid) --own;  // (a culled landmark's records never name it: it left the map)
    Frame::Ptr kf = own < feat_.size() ? dmap_->FrameAt(feat_[own].kf_row) : (map_ ? map_->GetFrame(kid) : nullptr);
    if (kf) {
        for (size_t i = own; i < feat_.size(); ++i) {
            Feature& f = kf->Features()[(size_t)feat_[i].feat_idx];
            if (map_)
                if (auto lm = map_->GetLandmark(f.landmark_id_)) lm->RemoveObservation(kid);   // (:766)
            Reset(f);
        }
    }
    if (map_) map_->RemoveKeyFrame(kid);                                                     // (:772)
    dmap_->DroppedKeyFrame(kid);
    ApplyLandmarks(own);                                                                     // (:838)
    return kf;
}

void MapCulling::RemoveKeyFrame(const Frame::Ptr& keyframe) {
    if (!keyframe) return;
    const uint64_t kid = keyframe->Id();
    std::vector<int> idx;
    auto& feats = keyframe->Features();
    for (size_t i = 0; i < feats.size(); ++i) {
        Feature& f = feats[i];
        if (!f.has_landmark) continue;
        auto lm = map_ ? map_->GetLandmark(f.landmark_id_) : nullptr;
        if (!lm) continue;
        lm->RemoveObservation(kid);
        dmap_->RemoveObservation(lm->Id(), kid);
        Reset(f);
        idx.push_back((int)i);
    }
    if (!idx.empty()) dmap_->UpdateFeatures(keyframe, idx);
    if (map_) map_->RemoveKeyFrame(kid);
    dmap_->RemoveKeyFrame(kid);
}

}  // namespace visionx
