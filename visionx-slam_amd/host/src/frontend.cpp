// frontend.cpp — visionx::Tracking: the reference's state machine over the device-resident adapters
// (see frontend.h).
#include "visionx/frontend.h"

#include <stdexcept>
#include <string>

namespace visionx {

namespace {

FrameTracker::Options TrackerOptions(const Tracking::Options& o) {
    FrameTracker::Options t;
    t.pnp.min_matches = o.min_matches;
    t.pnp.min_inliers = o.min_inliers;
    t.pnp.max_reproj_error = (float)o.max_reproj_error;
    t.essential.min_matches = o.min_matches;
    t.essential.min_inliers = o.min_inliers;
    return t;
}

MapCulling::Options CullingOptions(const Tracking::Options& o) {
    MapCulling::Options c;
    c.min_landmark_observations = o.min_landmark_observations;
    c.min_landmarks_for_culling = o.min_landmarks_for_culling;
    c.min_keyframes_for_culling = o.min_keyframes_for_culling;
    c.max_keyframes = o.max_keyframes;
    c.kf_min_shared_observations = o.kf_min_shared_observations;
    c.kf_redundant_ratio = o.kf_redundant_ratio;
    c.landmark_max_reproj_error = o.landmark_max_reproj_error;
    return c;
}

}  // namespace

// ================= construction (tracking.cpp:19-35) =================

Tracking::Tracking(const Options& options, std::shared_ptr<FeatureExtractor> extractor,
                   std::shared_ptr<FeatureMatcher> matcher, std::shared_ptr<Map> map)
    : options_(options),
      extractor_(std::move(extractor)),
      matcher_(std::move(matcher)),
      map_(std::move(map)),
      dmap_(std::make_shared<DeviceMap>()),
      tracker_(dmap_, TrackerOptions(options)),
      keyframes_(map_, matcher_, {options.triangulation_max_reproj_error, options.triangulation_min_angle_deg}),
      culling_(dmap_, map_, CullingOptions(options)) {
    keyframes_.UseDeviceMap(dmap_);
    if (options_.enable_local_ba) {
        LocalBA::Options ba_options;
        ba_options.window_size = options_.ba_window_size;
        ba_options.max_iterations = options_.ba_iterations;
        ba_options.min_pose_observations = options_.ba_min_pose_observations;
        ba_options.min_point_observations = options_.ba_min_point_observations;
        ba_options.huber_delta = options_.ba_huber_delta;
        ba_options.max_reproj_error = options_.ba_max_reproj_error;
        local_ba_ = std::make_unique<LocalBA>(ba_options);
        local_ba_->UseDeviceMap(dmap_);
    }
}

void Tracking::UseResidentFrames(bool on) {
    if (current_frame_) throw std::logic_error("Tracking::UseResidentFrames: only before the first frame");
    if (on) {
        const auto* orb = dynamic_cast<const ORBMatcher*>(matcher_.get());
        if (!orb) throw std::invalid_argument("Tracking::UseResidentFrames: the matcher is not an ORBMatcher");
        tracker_.SetRatio(orb->options().nn_ratio);
        if (auto* ex = dynamic_cast<ORBExtractor*>(extractor_.get())) ex->UseContext(dmap_->context());
    }
    keyframes_.UseTrackLists(on ? &tracker_ : nullptr);
    resident_ = on;
}

void Tracking::UseRelocalisation(int max_candidates) {
    if (current_frame_) throw std::logic_error("Tracking::UseRelocalisation: only before the first frame");
    if (max_candidates < 0 || max_candidates > VX_MAX_RELOC_CANDIDATES)
        throw std::invalid_argument("Tracking::UseRelocalisation: max_candidates outside [0, VX_MAX_RELOC_CANDIDATES]");
    if (max_candidates > 0 && !resident_) throw std::logic_error("Tracking::UseRelocalisation: requires UseResidentFrames(true)");
    reloc_candidates_ = max_candidates;
}

std::vector<Frame::Ptr> Tracking::RelocCandidates(const Map& map, int max_candidates) {
    std::vector<Frame::Ptr> out;
    const auto& kfs = map.KeyFrames();  // ascending ids
    for (auto it = kfs.rbegin(); it != kfs.rend() && (int)out.size() < max_candidates; ++it)
        if (it->second && it->second->Resident()) out.push_back(it->second);
    return out;
}

// ================= the entry point (tracking.cpp:39-89) =================

void Tracking::ProcessFrame(Frame::Ptr frame) {
    current_frame_ = frame;
    relocalised_ = false;

    if (resident_) {
        if (auto* orb = dynamic_cast<ORBExtractor*>(extractor_.get())) {
            orb->ExtractResident(*current_frame_);
        } else {
            extractor_->Extract(*current_frame_);
            if (!current_frame_->Resident())
                throw std::runtime_error("Tracking: resident frames, but the extractor left no resident handle on the frame");
        }
    } else {
        extractor_->Extract(*current_frame_);
    }
    bool just_initialized = false;

    if (state_ == State::INIT) {
        if (!init_frame_) {
            InitWithFirstFrame();  // success or not, the second frame is still to come (:47-52)
            return;
        } else {
            if (!InitWithSecondFrame()) return;
            UpdateTrackingState();
            last_frame_ = current_frame_;
            just_initialized = true;
        }
    } else if (state_ == State::TRACKING_GOOD) {
        if (!Track()) {
            HandleTrackingFailure();
            return;  // last_frame_ stays
        }
    } else if (state_ == State::TRACKING_BAD) {
        if (!HandleTrackingBad()) return;
    } else if (state_ == State::LOST) {
        if (!HandleTrackingLost()) return;
    }

    if (!just_initialized && NeedNewKeyFrame()) {
        CreateKeyFrame();
        if (options_.enable_culling) {
            culling_.CullLandmarks();
            culling_.CullKeyFrames(last_keyframe_, init_frame_, current_frame_);
        }
        if (local_ba_) local_ba_->Optimize(map_, last_keyframe_);
    }

    UpdateTrackingState();
    last_frame_ = current_frame_;
}

// ================= initialisation =================

// tracking.cpp:177-204: the feature count, CheckFeatureDistribution and CheckImageQuality as one call
bool Tracking::InitWithFirstFrame() {
    // resident frames: the gate stays the host-input one (the image is on the host anyway), after one
    // fetch of the keypoints
    if (resident_) Materialize(dmap_->context(), *current_frame_, false);
    const auto& feats = current_frame_->Features();
    const ImageU8& image = current_frame_->Image();
    last_gate_ = vx_init_gate_result{};
    last_gate_.n_features = (int32_t)feats.size();
    if (image.empty()) {
        // (:179 is decided before the image is looked at: a frame that failed to load, with no
        // features, waits for a better one as in the reference; cvtColor would throw on the rest)
        if (feats.size() >= static_cast<size_t>(options_.min_matches))
            throw std::invalid_argument("Tracking::InitWithFirstFrame: the frame has no image");
        last_gate_.status = VX_INIT_FEW_FEATURES;
        return false;
    }
    xy_.resize(2 * feats.size());
    for (size_t i = 0; i < feats.size(); ++i) {
        const float x = (float)feats[i].position.x, y = (float)feats[i].position.y;
        if ((double)x != feats[i].position.x || (double)y != feats[i].position.y)
            throw std::invalid_argument("Tracking::InitWithFirstFrame: feature position is not float-representable");
        xy_[2 * i] = x;
        xy_[2 * i + 1] = y;
    }
    vx_init_gate_options o;
    vx_init_gate_default_options(&o);
    o.min_features = options_.min_matches;
    vx_ctx* c = dmap_->context();
    int rc = vx_init_gate_host_async(c, image.ptr(), image.cols, image.rows, image.channels, (int64_t)image.step(),
                                     xy_.data(), 8, (int)feats.size(), &o);
    if (rc != VX_OK) throw std::runtime_error(std::string("vx_init_gate_host_async: ") + vx_last_error(c));
    rc = vx_init_gate_fetch(c, &last_gate_);
    if (rc != VX_OK) throw std::runtime_error(std::string("vx_init_gate_fetch: ") + vx_last_error(c));
    if (last_gate_.status != VX_INIT_OK) return false;

    init_frame_ = current_frame_;
    init_frame_->SetPose(SE3d());
    return true;
}

// tracking.cpp:206-263
bool Tracking::InitWithSecondFrame() {
    EssentialTracker& essential = tracker_.Essential();
    if (!(resident_ ? tracker_.EstimateInitialPoseResident(init_frame_, current_frame_)
                    : essential.EstimateInitialPose(init_frame_, current_frame_)))
        return false;  // :207-245
    keyframes_.CreateKeyFrame(nullptr, init_frame_);          // init's depth landmarks, its insertion (:248, :255)
    keyframes_.CreateKeyFrame(init_frame_, current_frame_);   // current's depth landmarks, triangulation (:249-256)
    last_keyframe_ = current_frame_;
    last_parallax_ = essential.LastParallax();
    last_inliers_ = essential.LastInliers();
    return true;
}

// ================= tracking (tracking.cpp:267-279) =================

bool Tracking::Track() {
    if (!(resident_ ? tracker_.TrackResident(last_keyframe_, last_frame_, current_frame_)
                    : tracker_.Track(last_keyframe_, last_frame_, current_frame_)))
        return false;
    last_parallax_ = tracker_.LastParallax();  // :325 / :449
    last_inliers_ = tracker_.LastInliers();    // :324 / :450
    return true;
}

// ================= state (tracking.cpp:459-499) =================

void Tracking::UpdateTrackingState() {
    state_ = last_inliers_ >= options_.min_inliers ? State::TRACKING_GOOD : State::TRACKING_BAD;
}

void Tracking::HandleTrackingFailure() {
    state_ = state_ == State::TRACKING_GOOD ? State::TRACKING_BAD : State::LOST;
}

void Tracking::Reset() {
    state_ = State::INIT;
    map_->removeAll();
    dmap_->removeAll();
    init_frame_.reset();
    last_frame_.reset();
    last_keyframe_.reset();
    last_inliers_ = 0;
    last_parallax_ = 0.0;
}

// The reference's TODO (:477-499): before the map is thrown away, one PnP of current_frame_ over the landmarks
// of the map's latest keyframes.  On success the frame is a tracked frame (:76-88 follow in ProcessFrame).
bool Tracking::Relocalise() {
    if (reloc_candidates_ <= 0) return false;
    const std::vector<Frame::Ptr> cands = RelocCandidates(*map_, reloc_candidates_);
    if (!tracker_.Relocalize(cands, current_frame_)) return false;
    last_keyframe_ = tracker_.RelocBestKeyFrame();
    last_parallax_ = tracker_.LastParallax();
    last_inliers_ = tracker_.LastInliers();
    relocalised_ = true;
    return true;
}

bool Tracking::HandleTrackingBad() {
    if (Relocalise()) return true;
    Reset();
    return false;
}

bool Tracking::HandleTrackingLost() {
    if (Relocalise()) return true;
    Reset();
    return false;
}

// ================= keyframes (tracking.cpp:562-584) =================

bool Tracking::NeedNewKeyFrame() const {
    if (state_ != State::TRACKING_GOOD) return false;
    if (!current_frame_ || !last_keyframe_) return false;
    if (last_inliers_ < options_.min_keyframe_inliers) return false;
    if (last_parallax_ < options_.min_parallax) return false;
    if (current_frame_->Id() - last_keyframe_->Id() < static_cast<uint64_t>(options_.min_keyframe_gap)) return false;
    return true;
}

void Tracking::CreateKeyFrame() {
    keyframes_.CreateKeyFrame(last_keyframe_, current_frame_);  // :578-579, :581 on the resident map
    last_keyframe_ = current_frame_;
}

}  // namespace visionx
