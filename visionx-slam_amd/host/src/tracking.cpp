// tracking.cpp — visionx::PnPTracker over vx_track_pnp_host_async / vx_track_pnp_fetch (see tracking.h).
#include "visionx/tracking.h"

#include <array>
#include <cmath>
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

namespace vxhost {
vx_ctx* ThreadContext();  // feature.cpp
}

namespace {

// cv::Point2f(position.x(), position.y()) (tracking.cpp:512-513) for every feature
void NarrowPositions(const std::vector<Feature>& feats, std::vector<float>& xy) {
    xy.resize(2 * feats.size());
    for (size_t i = 0; i < feats.size(); ++i) {
        const float x = (float)feats[i].position.x, y = (float)feats[i].position.y;
        if ((double)x != feats[i].position.x || (double)y != feats[i].position.y)
            throw std::invalid_argument("EssentialTracker: feature position is not float-representable");
        xy[2 * i] = x;
        xy[2 * i + 1] = y;
    }
}

}  // namespace

bool EssentialTracker::Run(const Frame::Ptr& last, const Frame::Ptr& current, const double* pose_last7) {
    const auto cam = current->GetCamera();  // (:516)
    if (!cam) return false;
    const double intr[4] = {cam->fx(), cam->fy(), cam->cx(), cam->cy()};
    const int n_last = last->Descriptors().rows, n_curr = current->Descriptors().rows;
    if ((size_t)n_last != last->Features().size() || (size_t)n_curr != current->Features().size())
        throw std::invalid_argument("EssentialTracker: descriptors / features mismatch");
    NarrowPositions(last->Features(), xy_last_);
    NarrowPositions(current->Features(), xy_curr_);
    vx_track_essential_options o;
    vx_track_essential_default_options(&o);
    o.min_matches = options_.min_matches;
    o.min_inliers = options_.min_inliers;
    vx_ctx* c = ctx_ ? ctx_ : vxhost::ThreadContext();
    int rc = vx_track_essential_host_async(c, last->Descriptors().ptr(), n_last, xy_last_.data(),
                                           current->Descriptors().ptr(), n_curr, xy_curr_.data(), options_.nn_ratio,
                                           pose_last7, intr, &o);
    if (rc != VX_OK) throw std::runtime_error(std::string("vx_track_essential_host_async: ") + vx_last_error(c));
    rc = vx_track_essential_fetch(c, &last_, nullptr, nullptr, 0);
    if (rc != VX_OK) throw std::runtime_error(std::string("vx_track_essential_fetch: ") + vx_last_error(c));
    return last_.status == VX_TRACK_OK;
}

bool EssentialTracker::TrackLastFrame(const Frame::Ptr& last, const Frame::Ptr& current) {
    if (!last || !current) return false;  // tracking.cpp:282-285
    const SE3d L = last->Pose();
    const double pose_last[7] = {L.qx, L.qy, L.qz, L.qw, L.tx, L.ty, L.tz};
    if (!Run(last, current, pose_last)) return false;
    const double* p = last_.pose;  // T_cl * T_lw, composed on the device as SE3d::operator* would
    SE3d T;
    T.qx = p[0]; T.qy = p[1]; T.qz = p[2]; T.qw = p[3];
    T.tx = p[4]; T.ty = p[5]; T.tz = p[6];
    current->SetPose(T);
    last_inliers_ = last_.ess.n_inliers;  // (:324-325)
    last_parallax_ = last_.parallax;
    return true;
}

bool EssentialTracker::EstimateInitialPose(const Frame::Ptr& init, const Frame::Ptr& current) {
    if (!init || !current) return false;
    if (!Run(init, current, nullptr)) return false;  // T_lw = identity (:200)
    const double* p = last_.pose;
    SE3d T;
    T.qx = p[0]; T.qy = p[1]; T.qz = p[2]; T.qw = p[3];
    T.tx = p[4]; T.ty = p[5]; T.tz = p[6];
    current->SetPose(T);  // (:232 -> :541, before the parallax gate, as the reference)
    const float parallax = (float)last_.parallax;            // (:240)
    const float min_parallax = 1.0f * M_PI / 180.0f;         // (:241)
    if (parallax < min_parallax) return false;               // (:242)
    last_parallax_ = parallax;                               // (:259-260: the float, widened)
    last_inliers_ = last_.ess.n_inliers;
    return true;
}

FrameTracker::FrameTracker(DeviceMap::Ptr map, const Options& options)
    : pnp_(map, options.pnp), essential_(map ? map->context() : nullptr, options.essential) {}

bool FrameTracker::Track(const Frame::Ptr& last_keyframe, const Frame::Ptr& last_frame, const Frame::Ptr& current) {
    used_fallback_ = false;
    if (last_keyframe && pnp_.TrackWithPnP(last_keyframe, current)) return true;  // tracking.cpp:269-273
    used_fallback_ = true;
    return essential_.TrackLastFrame(last_frame, current);                        // (:278)
}

static void SetPose7(const Frame::Ptr& f, const double* p) {
    SE3d T;
    T.qx = p[0]; T.qy = p[1]; T.qz = p[2]; T.qw = p[3];
    T.tx = p[4]; T.ty = p[5]; T.tz = p[6];
    f->SetPose(T);
}

void FrameTracker::SetRatio(float nn_ratio) { pnp_.options_.nn_ratio = essential_.options_.nn_ratio = nn_ratio; }
float FrameTracker::Ratio() const { return pnp_.options_.nn_ratio; }
const DeviceMap::Ptr& FrameTracker::ResidentMap() const { return pnp_.map_; }

bool FrameTracker::MatchList(uint64_t query_id, uint64_t train_id, const vx_match** d_matches, const int32_t** d_n,
                             int32_t* cap) const {
    for (int which = 0; which < 2; ++which)
        if (list_valid_[which] && list_ids_[which][0] == query_id && list_ids_[which][1] == train_id)
            return vx_track_frame_matches(pnp_.map_->context(), which, d_matches, d_n, cap) == VX_OK;
    for (const RigState& r : rig_)
        for (int which = 0; which < 2; ++which)
            if (r.slot >= 0 && r.list_valid[which] && r.list_ids[which][0] == query_id && r.list_ids[which][1] == train_id)
                return vx_track_rig_matches(pnp_.map_->context(), r.slot, which, d_matches, d_n, cap) == VX_OK;
    if (reloc_slot_ >= 0 && reloc_ids_[0] == query_id && reloc_ids_[1] == train_id)
        return vx_relocalize_matches(pnp_.map_->context(), reloc_slot_, d_matches, d_n, cap) == VX_OK;
    return false;
}

// one vx_track_frame_async + fetch; fills resident_, current->Features() and the list ids
void FrameTracker::RunResident(const Frame::Ptr& last_keyframe, const Frame::Ptr& last_frame, const Frame::Ptr& current,
                               bool identity_last) {
    for (const Frame::Ptr& f : {last_keyframe, last_frame, current})
        if (f && !f->Resident()) throw std::invalid_argument("FrameTracker: a frame without a resident handle");
    if (pnp_.options_.nn_ratio != essential_.options_.nn_ratio)
        throw std::invalid_argument("FrameTracker: resident calls take one nn_ratio for both matches (SetRatio)");
    const auto cam = current->GetCamera();
    const double intr[4] = {cam->fx(), cam->fy(), cam->cx(), cam->cy()};
    DeviceMap::Ptr& map = pnp_.map_;
    map->Flush();
    vx_track_options po;
    vx_track_default_options(&po);
    po.min_matches = pnp_.options_.min_matches;
    po.min_inliers = pnp_.options_.min_inliers;
    po.pnp.reproj_error = pnp_.options_.max_reproj_error;
    vx_track_essential_options eo;
    vx_track_essential_default_options(&eo);
    eo.min_matches = essential_.options_.min_matches;
    eo.min_inliers = essential_.options_.min_inliers;
    double pose_last[7] = {0, 0, 0, 1, 0, 0, 0};
    if (last_frame && !identity_last) {
        const SE3d L = last_frame->Pose();
        const double p[7] = {L.qx, L.qy, L.qz, L.qw, L.tx, L.ty, L.tz};
        for (int i = 0; i < 7; ++i) pose_last[i] = p[i];
    }
    list_valid_[0] = list_valid_[1] = false;
    vx_ctx* c = map->context();
    int rc = vx_track_frame_async(c, map->handle(), last_keyframe ? last_keyframe->Id() : 0,
                                  last_keyframe ? last_keyframe->Resident()->handle() : nullptr,
                                  last_frame ? last_frame->Resident()->handle() : nullptr, current->Resident()->handle(),
                                  pnp_.options_.nn_ratio, identity_last ? nullptr : pose_last, intr, &po, &eo);
    if (rc != VX_OK) throw std::runtime_error(std::string("vx_track_frame_async: ") + vx_last_error(c));
    kp_.resize((size_t)current->Resident()->capacity());
    int n = 0;
    rc = vx_track_frame_fetch(c, &resident_, kp_.data(), (int)kp_.size(), &n);
    if (rc != VX_OK) throw std::runtime_error(std::string("vx_track_frame_fetch: ") + vx_last_error(c));
    auto& feats = current->Features();  // what ORBExtractor::Extract leaves there (orb_extractor.cpp:19-24)
    feats.assign((size_t)n, Feature());
    for (int i = 0; i < n; ++i) {
        feats[i].position = Vec2d(kp_[i].x, kp_[i].y);
        feats[i].response = kp_[i].response;
    }
    if (last_keyframe) {
        list_ids_[0][0] = last_keyframe->Id(), list_ids_[0][1] = current->Id();
        list_valid_[0] = true;
    }
    if (last_frame && resident_.ess_ran) {  // (a closed gate leaves list 1 empty)
        list_ids_[1][0] = last_frame->Id(), list_ids_[1][1] = current->Id();
        list_valid_[1] = true;
    }
    if (resident_.pnp_ran) pnp_.last_ = resident_.pnp;
    if (resident_.ess_ran) essential_.last_ = resident_.ess;
}

bool FrameTracker::TrackResident(const Frame::Ptr& last_keyframe, const Frame::Ptr& last_frame, const Frame::Ptr& current) {
    used_fallback_ = false;
    if (!current) return false;  // tracking.cpp:333-336, :282-285
    if (!current->GetCamera() || (!last_keyframe && !last_frame)) {
        used_fallback_ = true;  // Track() gets to TrackLastFrame, which returns false (:282-285, :516)
        return false;
    }
    RunResident(last_keyframe, last_frame, current, false);
    if (resident_.path == VX_TRACK_PATH_PNP) {  // (:443-450)
        SetPose7(current, resident_.pose);
        pnp_.last_parallax_ = resident_.parallax;
        pnp_.last_inliers_ = resident_.n_inliers;
        return true;
    }
    used_fallback_ = true;
    if (resident_.path != VX_TRACK_PATH_ESSENTIAL) return false;
    SetPose7(current, resident_.pose);  // (:539-541, :324-325)
    essential_.last_inliers_ = resident_.n_inliers;
    essential_.last_parallax_ = resident_.parallax;
    return true;
}

std::vector<bool> FrameTracker::TrackRig(const std::vector<RigCamera>& cams) {
    if (cams.size() > (size_t)VX_MAX_RIG_CAMERAS) throw std::invalid_argument("FrameTracker::TrackRig: more than VX_MAX_RIG_CAMERAS cameras");
    if (pnp_.options_.nn_ratio != essential_.options_.nn_ratio)
        throw std::invalid_argument("FrameTracker: resident calls take one nn_ratio for both matches (SetRatio)");
    std::vector<bool> ok(cams.size(), false);
    rig_.resize(std::max(rig_.size(), cams.size()));
    for (RigState& r : rig_) {
        r.slot = -1;
        r.list_valid[0] = r.list_valid[1] = false;
    }
    // the cameras of the device call, with the host arrays their table entries point to
    std::vector<vx_rig_camera> table;
    std::vector<size_t> index;
    std::vector<std::array<double, 11>> host(cams.size());  // intr4 | pose_last7
    for (size_t i = 0; i < cams.size(); ++i) {
        const RigCamera& k = cams[i];
        rig_[i].used_fallback = false;
        if (!k.current) continue;  // tracking.cpp:333-336, :282-285
        if (!k.current->GetCamera() || (!k.last_keyframe && !k.last_frame)) {
            rig_[i].used_fallback = true;  // Track() gets to TrackLastFrame, which returns false (:282-285, :516)
            continue;
        }
        for (const Frame::Ptr& f : {k.last_keyframe, k.last_frame, k.current})
            if (f && !f->Resident()) throw std::invalid_argument("FrameTracker: a frame without a resident handle");
        const auto cam = k.current->GetCamera();
        host[i] = {cam->fx(), cam->fy(), cam->cx(), cam->cy(), 0, 0, 0, 1, 0, 0, 0};
        if (k.last_frame) {
            const SE3d L = k.last_frame->Pose();
            const double p[7] = {L.qx, L.qy, L.qz, L.qw, L.tx, L.ty, L.tz};
            for (int j = 0; j < 7; ++j) host[i][4 + j] = p[j];
        }
        vx_rig_camera t{};
        t.last_kf_id = k.last_keyframe ? k.last_keyframe->Id() : 0;
        t.last_kf = k.last_keyframe ? k.last_keyframe->Resident()->handle() : nullptr;
        t.last = k.last_frame ? k.last_frame->Resident()->handle() : nullptr;
        t.curr = k.current->Resident()->handle();
        t.intr4 = host[i].data();
        t.pose_last7 = host[i].data() + 4;
        rig_[i].slot = (int)table.size();
        table.push_back(t);
        index.push_back(i);
    }
    if (table.empty()) return ok;
    DeviceMap::Ptr& map = pnp_.map_;
    map->Flush();
    vx_track_options po;
    vx_track_default_options(&po);
    po.min_matches = pnp_.options_.min_matches;
    po.min_inliers = pnp_.options_.min_inliers;
    po.pnp.reproj_error = pnp_.options_.max_reproj_error;
    vx_track_essential_options eo;
    vx_track_essential_default_options(&eo);
    eo.min_matches = essential_.options_.min_matches;
    eo.min_inliers = essential_.options_.min_inliers;
    vx_ctx* c = map->context();
    int rc = vx_track_rig_async(c, map->handle(), (int)table.size(), table.data(), pnp_.options_.nn_ratio, &po, &eo);
    if (rc != VX_OK) throw std::runtime_error(std::string("vx_track_rig_async: ") + vx_last_error(c));
    std::vector<vx_track_frame_result> res(table.size());
    rc = vx_track_rig_fetch(c, 1, res.data(), (int)res.size(), nullptr);
    if (rc != VX_OK) throw std::runtime_error(std::string("vx_track_rig_fetch: ") + vx_last_error(c));
    for (size_t s = 0; s < table.size(); ++s) {
        const size_t i = index[s];
        const RigCamera& k = cams[i];
        RigState& r = rig_[i];
        r.result = res[s];
        kp_.resize((size_t)k.current->Resident()->capacity());
        int n = 0;
        rc = vx_track_rig_keypoints(c, (int)s, kp_.data(), (int)kp_.size(), &n);
        if (rc != VX_OK) throw std::runtime_error(std::string("vx_track_rig_keypoints: ") + vx_last_error(c));
        auto& feats = k.current->Features();  // as RunResident fills them
        feats.assign((size_t)n, Feature());
        for (int j = 0; j < n; ++j) {
            feats[j].position = Vec2d(kp_[j].x, kp_[j].y);
            feats[j].response = kp_[j].response;
        }
        if (k.last_keyframe) {
            r.list_ids[0][0] = k.last_keyframe->Id(), r.list_ids[0][1] = k.current->Id();
            r.list_valid[0] = true;
        }
        if (k.last_frame && r.result.ess_ran) {  // (a closed gate leaves list 1 empty)
            r.list_ids[1][0] = k.last_frame->Id(), r.list_ids[1][1] = k.current->Id();
            r.list_valid[1] = true;
        }
        if (r.result.path == VX_TRACK_PATH_PNP) {  // as TrackResident (:443-450)
            SetPose7(k.current, r.result.pose);
            r.pnp_parallax = r.result.parallax;
            r.pnp_inliers = r.result.n_inliers;
            ok[i] = true;
            continue;
        }
        r.used_fallback = true;
        if (r.result.path != VX_TRACK_PATH_ESSENTIAL) continue;
        SetPose7(k.current, r.result.pose);  // (:539-541, :324-325)
        r.ess_inliers = r.result.n_inliers;
        r.ess_parallax = r.result.parallax;
        ok[i] = true;
    }
    return ok;
}

bool FrameTracker::Relocalize(const std::vector<Frame::Ptr>& keyframes, const Frame::Ptr& current) {
    reloc_best_.reset();
    reloc_slot_ = -1;
    reloc_ = vx_reloc_result{};
    if (!current || keyframes.empty() || !current->GetCamera()) return false;
    if (keyframes.size() > (size_t)VX_MAX_RELOC_CANDIDATES)
        throw std::invalid_argument("FrameTracker::Relocalize: more than VX_MAX_RELOC_CANDIDATES keyframes");
    if (!current->Resident()) throw std::invalid_argument("FrameTracker: a frame without a resident handle");
    std::vector<vx_reloc_candidate> table;
    for (const Frame::Ptr& k : keyframes) {
        if (!k || !k->Resident()) throw std::invalid_argument("FrameTracker: a frame without a resident handle");
        table.push_back({k->Id(), k->Resident()->handle()});
    }
    const auto cam = current->GetCamera();
    const double intr[4] = {cam->fx(), cam->fy(), cam->cx(), cam->cy()};
    DeviceMap::Ptr& map = pnp_.map_;
    map->Flush();
    vx_track_options po;
    vx_track_default_options(&po);
    po.min_matches = pnp_.options_.min_matches;
    po.min_inliers = pnp_.options_.min_inliers;
    po.pnp.reproj_error = pnp_.options_.max_reproj_error;
    vx_ctx* c = map->context();
    int rc = vx_relocalize_async(c, map->handle(), (int)table.size(), table.data(), current->Resident()->handle(),
                                 pnp_.options_.nn_ratio, intr, &po);
    if (rc != VX_OK) throw std::runtime_error(std::string("vx_relocalize_async: ") + vx_last_error(c));
    rc = vx_relocalize_fetch(c, &reloc_, nullptr, nullptr, nullptr, nullptr, 0);
    if (rc != VX_OK) throw std::runtime_error(std::string("vx_relocalize_fetch: ") + vx_last_error(c));
    Materialize(c, *current, false);  // Features() as TrackResident leaves them
    if (reloc_.status != VX_TRACK_OK) return false;
    used_fallback_ = false;
    SetPose7(current, reloc_.pnp.pose);  // (:443-450)
    pnp_.last_parallax_ = reloc_.parallax;
    pnp_.last_inliers_ = reloc_.pnp.n_inliers;
    reloc_slot_ = reloc_.best_cand;
    reloc_best_ = keyframes[(size_t)reloc_.best_cand];
    reloc_ids_[0] = reloc_best_->Id(), reloc_ids_[1] = current->Id();
    return true;
}

bool FrameTracker::EstimateInitialPoseResident(const Frame::Ptr& init, const Frame::Ptr& current) {
    if (!init || !current || !current->GetCamera()) return false;
    RunResident(nullptr, init, current, true);  // T_lw = identity (:200)
    if (resident_.path != VX_TRACK_PATH_ESSENTIAL) return false;
    SetPose7(current, resident_.pose);                        // (:232 -> :541, before the parallax gate)
    const float parallax = (float)resident_.parallax;         // (:240)
    const float min_parallax = 1.0f * M_PI / 180.0f;          // (:241)
    if (parallax < min_parallax) return false;                // (:242)
    essential_.last_parallax_ = parallax;                     // (:259-260: the float, widened)
    essential_.last_inliers_ = resident_.n_inliers;
    return true;
}

}  // namespace visionx
