// mapping.cpp — KeyFrameLandmarks over vx_depth_landmarks / vx_triangulate (see mapping.h).
#include "visionx/mapping.h"
#include "visionx/tracking.h"

#include "visionx/device_map.h"

#include <cstdio>
#include <stdexcept>
#include <string>

namespace visionx {

namespace vxhost {
vx_ctx* ThreadContext();  // feature.cpp
}

static void check(vx_ctx* c, int rc, const char* what) {
    if (rc != VX_OK) throw std::runtime_error(std::string(what) + ": " + vx_last_error(c));
}

static void pose7(const SE3d& T, double* p) {
    p[0] = T.qx; p[1] = T.qy; p[2] = T.qz; p[3] = T.qw;
    p[4] = T.tx; p[5] = T.ty; p[6] = T.tz;
}

// tracking.cpp:586-650
void KeyFrameLandmarks::CreateLandmarksFromDepth(const Frame::Ptr& frame) {
    if (!map_ || !frame) return;
    const DepthImage& depth = frame->Depth();
    if (depth.empty()) return;
    const auto cam = frame->GetCamera();
    if (!cam) return;
    auto& features = frame->Features();
    const int n = (int)features.size();
    uv_.resize(2 * (size_t)n);
    has_.resize(n);
    for (int i = 0; i < n; ++i) {
        uv_[2 * i] = features[i].position.x;
        uv_[2 * i + 1] = features[i].position.y;
        has_[i] = features[i].has_landmark ? 1 : 0;
    }
    const double intr[4] = {cam->fx(), cam->fy(), cam->cx(), cam->cy()};
    double T[7];
    pose7(frame->Pose(), T);
    idx_.assign(n, -1);
    pw_.resize(3 * (size_t)n);
    int created = 0;
    vx_ctx* c = vxhost::ThreadContext();
    check(c, vx_depth_landmarks(c, uv_.data(), has_.data(), n, depth.ptr(), depth.type, depth.rows, depth.cols,
                                (int64_t)depth.step, intr, T, idx_.data(), pw_.data(), &created),
          "vx_depth_landmarks");
    for (int i = 0; i < n; ++i) {  // the loop body of tracking.cpp:634-643, in feature order
        if (idx_[i] < 0) continue;
        const double* p = &pw_[3 * (size_t)idx_[i]];
        auto lm = std::make_shared<Landmark>(landmark_id_++, Vec3d(p[0], p[1], p[2]));
        lm->AddObservation(frame->Id(), (size_t)i);
        map_->InsertLandmark(lm);
        features[i].landmark_id_ = lm->Id();
        features[i].has_landmark = true;
        features[i].is_outlier = false;
    }
}

// tracking.cpp:856-929
void KeyFrameLandmarks::TriangulateWithLastKeyFrame(Frame::Ptr last_frame, Frame::Ptr curr_frame) {
    if (!last_frame || !curr_frame) {
        std::fprintf(stderr, "[TriangulateWithLastKeyFrame] Invalid frames.\n");
        return;
    }
    std::vector<DMatch> matches;
    matcher_->Match(last_frame, curr_frame, matches);
    auto cam = curr_frame->GetCamera();
    auto cam1 = last_frame->GetCamera();
    if (!cam || !cam1 || matches.empty()) return;
    auto& f1 = last_frame->Features();
    auto& f2 = curr_frame->Features();
    const int n1 = (int)f1.size(), n2 = (int)f2.size(), nm = (int)matches.size();
    uv_.resize(2 * (size_t)n1);
    has_.resize(n1);
    uv2_.resize(2 * (size_t)n2);
    has2_.resize(n2);
    for (int i = 0; i < n1; ++i) {
        uv_[2 * i] = f1[i].position.x;
        uv_[2 * i + 1] = f1[i].position.y;
        has_[i] = f1[i].has_landmark ? 1 : 0;
    }
    for (int i = 0; i < n2; ++i) {
        uv2_[2 * i] = f2[i].position.x;
        uv2_[2 * i + 1] = f2[i].position.y;
        has2_[i] = f2[i].has_landmark ? 1 : 0;
    }
    m_.resize(nm);
    for (int k = 0; k < nm; ++k) m_[k] = vx_match{matches[k].queryIdx, matches[k].trainIdx, matches[k].distance};
    const double i1[4] = {cam1->fx(), cam1->fy(), cam1->cx(), cam1->cy()};
    const double i2[4] = {cam->fx(), cam->fy(), cam->cx(), cam->cy()};
    double T1[7], T2[7];
    pose7(last_frame->Pose(), T1);
    pose7(curr_frame->Pose(), T2);
    idx_.assign(nm, -1);
    pw_.resize(3 * (size_t)nm);
    int created = 0;
    vx_ctx* c = vxhost::ThreadContext();
    check(c, vx_triangulate(c, uv_.data(), has_.data(), n1, i1, T1, uv2_.data(), has2_.data(), n2, i2, T2, m_.data(),
                            nm, options_.triangulation_min_angle_deg, options_.triangulation_max_reproj_error,
                            idx_.data(), pw_.data(), &created),
          "vx_triangulate");
    for (int k = 0; k < nm; ++k) {  // the loop body of tracking.cpp:915-925, in match order
        if (idx_[k] < 0) continue;
        const double* p = &pw_[3 * (size_t)idx_[k]];
        const auto& m = matches[k];
        auto lm = std::make_shared<Landmark>(landmark_id_++, Vec3d(p[0], p[1], p[2]));
        lm->AddObservation(last_frame->Id(), (size_t)m.queryIdx);
        lm->AddObservation(curr_frame->Id(), (size_t)m.trainIdx);
        map_->InsertLandmark(lm);
        f1[m.queryIdx].landmark_id_ = lm->Id();
        f1[m.queryIdx].has_landmark = true;
        f1[m.queryIdx].is_outlier = false;
        f2[m.trainIdx].landmark_id_ = lm->Id();
        f2[m.trainIdx].has_landmark = true;
        f2[m.trainIdx].is_outlier = false;
    }
}

// tracking.cpp:577-581 on the resident map
uint64_t KeyFrameLandmarks::CreateKeyFrame(Frame::Ptr last_frame, Frame::Ptr curr_frame) {
    if (!dmap_) throw std::runtime_error("KeyFrameLandmarks::CreateKeyFrame: no DeviceMap (UseDeviceMap)");
    if (!map_ || !curr_frame) return landmark_id_;
    const auto cam = curr_frame->GetCamera();
    if (!cam) throw std::runtime_error("KeyFrameLandmarks::CreateKeyFrame: the frame has no camera");
    auto& f2 = curr_frame->Features();
    const double intr[4] = {cam->fx(), cam->fy(), cam->cx(), cam->cy()};
    double T[7];
    pose7(curr_frame->Pose(), T);
    const DepthImage& depth = curr_frame->Depth();
    const vx_keyframe_options o{options_.triangulation_min_angle_deg, options_.triangulation_max_reproj_error};
    dmap_->Flush();  // queued edits first: the call reads the resident map
    vx_ctx* c = dmap_->context();
    vx_keyframe_result res{};
    if (tracks_ && curr_frame->Resident() && (!last_frame || last_frame->Resident())) {
        // resident frames: the track's own match list (tracking.cpp:340 / :208 matched these two frames
        // a moment ago), or a device match when it holds none; no host matcher either way
        const vx_match* dm = nullptr;
        const int32_t* dn = nullptr;
        int32_t mcap = 0;
        if (last_frame && !tracks_->MatchList(last_frame->Id(), curr_frame->Id(), &dm, &dn, &mcap)) {
            const uint8_t *qd, *td;
            const int32_t *qn, *tn;
            int32_t qc, tc;
            check(c, vx_frame_device(last_frame->Resident()->handle(), nullptr, nullptr, &qd, &qn, &qc), "vx_frame_device");
            check(c, vx_frame_device(curr_frame->Resident()->handle(), nullptr, nullptr, &td, &tn, &tc), "vx_frame_device");
            check(c, vx_match_device_async(c, qd, qn, qc, td, tn, tc, tracks_->Ratio()), "vx_match_device_async");
        }
        check(c, vx_dmap_create_keyframe_frame(c, dmap_->handle(), curr_frame->Id(), T, intr, curr_frame->Resident()->handle(),
                                               last_frame ? 1 : 0, last_frame ? last_frame->Id() : 0, dm, dn, mcap,
                                               depth.empty() ? nullptr : depth.ptr(), depth.type, depth.rows, depth.cols,
                                               (int64_t)depth.step, landmark_id_, &o, &res),
              "vx_dmap_create_keyframe_frame");
    } else {
        std::vector<DMatch> matches;
        if (last_frame) matcher_->Match(last_frame, curr_frame, matches);
        const int n = (int)f2.size(), nm = (int)matches.size();
        uv_.resize(2 * (size_t)n);
        for (int i = 0; i < n; ++i) {
            uv_[2 * i] = f2[i].position.x;
            uv_[2 * i + 1] = f2[i].position.y;
        }
        m_.resize(nm);
        for (int k = 0; k < nm; ++k) m_[k] = vx_match{matches[k].queryIdx, matches[k].trainIdx, matches[k].distance};
        check(c, vx_dmap_create_keyframe_host(c, dmap_->handle(), curr_frame->Id(), T, intr, uv_.data(), n,
                                              last_frame ? 1 : 0, last_frame ? last_frame->Id() : 0, m_.data(), nm,
                                              depth.empty() ? nullptr : depth.ptr(), depth.type, depth.rows, depth.cols,
                                              (int64_t)depth.step, landmark_id_, &o, &res),
              "vx_dmap_create_keyframe_host");
    }
    int n_rec = 0;
    rec_.resize((size_t)res.n_depth + (size_t)res.n_triangulated);
    check(c, vx_dmap_create_results(dmap_->handle(), (int)rec_.size(), rec_.data(), &n_rec), "vx_dmap_create_results");
    ApplyRecords(last_frame, curr_frame, rec_.data(), rec_.size());
    landmark_id_ = res.next_landmark_id;
    return landmark_id_;
}

// the loop bodies of tracking.cpp:634-643 and :915-925 over one keyframe's records, then :581
void KeyFrameLandmarks::ApplyRecords(const Frame::Ptr& last_frame, const Frame::Ptr& curr_frame,
                                     const vx_keyframe_landmark* rec, size_t n) {
    auto& f2 = curr_frame->Features();
    std::vector<Landmark::Ptr> made;
    made.reserve(n);
    for (size_t i = 0; i < n; ++i) {
        const vx_keyframe_landmark& r = rec[i];
        auto lm = std::make_shared<Landmark>(r.lm_id, Vec3d(r.pw[0], r.pw[1], r.pw[2]));
        if (r.kind == 1) {
            lm->AddObservation(last_frame->Id(), (size_t)r.feat_last);
            Feature& a = last_frame->Features()[(size_t)r.feat_last];
            a.landmark_id_ = lm->Id();
            a.has_landmark = true;
            a.is_outlier = false;
        }
        lm->AddObservation(curr_frame->Id(), (size_t)r.feat_curr);
        map_->InsertLandmark(lm);
        Feature& b = f2[(size_t)r.feat_curr];
        b.landmark_id_ = lm->Id();
        b.has_landmark = true;
        b.is_outlier = false;
        made.push_back(std::move(lm));
    }
    map_->InsertKeyFrame(curr_frame);  // tracking.cpp:581
    dmap_->Created(n ? rec[0].row : 0, made, curr_frame);
}

// tracking.cpp:577-581 for every camera of a rig step that inserts a keyframe
uint64_t KeyFrameLandmarks::CreateKeyFrameRig(const std::vector<std::pair<Frame::Ptr, Frame::Ptr>>& last_curr) {
    if (!dmap_) throw std::runtime_error("KeyFrameLandmarks::CreateKeyFrameRig: no DeviceMap (UseDeviceMap)");
    // one rig call needs the map, 1 .. VX_MAX_RIG_CAMERAS resident current frames with a camera, and the
    // tracker's own list for every pair that has a last frame; anything else goes pair by pair
    const size_t n = last_curr.size();
    bool rig = tracks_ && map_ && n >= 1 && n <= (size_t)VX_MAX_RIG_CAMERAS;
    std::vector<vx_rig_keyframe> table(rig ? n : 0);
    std::vector<double> host(rig ? 11 * n : 0);  // per camera: pose7 | intr4
    for (size_t i = 0; rig && i < n; ++i) {
        const Frame::Ptr& last = last_curr[i].first;
        const Frame::Ptr& curr = last_curr[i].second;
        if (!curr || !curr->Resident() || !curr->GetCamera() || (last && !last->Resident())) {
            rig = false;
            break;
        }
        vx_rig_keyframe& t = table[i];
        t = vx_rig_keyframe{};
        if (last && !tracks_->MatchList(last->Id(), curr->Id(), &t.d_matches, &t.d_n_matches, &t.cap_matches)) {
            rig = false;
            break;
        }
        const auto cam = curr->GetCamera();
        double* T = &host[11 * i];
        double* intr = T + 7;
        pose7(curr->Pose(), T);
        intr[0] = cam->fx(); intr[1] = cam->fy(); intr[2] = cam->cx(); intr[3] = cam->cy();
        const DepthImage& depth = curr->Depth();
        t.kf_id = curr->Id();
        t.pose7 = T;
        t.intr4 = intr;
        t.curr = curr->Resident()->handle();
        t.has_last = last ? 1 : 0;
        t.last_kf_id = last ? last->Id() : 0;
        t.depth = depth.empty() ? nullptr : depth.ptr();
        t.depth_type = depth.type;
        t.rows = depth.rows;
        t.cols = depth.cols;
        t.row_stride = (int64_t)depth.step;
    }
    if (!rig) {
        for (const auto& p : last_curr) CreateKeyFrame(p.first, p.second);
        return landmark_id_;
    }
    const vx_keyframe_options o{options_.triangulation_min_angle_deg, options_.triangulation_max_reproj_error};
    dmap_->Flush();  // queued edits first: the call reads the resident map
    vx_ctx* c = dmap_->context();
    std::vector<vx_keyframe_result> res(n);
    check(c, vx_dmap_create_keyframes_rig(c, dmap_->handle(), (int)n, table.data(), landmark_id_, &o, res.data()),
          "vx_dmap_create_keyframes_rig");
    size_t total = 0;
    for (const vx_keyframe_result& r : res) total += (size_t)r.n_depth + (size_t)r.n_triangulated;
    int n_rec = 0;
    rec_.resize(total);
    check(c, vx_dmap_create_results(dmap_->handle(), (int)rec_.size(), rec_.data(), &n_rec), "vx_dmap_create_results");
    size_t at = 0;
    for (size_t i = 0; i < n; ++i) {  // camera i's slice of the records, in camera order
        const size_t k = (size_t)res[i].n_depth + (size_t)res[i].n_triangulated;
        ApplyRecords(last_curr[i].first, last_curr[i].second, rec_.data() + at, k);
        at += k;
    }
    landmark_id_ = res[n - 1].next_landmark_id;
    return landmark_id_;
}

}  // namespace visionx
