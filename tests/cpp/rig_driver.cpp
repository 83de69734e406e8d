// rig_driver.cpp — drives the rig adapters (visionx-slam_amd/host: FrameTracker::TrackRig,
// ORBExtractor::ExtractResidentBatch) beside the single-camera resident ones on the same scenes, for
// tests/test_gpu_track_rig_adapter.py.
//
//   rig_driver track <dir> <cameras> <keyframe camera>
//     reads  per camera i, <dir>/cam<i>/: resident_driver's `track` files (last_xy.bin / curr_xy.bin (f32 x2),
//            desc_last.bin / desc_curr.bin / desc_kf.bin (u8 x32), intr.bin (f64 x4), pose_last.bin /
//            kf_pose.bin (f64 x7), kf_uv.bin (f64 x2), lm_id.bin (u64, distinct over the cameras), flags.bin
//            (u8), lm_pos.bin (f64 x3), lm_bad.bin (u8)).  Camera i's last keyframe is keyframe 100 + i, its
//            last frame 200 + i and its current frame 300 + i of ONE map.
//     runs   two worlds, each a Map with every camera's keyframe mirrored on a resident map of its own, the
//            frames holding resident handles only: in `single`, one FrameTracker::TrackResident per camera
//            (a tracker of its own each); in `rig`, ONE FrameTracker::TrackRig over all cameras.  In both,
//            KeyFrameLandmarks::CreateKeyFrame of the keyframe camera's current frame on the track's list
//            (UseTrackLists): in `single` right after that camera's track (the next TrackResident on the
//            context overwrites the list), in `rig` after the one call.
//     writes pose_single_<i>.out, pose_rig_<i>.out (f64 x7)
//     prints single <i> <returned> <UsedFallback> <LastInliers> <LastParallax, 17 digits>
//            rig    <i> <the same four> <Features() equal the single world's> <Descriptors() empty>
//            list <world> <the tracker holds Match(keyframe, current) of the keyframe camera>
//            initlm <world> <next landmark id> <records> then <landmark id>:<observed by the keyframe | 2 * by
//                   the new keyframe> for every landmark of the map
//   rig_driver extract <dir> <width> <height> <channels>
//     reads  images.bin (u8: frames of height x width x channels back to back)
//     runs   ORBExtractor::ExtractResident on each and ExtractResidentBatch on all (+ vx_frame_fetch)
//     prints per image: <features> <keypoints equal> <descriptors equal> <Features() / Descriptors() untouched>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "visionx/device_map.h"
#include "visionx/feature.h"
#include "visionx/mapping.h"
#include "visionx/tracking.h"

using namespace visionx;

template <class T>
static std::vector<T> read_bin(const std::string& path) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) {
        std::cerr << "cannot open " << path << "\n";
        std::exit(2);
    }
    const size_t n = (size_t)f.tellg();
    f.seekg(0);
    std::vector<T> v(n / sizeof(T));
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
    return v;
}

template <class T>
static void write_bin(const std::string& path, const T* p, size_t n) {
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(p), (std::streamsize)(n * sizeof(T)));
}

static SE3d to_se3(const std::vector<double>& p) {
    SE3d T;
    T.qx = p[0]; T.qy = p[1]; T.qz = p[2]; T.qw = p[3];
    T.tx = p[4]; T.ty = p[5]; T.tz = p[6];
    return T;
}

static void write_pose(const std::string& path, const SE3d& P) {
    const double pose[7] = {P.qx, P.qy, P.qz, P.qw, P.tx, P.ty, P.tz};
    write_bin(path, pose, 7);
}

static bool same_features(const std::vector<Feature>& a, const std::vector<Feature>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].position.x != b[i].position.x || a[i].position.y != b[i].position.y || a[i].response != b[i].response)
            return false;
    return true;
}

struct CamFiles {
    std::vector<double> intr, pose_last, kf_pose, kf_uv, lm_pos;
    std::vector<float> last_xy, curr_xy;
    std::vector<uint8_t> desc_last, desc_curr, desc_kf, flags, lm_bad;
    std::vector<uint64_t> lm_id;
};

static CamFiles read_cam(const std::string& dir) {
    CamFiles s;
    s.intr = read_bin<double>(dir + "/intr.bin");
    s.pose_last = read_bin<double>(dir + "/pose_last.bin");
    s.kf_pose = read_bin<double>(dir + "/kf_pose.bin");
    s.last_xy = read_bin<float>(dir + "/last_xy.bin");
    s.curr_xy = read_bin<float>(dir + "/curr_xy.bin");
    s.desc_last = read_bin<uint8_t>(dir + "/desc_last.bin");
    s.desc_curr = read_bin<uint8_t>(dir + "/desc_curr.bin");
    s.desc_kf = read_bin<uint8_t>(dir + "/desc_kf.bin");
    s.kf_uv = read_bin<double>(dir + "/kf_uv.bin");
    s.lm_id = read_bin<uint64_t>(dir + "/lm_id.bin");
    s.flags = read_bin<uint8_t>(dir + "/flags.bin");
    s.lm_pos = read_bin<double>(dir + "/lm_pos.bin");
    s.lm_bad = read_bin<uint8_t>(dir + "/lm_bad.bin");
    const size_t n = s.flags.size();
    if (s.intr.size() != 4 || s.pose_last.size() != 7 || s.kf_pose.size() != 7 || s.kf_uv.size() != 2 * n || s.lm_id.size() != n ||
        s.lm_pos.size() != 3 * n || s.lm_bad.size() != n || s.desc_kf.size() != 32 * n || s.desc_last.size() != 16 * s.last_xy.size() ||
        s.desc_curr.size() != 16 * s.curr_xy.size()) {
        std::cerr << "inconsistent scene files in " << dir << "\n";
        std::exit(2);
    }
    return s;
}

// one world: the map with every camera's last keyframe, its resident mirror, the frames (handles only)
struct World {
    Map::Ptr map = std::make_shared<Map>();
    DeviceMap::Ptr dmap = std::make_shared<DeviceMap>();
    std::vector<Frame::Ptr> kf, last, curr;
};

static void build_world(World& w, const std::vector<CamFiles>& cams) {
    std::vector<std::vector<float>> kf_xy(cams.size());
    for (size_t i = 0; i < cams.size(); ++i) {
        const CamFiles& s = cams[i];
        const size_t n = s.flags.size();
        auto cam = std::make_shared<Camera>(s.intr[0], s.intr[1], s.intr[2], s.intr[3]);
        auto kf = std::make_shared<Frame>(100 + i, 0.0, cam, ImageU8());
        kf->SetPose(to_se3(s.kf_pose));
        kf->Features().resize(n);
        kf_xy[i].resize(2 * n);
        for (size_t k = 0; k < n; ++k) {
            Feature& f = kf->Features()[k];
            f.position = Vec2d(s.kf_uv[2 * k], s.kf_uv[2 * k + 1]);
            kf_xy[i][2 * k] = (float)s.kf_uv[2 * k];
            kf_xy[i][2 * k + 1] = (float)s.kf_uv[2 * k + 1];
            f.landmark_id_ = s.lm_id[k];
            f.has_landmark = (s.flags[k] & 1) != 0;
            f.is_outlier = (s.flags[k] & 2) != 0;
            auto lm = std::make_shared<Landmark>(s.lm_id[k], Vec3d(s.lm_pos[3 * k], s.lm_pos[3 * k + 1], s.lm_pos[3 * k + 2]));
            lm->SetBad(s.lm_bad[k] == 1);
            lm->AddObservation(kf->Id(), k);
            w.map->InsertLandmark(lm);
        }
        kf->Descriptors().rows = (int)n;
        kf->Descriptors().data = s.desc_kf;
        w.map->InsertKeyFrame(kf);
        w.kf.push_back(kf);
        auto last = std::make_shared<Frame>(200 + i, 0.1, cam, ImageU8());
        last->SetPose(to_se3(s.pose_last));
        w.last.push_back(last);
        w.curr.push_back(std::make_shared<Frame>(300 + i, 0.2, cam, ImageU8()));
    }
    w.dmap->Mirror(*w.map);
    vx_ctx* c = w.dmap->context();
    for (size_t i = 0; i < cams.size(); ++i) {
        const CamFiles& s = cams[i];
        UploadResident(c, *w.kf[i], kf_xy[i].data(), s.desc_kf.data(), (int)s.flags.size());
        UploadResident(c, *w.last[i], s.last_xy.data(), s.desc_last.data(), (int)(s.last_xy.size() / 2));
        UploadResident(c, *w.curr[i], s.curr_xy.data(), s.desc_curr.data(), (int)(s.curr_xy.size() / 2));
    }
}

// CreateKeyFrame of camera k's current frame on the tracker's list; prints the list and initlm lines
static void create_keyframe(const char* world, World& w, const FrameTracker& tracker, size_t k) {
    const vx_match* dm = nullptr;
    const int32_t* dn = nullptr;
    int32_t cap = 0;
    std::printf("list %s %d\n", world, tracker.MatchList(w.kf[k]->Id(), w.curr[k]->Id(), &dm, &dn, &cap) ? 1 : 0);
    KeyFrameLandmarks keyframes(w.map, std::make_shared<ORBMatcher>(), KeyFrameLandmarks::Options());
    keyframes.UseDeviceMap(w.dmap);
    keyframes.UseTrackLists(&tracker);
    keyframes.landmark_id_ = 50000000;
    const uint64_t next = keyframes.CreateKeyFrame(w.kf[k], w.curr[k]);
    std::vector<Landmark::Ptr> lms;
    for (const auto& kv : w.map->Landmarks()) lms.push_back(kv.second);
    std::sort(lms.begin(), lms.end(), [](const Landmark::Ptr& a, const Landmark::Ptr& b) { return a->Id() < b->Id(); });
    std::printf("initlm %s %llu %zu", world, (unsigned long long)next, keyframes.LastRecords().size());
    for (const auto& lm : lms) {
        const auto& ob = lm->Observations();
        std::printf(" %llu:%d", (unsigned long long)lm->Id(), (ob.count(w.kf[k]->Id()) ? 1 : 0) | (ob.count(w.curr[k]->Id()) ? 2 : 0));
    }
    std::printf("\n");
}

static int cmd_track(const std::string& dir, int n_cams, int kf_cam) {
    std::vector<CamFiles> cams;
    for (int i = 0; i < n_cams; ++i) cams.push_back(read_cam(dir + "/cam" + std::to_string(i)));
    World ws, wr;
    build_world(ws, cams);
    build_world(wr, cams);
    // single: one TrackResident per camera, a tracker of its own each
    std::vector<std::unique_ptr<FrameTracker>> singles;
    for (int i = 0; i < n_cams; ++i) {
        singles.push_back(std::make_unique<FrameTracker>(ws.dmap));
        FrameTracker& t = *singles.back();
        const bool ok = t.TrackResident(ws.kf[i], ws.last[i], ws.curr[i]);
        write_pose(dir + "/pose_single_" + std::to_string(i) + ".out", ws.curr[i]->Pose());
        std::printf("single %d %d %d %d %.17g\n", i, ok ? 1 : 0, t.UsedFallback() ? 1 : 0, t.LastInliers(), t.LastParallax());
        // (the single call's lists live until the next TrackResident on the context: the keyframe comes first)
        if (i == kf_cam) create_keyframe("single", ws, t, (size_t)i);
    }
    // rig: one TrackRig
    FrameTracker rig(wr.dmap);
    std::vector<FrameTracker::RigCamera> rc;
    for (int i = 0; i < n_cams; ++i) rc.push_back({wr.kf[i], wr.last[i], wr.curr[i]});
    const std::vector<bool> ok = rig.TrackRig(rc);
    for (int i = 0; i < n_cams; ++i) {
        write_pose(dir + "/pose_rig_" + std::to_string(i) + ".out", wr.curr[i]->Pose());
        std::printf("rig %d %d %d %d %.17g %d %d\n", i, ok[i] ? 1 : 0, rig.RigUsedFallback(i) ? 1 : 0, rig.RigLastInliers(i),
                    rig.RigLastParallax(i), same_features(wr.curr[i]->Features(), ws.curr[i]->Features()) ? 1 : 0,
                    wr.curr[i]->Descriptors().empty() ? 1 : 0);
    }
    if (kf_cam >= 0 && kf_cam < n_cams) create_keyframe("rig", wr, rig, (size_t)kf_cam);
    return 0;
}

static int cmd_extract(const std::string& dir, int w, int h, int ch) {
    const auto images = read_bin<uint8_t>(dir + "/images.bin");
    const size_t bytes = (size_t)w * h * ch;
    if (bytes == 0 || images.size() % bytes) {
        std::cerr << "inconsistent image file\n";
        return 2;
    }
    auto cam = std::make_shared<Camera>(300.0, 300.0, w / 2.0, h / 2.0);
    ORBExtractor extractor(400);
    vx_ctx* c = vxhost::ThreadContext();
    std::vector<Frame::Ptr> one, batch;
    for (size_t k = 0; k < images.size() / bytes; ++k) {
        ImageU8 im;
        im.rows = h;
        im.cols = w;
        im.channels = ch;
        im.data.assign(images.begin() + (std::ptrdiff_t)(k * bytes), images.begin() + (std::ptrdiff_t)((k + 1) * bytes));
        one.push_back(std::make_shared<Frame>(k, 0.0, cam, im));
        batch.push_back(std::make_shared<Frame>(k, 0.0, cam, im));
        extractor.ExtractResident(*one.back());
    }
    extractor.ExtractResidentBatch(batch);
    for (size_t k = 0; k < one.size(); ++k) {
        const int untouched = batch[k]->Features().empty() && batch[k]->Descriptors().empty() ? 1 : 0;
        int n[2] = {0, 0};
        std::vector<vx_keypoint> kp[2];
        std::vector<uint8_t> desc[2];
        const Frame::Ptr f[2] = {one[k], batch[k]};
        for (int m = 0; m < 2; ++m) {
            const int cap = f[m]->Resident()->capacity();
            kp[m].resize((size_t)cap);
            desc[m].resize((size_t)cap * 32);
            if (vx_frame_fetch(c, f[m]->Resident()->handle(), kp[m].data(), desc[m].data(), cap, &n[m]) != VX_OK) {
                std::cerr << "vx_frame_fetch: " << vx_last_error(c) << "\n";
                return 1;
            }
        }
        const bool kp_equal = n[0] == n[1] && std::memcmp(kp[0].data(), kp[1].data(), (size_t)n[0] * sizeof(vx_keypoint)) == 0;
        const bool desc_equal = n[0] == n[1] && std::memcmp(desc[0].data(), desc[1].data(), (size_t)n[0] * 32) == 0;
        std::printf("%d %d %d %d\n", n[1], kp_equal ? 1 : 0, desc_equal ? 1 : 0, untouched);
    }
    return 0;
}

int main(int argc, char** argv) {
    try {
        const std::string cmd = argc > 1 ? argv[1] : "";
        if (cmd == "track" && argc >= 5) return cmd_track(argv[2], std::atoi(argv[3]), std::atoi(argv[4]));
        if (cmd == "extract" && argc >= 6) return cmd_extract(argv[2], std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]));
        std::cerr << "usage: rig_driver track <dir> <cameras> <keyframe camera> | extract <dir> <width> <height> <channels>\n";
        return 2;
    } catch (const std::exception& e) {
        std::cerr << "error: " << e.what() << "\n";
        return 1;
    }
}
