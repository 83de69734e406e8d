// track_driver.cpp — drives visionx::PnPTracker (visionx-slam_amd/host/include/visionx/tracking.h)
// the way Tracking::Track calls TrackWithPnP (core/frontend/tracking.cpp:332-455), on a scene written
// by tests/test_gpu_track_adapter.py as raw files, and writes the results back.
//
//   track_driver pnp <dir>
//     reads  kf_uv.bin (f64 x2), lm_id.bin (u64), flags.bin (u8), lm_pos.bin (f64 x3), lm_bad.bin (u8),
//            desc_kf.bin / desc_curr.bin (u8 x32), curr_xy.bin (f32 x2), intr.bin (f64 x4),
//            kf_pose.bin (f64 x7)
//     builds the Map the reference would hold (landmarks, the last keyframe with its features),
//     mirrors it into a DeviceMap, runs TrackWithPnP(last_keyframe, current)
//     writes pose.out (f64 x7: current->Pose()), result.out (vx_track_result)
//     prints <returned> <LastInliers> <LastParallax, 17 digits>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "visionx/device_map.h"
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

static int cmd_pnp(const std::string& dir) {
    const auto kf_uv = read_bin<double>(dir + "/kf_uv.bin");
    const auto lm_id = read_bin<uint64_t>(dir + "/lm_id.bin");
    const auto flags = read_bin<uint8_t>(dir + "/flags.bin");
    const auto lm_pos = read_bin<double>(dir + "/lm_pos.bin");
    const auto lm_bad = read_bin<uint8_t>(dir + "/lm_bad.bin");
    const auto desc_kf = read_bin<uint8_t>(dir + "/desc_kf.bin");
    const auto desc_curr = read_bin<uint8_t>(dir + "/desc_curr.bin");
    const auto curr_xy = read_bin<float>(dir + "/curr_xy.bin");
    const auto intr = read_bin<double>(dir + "/intr.bin");
    const auto kf_pose = read_bin<double>(dir + "/kf_pose.bin");
    const size_t n = flags.size(), nc = curr_xy.size() / 2;
    if (kf_uv.size() != 2 * n || lm_id.size() != n || lm_pos.size() != 3 * n || lm_bad.size() != n ||
        desc_kf.size() != 32 * n || desc_curr.size() != 32 * nc || intr.size() != 4 || kf_pose.size() != 7) {
        std::cerr << "inconsistent scene files\n";
        return 2;
    }
    auto cam = std::make_shared<Camera>(intr[0], intr[1], intr[2], intr[3]);
    auto map = std::make_shared<Map>();
    auto kf = std::make_shared<Frame>(7, 0.0, cam, ImageU8());
    SE3d T;
    T.qx = kf_pose[0]; T.qy = kf_pose[1]; T.qz = kf_pose[2]; T.qw = kf_pose[3];
    T.tx = kf_pose[4]; T.ty = kf_pose[5]; T.tz = kf_pose[6];
    kf->SetPose(T);
    kf->Features().resize(n);
    for (size_t i = 0; i < n; ++i) {
        Feature& f = kf->Features()[i];
        f.position = Vec2d(kf_uv[2 * i], kf_uv[2 * i + 1]);
        f.landmark_id_ = lm_id[i];
        f.has_landmark = (flags[i] & 1) != 0;
        f.is_outlier = (flags[i] & 2) != 0;
        if (lm_bad[i] == 2) continue;  // a landmark the map never held
        auto lm = std::make_shared<Landmark>(lm_id[i], Vec3d(lm_pos[3 * i], lm_pos[3 * i + 1], lm_pos[3 * i + 2]));
        lm->SetBad(lm_bad[i] == 1);
        lm->AddObservation(kf->Id(), i);
        map->InsertLandmark(lm);
    }
    kf->Descriptors().rows = (int)n;
    kf->Descriptors().data = desc_kf;
    map->InsertKeyFrame(kf);
    auto curr = std::make_shared<Frame>(8, 0.1, cam, ImageU8());
    curr->Features().resize(nc);
    for (size_t i = 0; i < nc; ++i) curr->Features()[i].position = Vec2d(curr_xy[2 * i], curr_xy[2 * i + 1]);
    curr->Descriptors().rows = (int)nc;
    curr->Descriptors().data = desc_curr;

    auto dmap = std::make_shared<DeviceMap>();
    dmap->Mirror(*map);
    PnPTracker tracker(dmap);
    const bool ok = tracker.TrackWithPnP(kf, curr);
    const SE3d P = curr->Pose();
    const double pose[7] = {P.qx, P.qy, P.qz, P.qw, P.tx, P.ty, P.tz};
    write_bin(dir + "/pose.out", pose, 7);
    write_bin(dir + "/result.out", &tracker.LastResult(), 1);
    std::printf("%d %d %.17g\n", ok ? 1 : 0, tracker.LastInliers(), tracker.LastParallax());
    return 0;
}

int main(int argc, char** argv) {
    try {
        const std::string cmd = argc > 1 ? argv[1] : "";
        if (cmd == "pnp" && argc >= 3) return cmd_pnp(argv[2]);
        std::cerr << "usage: track_driver pnp <dir>\n";
        return 2;
    } catch (const std::exception& e) {
        std::cerr << "error: " << e.what() << "\n";
        return 1;
    }
}
