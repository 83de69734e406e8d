// track_status_check — the status rules of csrc/track_common.hpp (the ONE statement vx_track_pnp_fetch,
// vx_track_essential_fetch, k_track_gate and k_track_final share) evaluated on the host, for
// tests/test_track_frame_cpu.py.  One case per line on stdin:
//   pnp <n_good> <n_pairs> <ok> <n_inliers> <pose: finite|nan|inf> <min_matches> <min_inliers>
//   ess <n_good> <ok> <n_inliers> <min_matches> <min_inliers>
// One status per line on stdout.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "track_common.hpp"

int main() {
    char kind[8], pose[8];
    while (std::scanf("%7s", kind) == 1) {
        if (!std::strcmp(kind, "pnp")) {
            vx_track_result r{};
            int mm, mi;
            if (std::scanf("%d %d %d %d %7s %d %d", &r.n_good_matches, &r.n_pairs, &r.pnp.ok, &r.pnp.n_inliers, pose, &mm, &mi) != 7) return 2;
            r.pnp.pose[3] = 1.0;
            if (!std::strcmp(pose, "nan")) r.pnp.pose[5] = std::numeric_limits<double>::quiet_NaN();
            if (!std::strcmp(pose, "inf")) r.pnp.pose[0] = -std::numeric_limits<double>::infinity();
            std::printf("%d\n", vx::trk::pnp_status(r, mm, mi));
        } else if (!std::strcmp(kind, "ess")) {
            vx_track_essential_result r{};
            int mm, mi;
            if (std::scanf("%d %d %d %d %d", &r.n_good_matches, &r.ess.ok, &r.ess.n_inliers, &mm, &mi) != 5) return 2;
            std::printf("%d\n", vx::trk::ess_status(r, mm, mi));
        } else {
            return 2;
        }
    }
    return 0;
}
