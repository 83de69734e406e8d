// track_pairs_body.inc — k_track_pairs' stages 1-6 (track.hip) as program text, included into the body of
// k_track_pairs and of k_rig_pairs (track_rig.hip): ONE statement of the rules, and the single-camera
// kernel compiles to exactly what it was.  The including kernel is ONE workgroup of trk::kBlock threads
// per problem and provides `a` (a trk::TrackArgs, value or reference).  256 B of LDS.
    __shared__ int s_cnt[trk::kWaves];
    __shared__ float s_min[trk::kWaves];
    __shared__ double s_sum[trk::kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(max(*a.n_matches, 0), a.cap_matches);
    const int n_curr = *a.n_curr;

    // 1-3: min distance, threshold, the kept matches in match order (track_common.hpp)
    float mn;
    const int n_good = trk::filter_matches(a.matches, n, a.good, s_cnt, s_min, &mn);

    // 4 + 5: pairs in kept-match order, parallax partials
    const bool enough = n_good >= a.min_matches;
    int n_pairs = 0, n_bad = 0;
    double part = 0.0;
    for (int base = 0; base < n_good; base += trk::kBlock) {
        const int j = base + tid;
        bool pair = false, bad_index = false;
        int mi = 0;
        float ox = 0.f, oy = 0.f, oz = 0.f, ix = 0.f, iy = 0.f;
        if (j < n_good) {
            mi = a.good[j];
            const vx_match m = a.matches[mi];
            if (m.query_idx < 0 || m.query_idx >= a.nf || m.train_idx < 0 || m.train_idx >= n_curr) {
                bad_index = true;
            } else {
                const int64_t f = a.f0 + m.query_idx;
                trk::curr_pos(a, m.train_idx, &ix, &iy);
                if (enough) {  // ComputeParallax (:548-560): (p1 - p2).norm() in double
                    const double dx = a.feat_uv[2 * f] - (double)ix;
                    const double dy = a.feat_uv[2 * f + 1] - (double)iy;
                    part += sqrt(dx * dx + dy * dy);
                }
                const uint8_t fl = a.feat_fl[f];
                if ((fl & 1) && !(fl & 2)) {  // has_landmark && !is_outlier (:375)
                    const int row = ht_get(a.ht_key, a.ht_val, a.ht_mask, a.feat_lm[f]);  // GetLandmark (:378)
                    if (row >= 0 && a.lm_bad[row] == 0) {                                  // !lm, IsBad (:379-384)
                        const double px = a.lm_pos[3 * (int64_t)row], py = a.lm_pos[3 * (int64_t)row + 1],
                                     pz = a.lm_pos[3 * (int64_t)row + 2];
                        const bool nan = px != px || py != py || pz != pz;              // (:388)
                        const bool far = fabs(px) > 1000 || fabs(py) > 1000 || fabs(pz) > 1000;  // (:391)
                        if (!nan && !far) {
                            pair = true;
                            ox = (float)px;  // cv::Point3f (:395)
                            oy = (float)py;
                            oz = (float)pz;
                        }
                    }
                }
            }
        }
        int total;
        const int r = trk::block_rank(pair, s_cnt, &total);
        if (pair) {
            const int k = n_pairs + r;
            a.obj[3 * k] = ox;
            a.obj[3 * k + 1] = oy;
            a.obj[3 * k + 2] = oz;
            a.img[2 * k] = ix;
            a.img[2 * k + 1] = iy;
            a.pair_match[k] = mi;
            a.mask[k] = 0;
        }
        n_pairs += total;
        n_bad += bad_index ? 1 : 0;
    }

    // 5: parallax (and the skipped-index count), fixed order
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        part += __shfl_xor(part, off);
        n_bad += __shfl_xor(n_bad, off);
    }
    if (lane == 0) {
        s_sum[wave] = part;
        s_cnt[wave] = n_bad;
    }
    __syncthreads();

    // 6: result counts and the PnP problem record
    if (tid == 0) {
        double sum = s_sum[0];
        n_bad = s_cnt[0];
#pragma unroll
        for (int w = 1; w < trk::kWaves; ++w) {
            sum += s_sum[w];
            n_bad += s_cnt[w];
        }
        vx_track_result* r = a.res;
        r->status = 0;
        r->n_matches = n;
        r->n_good_matches = n_good;
        r->n_pairs = n_pairs;
        r->n_bad_index = n_bad;
        r->min_distance = mn;
        r->parallax = enough && n_good > 0 ? sum / (double)n_good : 0.0;  // cnt > 0 ? sum / cnt : 0 (:559)
        const bool run = enough && n_pairs >= a.min_inliers;
        a.offsets[0] = 0;
        a.offsets[1] = run ? n_pairs : 0;
        for (int k = 0; k < 4; ++k) a.intr_out[k] = a.intr[k];
        vx_pnp_options o = a.pnp;
        if (o.max_iterations < 0) o.max_iterations = min(100, 2 * n_pairs);  // (:421)
        *a.opt_out = o;
    }
