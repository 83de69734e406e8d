// track_epairs_body.inc — k_track_epairs' stages 1-6 (track_ess.hip) as program text, included into the
// body of k_track_epairs and of k_rig_epairs (track_rig.hip), as track_pairs_body.inc.  The including
// kernel is ONE workgroup of trk::kBlock threads per problem and provides `a` (a trk::EPairArgs).
    __shared__ int s_cnt[trk::kWaves];
    __shared__ float s_min[trk::kWaves];
    __shared__ double s_sum[trk::kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(max(*a.n_matches, 0), a.cap_matches);
    const int n_last = *a.n_last, n_curr = *a.n_curr;

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
        float lx = 0.f, ly = 0.f, cx = 0.f, cy = 0.f;
        if (j < n_good) {
            mi = a.good[j];
            const vx_match m = a.matches[mi];
            if (m.query_idx < 0 || m.query_idx >= n_last || m.train_idx < 0 || m.train_idx >= n_curr) {
                bad_index = true;
            } else {
                const float* pl = reinterpret_cast<const float*>(a.last_xy + (int64_t)m.query_idx * a.last_stride);
                const float* pc = reinterpret_cast<const float*>(a.curr_xy + (int64_t)m.train_idx * a.curr_stride);
                lx = pl[0];
                ly = pl[1];
                cx = pc[0];
                cy = pc[1];
                pair = true;
                if (enough) {  // ComputeParallax (:548-560): (p1 - p2).norm() in double
                    const double dx = (double)lx - (double)cx;
                    const double dy = (double)ly - (double)cy;
                    part += sqrt(dx * dx + dy * dy);
                }
            }
        }
        int total;
        const int r = trk::block_rank(pair, s_cnt, &total);
        if (pair) {
            const int k = n_pairs + r;
            a.p1[2 * k] = lx;
            a.p1[2 * k + 1] = ly;
            a.p2[2 * k] = cx;
            a.p2[2 * k + 1] = cy;
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

    // 6: result counts and the essential problem record
    if (tid == 0) {
        double sum = s_sum[0];
        n_bad = s_cnt[0];
#pragma unroll
        for (int w = 1; w < trk::kWaves; ++w) {
            sum += s_sum[w];
            n_bad += s_cnt[w];
        }
        vx_track_essential_result* r = a.res;
        r->status = 0;
        r->n_matches = n;
        r->n_good_matches = n_good;
        r->n_pairs = n_pairs;
        r->n_bad_index = n_bad;
        r->min_distance = mn;
        r->parallax = enough && n_good > 0 ? sum / (double)n_good : 0.0;  // cnt > 0 ? sum / cnt : 0 (:559)
        a.offsets[0] = 0;
        a.offsets[1] = enough ? n_pairs : 0;  // (:306)
        for (int k = 0; k < 4; ++k) a.intr_out[k] = a.intr[k];
        *a.opt_out = a.ess;
    }
