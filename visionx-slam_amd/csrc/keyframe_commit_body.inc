// keyframe_commit_body.inc — the commit workgroup of CreateKeyFrame on the resident map (kBlock threads),
// included by k_kf_commit (keyframe.hip) and k_rig_kf_commit (keyframe_rig.hip).  Expects in scope:
//   a       const KfArgs&: the camera's argument record
//   b       its base (OwnBase / RigBase, keyframe_bodies.hpp)
//   s_cnt   __shared__ int[kWaves]
//   KF_REJECTED(err)   whether the call is refused, given this camera's own error word
    const int tid = threadIdx.x;
    const int nf = clampi(*a.n_feat, a.cap_feat);
    const int nm = a.has_last ? clampi(*a.n_matches, a.cap_matches) : 0;
    const int err = *a.err;
    if (KF_REJECTED(err)) {  // validate-then-commit: a rejected call writes the header only
        if (tid == 0) {
            vx_keyframe_result h{};
            h.n_feat = nf;
            h.n_matches = nm;
            h.first_landmark_id = h.next_landmark_id = b.first_id();
            h.error_bits = err;
            *a.hdr = h;
        }
        return;
    }
    // 1: CreateLandmarksFromDepth's landmarks, feature order
    int nd = 0;
    for (int base = 0; base < nf; base += kBlock) {
        const int i = base + tid;
        const bool made = depth_made(a, i, nf);
        int total;
        const int r = block_rank(made, s_cnt, &total);
        if (made) {
            const int j = nd + r;
            put_landmark(a, b, j, 0, i, -1, a.dpw + 3 * (int64_t)i);
            put_obs(a, b, j, (int)(b.n_lm0() + j), a.kf_id, (uint64_t)i);
        }
        nd += total;
    }
    // 2: TriangulateWithLastKeyFrame's, match order; a train feature's first passing match wins
    int nt = 0;
    for (int base = 0; base < nm; base += kBlock) {
        const int k = base + tid;
        vx_match mt{};
        const bool made = tri_made(a, k, nm, mt);
        int total;
        const int r = block_rank(made, s_cnt, &total);
        if (made) {
            const int j = nd + nt + r;
            const int64_t o = (int64_t)nd + 2 * (int64_t)(nt + r);
            const uint64_t id = b.first_id() + (uint64_t)j;
            put_landmark(a, b, j, 1, mt.train_idx, mt.query_idx, a.tpw + 3 * (int64_t)k);
            put_obs(a, b, o, (int)(b.n_lm0() + j), a.last_kf_id, (uint64_t)mt.query_idx);  // (tracking.cpp:916)
            put_obs(a, b, o + 1, (int)(b.n_lm0() + j), a.kf_id, (uint64_t)mt.train_idx);   // (:917)
            a.feat_lm[a.f0_last + mt.query_idx] = id;
            a.feat_fl[a.f0_last + mt.query_idx] = 1;
        }
        nt += total;
    }
    if (tid == 0) {  // Map::InsertKeyFrame's rows and the header
        for (int j = 0; j < 7; ++j) a.kf_pose[7 * (int64_t)a.k_new + j] = a.pose[j];
        for (int j = 0; j < 4; ++j) a.kf_intr[4 * (int64_t)a.k_new + j] = a.intr[j];
        vx_keyframe_result h{};
        h.n_feat = nf;
        h.n_depth = nd;
        h.n_triangulated = nt;
        h.n_matches = nm;
        h.first_landmark_id = b.first_id();
        h.next_landmark_id = b.first_id() + (uint64_t)(nd + nt);
        *a.hdr = h;
    }
