// LocalMapping's and LoopClosing's Fuse loops on CDNA4 (included into orbfe_engine.hip last: it uses the
// matcher's per-thread arena and batch completion, the resident orbfe_keyframe with its search grid and
// the bodies of k_kf_geom / k_kf_search).
//  * orbfe_fuse_batch: the search half of Fuse(pKF[c], vpMapPoints, th) (ORBmatcher.cc:1148-1337) or of
//    Fuse(pKF[c], Scw[c], vpPoints, th, vpReplacePoint) (:1339-1455) for every target keyframe c of
//    LocalMapping::SearchInNeighbors (LocalMapping.cc:714-830) or LoopClosing::SearchAndFuse
//    (LoopClosing.cc:3446-3530) in one launch over resident keyframes and one shared point set.
#pragma once

// One (keyframe, pose) job of the batch: the projection of its pose and camera (KfGeom, as the single
// call builds it), the device pointers of the handle's three blocks, and where its skip bytes start.
struct FuseJobDev {
    KfGeom g;
    const uint8_t* grid;   // [KfGridHdr | mvInvLevelSigma2 | cstart | cidx]; nullptr: the row is -1
    const float4* keys;    // the geometry block: n_kp keypoint records, then mvScaleFactors
    const uint32_t* desc;  // the pack's descriptors
    long long o_skip;      // this job's first byte in the skip slab; -1: no point is skipped
    int n_kp, cell_off;    // cell_off = MT_NCELL: a two-camera keyframe's right cells (bRight)
    int o_inv, o_cs, o_ci; // byte offsets inside the grid block
    int gstride_c, gstride_i;
};
struct FuseBatchIn {
    const FuseJobDev* jobs;
    const orbfe_map_point_3d* pts;   // [n], shared by every job
    const uint8_t* skip;
    int n, nchunk;                   // nchunk = workgroups per job
    float th;
    int reproj, init_best;           // sim3 = 0: the chi-square gates, 256; sim3 = 1: none, INT_MAX
    int* idx_out;                    // [n_jobs][n] in the mapped pinned block
    int* dist_out;                   // [n_jobs][n]
    int* cnt_out;                    // [n_jobs][nchunk]: fused points of each workgroup
    BatchEnd end;
};

// Workgroup b = points [256 * (b % nchunk), + 256) of job b / nchunk; one lane per point. The lane runs
// k_kf_geom's body (kf_project) and, when the point survives, k_kf_search's (kf_search_point) on the
// job's level grid with the projection record in registers; the keyframe's records, cells and
// descriptors are read through L2 (every workgroup of a job, and every job of a keyframe, reads the same
// lines). Each lane stores its own two slots, so there is no fill pass. The job record is the same for
// the whole workgroup, so every branch on it and both barriers are workgroup-uniform.
__global__ __launch_bounds__(MT_NT) void k_fuse_batch(FuseBatchIn in) {
    __shared__ int s_n;
    const int tid = threadIdx.x;
    const int c = (int)blockIdx.x / in.nchunk;
    const int q = ((int)blockIdx.x - c * in.nchunk) * MT_NT + tid;
    const FuseJobDev& jd = in.jobs[c];
    if (tid == 0) s_n = 0;
    SYNC();
    int result = -1, bestIdx = -1, bestDist = in.init_best;
    if (q < in.n && jd.grid) {
        const orbfe_map_point_3d mp = in.pts[q];
        const bool skipped = jd.o_skip >= 0 && in.skip[jd.o_skip + q] != 0;
        const KfProj p = kf_project(jd.g, mp, skipped);
        if (p.level >= 0) {
            const KfGridHdr h = *(const KfGridHdr*)jd.grid;
            const KfGridFrame fr{h.minx, h.miny, h.invw, h.invh, KfGridKeys{jd.keys}, jd.desc};
            const float* scale = (const float*)(jd.keys + jd.n_kp);
            const float radius = in.th * scale[p.level];
            // level grid p.level is grid p.level + 1 of the block (grid 0, the full one, is not built)
            const int* cs = (const int*)(jd.grid + jd.o_cs) + (size_t)(p.level + 1) * jd.gstride_c + jd.cell_off;
            const int* ci = (const int*)(jd.grid + jd.o_ci) + (size_t)(p.level + 1) * jd.gstride_i;
            kf_search_point(fr, cs, ci, p, mp, radius, in.reproj, (const float*)(jd.grid + jd.o_inv), (const int*)nullptr,
                            (const int*)nullptr, q, bestIdx, bestDist);
            if (bestIdx >= 0 && (float)bestDist <= (float)MT_TH_LOW) result = bestIdx;
        }
    }
    if (q < in.n) {
        in.idx_out[(size_t)c * in.n + q] = result;
        in.dist_out[(size_t)c * in.n + q] = bestIdx >= 0 ? bestDist : -1;
    }
    // nfused: one ballot and one atomic per wave
    const unsigned long long m = __ballot(result >= 0);
    if ((tid & 63) == 0 && m) atomicAdd(&s_n, (int)__popcll(m));
    __builtin_amdgcn_s_waitcnt(0);
    SYNC();
    if (tid == 0) {
        ((volatile int*)in.cnt_out)[blockIdx.x] = s_n;
        mt_batch_end(in.end);   // this workgroup's slots and count are released before it is counted
    }
}

namespace {
// orbfe_matcher_last_fuse_batch: searched jobs, empty rows, workgroups (host record)
thread_local int t_fuse_batch[3] = {0, 0, 0};
}  // namespace

extern "C" {

int orbfe_fuse_batch(const orbfe_fuse_job* jobs, int32_t n_jobs, const orbfe_map_point_3d* pts, int32_t n, float th,
                     int32_t sim3, int32_t* best_idx, int32_t* best_dist, int32_t* nfused) {
    t_fuse_batch[0] = t_fuse_batch[1] = t_fuse_batch[2] = 0;
    // every refusal below comes before any device work and before any write to the outputs
    if (n_jobs < 0 || n < 0) return ORBFE_E_ARG;
    if (n_jobs == 0) return ORBFE_OK;
    if (!jobs || !nfused || (n > 0 && (!pts || !best_idx || !best_dist))) return ORBFE_E_ARG;
    int nlive = 0;
    for (int c = 0; c < n_jobs; c++) {
        const orbfe_fuse_job& j = jobs[c];
        const orbfe_keyframe* k = j.kf;
        if (!k) continue;   // isBad(): the other fields are not read
        if (!k->has_grid || !pose_ok(&j.cam.Tcw) || !cam_model_ok(&j.model) || (j.bRight && (sim3 || !k->two)))
            return ORBFE_E_ARG;
        if (k->n > 0) nlive++;
    }
    const size_t rows = (size_t)n_jobs * (size_t)n;
    const int nchunk = (n + MT_NT - 1) / MT_NT;
    if (2 * rows + (size_t)n_jobs * (size_t)std::max(nchunk, 1) > ((size_t)1 << 28)) return ORBFE_E_CAPACITY;
    const bool live = nlive > 0 && n > 0;   // else every row is empty and the call needs no device
    if (live) {   // a handle belongs to its create's device
        int dev = 0;
        HIPCHK(hipGetDevice(&dev));
        for (int c = 0; c < n_jobs; c++)
            if (jobs[c].kf && jobs[c].kf->device != dev) return ORBFE_E_ARG;
    }
    if (!live) {
        for (int c = 0; c < n_jobs; c++) nfused[c] = 0;
        for (size_t i = 0; i < rows; i++) best_idx[i] = best_dist[i] = -1;
        t_fuse_batch[1] = n_jobs;
        return ORBFE_OK;
    }
    // one upload for the call: the points, the skip bytes of every job that has them, the zeroed
    // completion counter and the job records
    Plan p;
    const size_t o_pts = p.upload(pts, (size_t)n * sizeof(orbfe_map_point_3d));
    std::vector<FuseJobDev> jd(n_jobs);
    std::vector<uint8_t> slab;
    for (int c = 0; c < n_jobs; c++) {
        const orbfe_fuse_job& j = jobs[c];
        const orbfe_keyframe* k = j.kf;
        FuseJobDev& d = jd[c];
        memset(&d, 0, sizeof(d));
        d.o_skip = -1;
        if (!k || k->n == 0) continue;
        // the single call's KfGeom (kf_geom, BE_PRJ_MODEL) from the handle's bounds and the job's camera
        KfGeom& g = d.g;
        g.T = j.cam.Tcw;
        memcpy(g.Ow, j.cam.Ow, sizeof(g.Ow));
        g.logsf = j.cam.log_scale_factor;
        g.mbf = k->mbf;
        g.minx = k->minx; g.maxx = k->maxx; g.miny = k->miny; g.maxy = k->maxy;
        g.nlevels = k->nlevels;
        g.proj = BE_PRJ_MODEL;
        g.view = 1;
        g.skip_flags = ORBFE_MP_BAD | ORBFE_MP_SKIP;
        g.cam_type = j.model.type;
        g.fx = j.model.params[0]; g.fy = j.model.params[1]; g.cx = j.model.params[2]; g.cy = j.model.params[3];
        for (int t = 0; t < 4; t++) g.kb[t] = j.model.type == ORBFE_CAM_KANNALA_BRANDT8 ? j.model.params[4 + t] : 0.f;
        d.grid = k->grid;
        d.keys = (const float4*)k->geom;
        d.desc = (const uint32_t*)(k->pack + k->o_desc);
        d.n_kp = k->n;
        d.cell_off = j.bRight ? MT_NCELL : 0;
        d.o_inv = k->g_inv;
        d.o_cs = k->g_cs;
        d.o_ci = k->g_ci;
        d.gstride_c = k->gstride_c;
        d.gstride_i = k->gstride_i;
        if (j.skip) {
            d.o_skip = (long long)slab.size();
            slab.insert(slab.end(), j.skip, j.skip + n);
        }
    }
    const size_t o_skip = slab.empty() ? 0 : p.upload(slab.data(), slab.size());
    const size_t o_done = ms_plan_done(p);
    const size_t o_jobs = p.upload(jd.data(), (size_t)n_jobs * sizeof(FuseJobDev));
    const size_t nwg = (size_t)n_jobs * nchunk;
    FuseBatchIn in;
    memset(&in, 0, sizeof(in));
    MSCHK(ms_batch_prepare(p, 2 * rows + nwg, o_done, in.end));   // the two row blocks, then the counts
    MatchScratch& m = t_ms;
    hipStream_t s = m.stream;
    MsTimer timer(s);
    in.jobs = ms_ptr<const FuseJobDev>(o_jobs);
    in.pts = ms_ptr<const orbfe_map_point_3d>(o_pts);
    in.skip = ms_ptr<const uint8_t>(o_skip);
    in.n = n;
    in.nchunk = nchunk;
    in.th = th;
    in.reproj = sim3 ? 0 : 1;
    in.init_best = sim3 ? INT_MAX : 256;
    in.idx_out = m.ho_dev;
    in.dist_out = m.ho_dev + rows;
    in.cnt_out = m.ho_dev + 2 * rows;
    hipLaunchKernelGGL(k_fuse_batch, dim3((unsigned)nwg), dim3(MT_NT), 0, s, in);
    HIPCHK(hipGetLastError());
    timer.end();
    MSCHK(ms_wait_seq(s, in.end.seq));
    // complete: the sequence word comes after every workgroup's release
    memcpy(best_idx, m.ho, rows * 4);
    memcpy(best_dist, m.ho + rows, rows * 4);
    for (int c = 0; c < n_jobs; c++) {
        int nf = 0;
        for (int b = 0; b < nchunk; b++) nf += m.ho[2 * rows + (size_t)c * nchunk + b];
        nfused[c] = nf;
    }
    t_fuse_batch[0] = nlive;
    t_fuse_batch[1] = n_jobs - nlive;
    t_fuse_batch[2] = (int)nwg;
    return ORBFE_OK;
}

int orbfe_matcher_last_fuse_batch(int32_t* out) {
    if (!out) return ORBFE_E_ARG;
    for (int i = 0; i < 3; i++) out[i] = t_fuse_batch[i];
    return ORBFE_OK;
}

}  // extern "C"
