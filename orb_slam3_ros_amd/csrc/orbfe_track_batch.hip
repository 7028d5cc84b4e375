// TrackWithMotionModel's SearchByProjection(CurrentFrame, LastFrame, th, bMono) (ORBmatcher.cc:1676-1887)
// for the frames of a batch extraction in ONE launch, read where orbfe_extract_batch and
// orbfe_stereo_match_batch left them (included into orbfe_engine.hip's translation unit after
// orbfe_matcher.hip, whose one-workgroup search and per-thread arena it uses).
//
// Workgroup f = frame f = image base + f * step of the slabs: its keypoint count is read on the device,
// its FrameDev is built from the slab pointers, its queries are made in registers from the job's
// last-frame points (k_last_proj's projection and blk_load<1>'s gates, in that order and arithmetic), and
// blk_search<1> does the rest. Frames are independent: each has its own pose, points and empty
// mvpMapPoints (Tracking fills them with NULL before the search).
#pragma once

// Frame f's job on the device: where the call's upload put its points (TrkIn::arena), the pose and the
// search parameters. nq == 0: the frame is skipped.
struct TrkJob {
    size_t o_pts;
    int nq;
    float th;
    int fwd, bwd;
    orbfe_pose T;
};
// Point p as a query: k_last_proj (x3Dc = Tcw * x3Dw, invzc in double, project) followed by blk_load<1>
// (valid and octave, invzc < 0, the inclusive image bounds, radius and level window), without the
// record in between.
__device__ __forceinline__ BlkQuery trk_query(const FrameDev& fr, const TrkJob& jb, const CamModelDev& cam,
                                              const orbfe_last_point& p) {
    BlkQuery Q;
    Q.x = Q.y = Q.R = Q.xr = 0.f;
    Q.olo = 0;
    Q.ohi = -1;
    Q.obs = p.observations;
    Q.ok = p.valid != 0 && p.octave >= 0 && p.octave < fr.nlevels;
    if (!Q.ok) return Q;
    const float pos[3] = {p.pos[0], p.pos[1], p.pos[2]};
    float c[3];
    be_pose_apply(jb.T, pos, c);
    const float invzc = (float)(1.0 / (double)c[2]);
    if (invzc < 0) {   // ORBmatcher.cc:1718
        Q.ok = false;
        return Q;
    }
    const float2 uv = mt_cam_project(cam, c[0], c[1], c[2]);
    if (uv.x < fr.minx || uv.x > fr.maxx) Q.ok = false;
    else if (uv.y < fr.miny || uv.y > fr.maxy) Q.ok = false;
    if (!Q.ok) return Q;
    const int oct = p.octave;
    Q.R = jb.th * fr.scale[oct];
    Q.x = uv.x;
    Q.y = uv.y;
    Q.xr = uv.x - fr.mbf * invzc;   // ur of :1752
    int minL, maxL;   // GetFeaturesInArea's level filter (Frame.cc:689,704-711), as blk_load<1>
    if (jb.fwd) { minL = oct; maxL = -1; }
    else if (jb.bwd) { minL = 0; maxL = oct; }
    else { minL = oct - 1; maxL = oct + 1; }
    const bool chk = (minL > 0) || (maxL >= 0);
    Q.olo = chk ? max(minL, 0) : 0;
    Q.ohi = (chk && maxL >= 0) ? min(maxL, fr.nlevels - 1) : fr.nlevels - 1;
    memcpy(Q.qd, p.desc, 32);
    return Q;
}
// sl: the extractor's batch outputs. rows: [nframes][cap] slots in HBM (the search's mvp_in and mvp_out:
// filled with -1 here, so every slot is free); mvp_out: the same rows in mapped pinned memory, each slot
// stored once, after the search. counts_out: [nframes][3] = {assigned (ORBFE_E_CAPACITY: a frame of more
// keypoints than the workgroup holds), dropped, N}. end: the call's completion (mt_batch_end).
struct TrkIn {
    SlabView sl;
    const TrkJob* jobs;
    const uint8_t* arena;
    int32_t* rows;
    int32_t* mvp_out;
    int* counts_out;
    BatchEnd end;
    int checkOri;
    CamModelDev cam;
};
__global__ __launch_bounds__(MT_BLK_NT) void k_sbp_track_batch(FrameDev fr0, BlkGeom gm, TrkIn in) {
    extern __shared__ __attribute__((aligned(16))) uint8_t mt_sm[];
    const int tid = threadIdx.x, f = blockIdx.x;
    const int cap = in.sl.cap, img = in.sl.image(f);
    const int N = in.sl.count(img);   // (uniform over the workgroup)
    const TrkJob& jb = in.jobs[f];
    const int nq = jb.nq;
    int32_t* row = in.rows + (size_t)f * cap;
    for (int k = tid; k < cap; k += MT_BLK_NT) row[k] = -1;
    const bool over = in.sl.over(N);
    const int* cnt = nullptr;
    if (nq > 0 && N > 0 && !over) {
        // the -1 fill is the staging's slot state: complete before any thread reads it
        __builtin_amdgcn_s_waitcnt(0);
        SYNC();
        const FrameDev fr = in.sl.frame(fr0, f, img, N);
        const orbfe_last_point* pts = (const orbfe_last_point*)(in.arena + jb.o_pts);
        int qid[MT_BLK_QPT];
        float qang[MT_BLK_QPT];
        BlkQuery QS[MT_BLK_QPT];
#pragma unroll
        for (int i = 0; i < MT_BLK_QPT; i++) {
            qid[i] = -1;
            qang[i] = 0.f;
            QS[i].ok = false;
            QS[i].obs = 0;
            const int q = tid + i * MT_BLK_NT;
            if (q >= nq) continue;
            qid[i] = pts[q].id;
            if (in.checkOri) qang[i] = pts[q].angle;
            QS[i] = trk_query(fr, jb, in.cam, pts[q]);
        }
        const BlkIO io{row, nullptr, row, 0, 0, 0, in.checkOri, nullptr, nullptr, 0, nullptr, nullptr};
        blk_search<1>(fr, gm, QS, qid, qang, nq, 0.f, MT_TH_HIGH, 1, io, mt_sm,
                      [&](int q) { return trk_query(fr, jb, in.cam, pts[q]); }, cnt);
    } else {
        __builtin_amdgcn_s_waitcnt(0);
        SYNC();
    }
    // the row to the host, each slot once (blk_search ended with its stores complete and a barrier)
    int32_t* out = in.mvp_out + (size_t)f * cap;
    for (int k = tid; k < cap; k += MT_BLK_NT) out[k] = row[k];
    __builtin_amdgcn_s_waitcnt(0);
    SYNC();
    if (tid == 0) {
        volatile int* co = in.counts_out + 3 * f;
        co[0] = over && nq > 0 ? ORBFE_E_CAPACITY : cnt ? cnt[0] : 0;
        co[1] = cnt ? cnt[1] : 0;
        co[2] = N;
        mt_batch_end(in.end);   // this workgroup's row and counts are released before it is counted
    }
}

namespace {
// orbfe_matcher_last_track_batch: frames searched, skipped, over capacity (host record)
thread_local int t_track_batch[3] = {0, 0, 0};
}  // namespace

extern "C" {

int orbfe_search_by_projection_lastframe_slabs(const orbfe_keypoint* d_kps, const uint8_t* d_desc,
                                               const int32_t* d_counts, int32_t cap, int32_t base, int32_t step,
                                               const float* d_uright, const orbfe_frame* geom,
                                               const orbfe_camera_model* cam, const orbfe_track_job* jobs,
                                               int32_t nframes, int32_t checkOri, int32_t* mvp_out, int32_t* nmatches,
                                               int32_t* n_keys, void* stream) {
    t_track_batch[0] = t_track_batch[1] = t_track_batch[2] = 0;
    // every refusal below comes before any device work and before any write to the outputs
    if (nframes < 0) return ORBFE_E_ARG;
    if (nframes == 0) return ORBFE_OK;
    if (!slabs_ok(d_kps, d_desc, d_counts, cap, base, step) || !geom || !cam || !jobs || !mvp_out || !nmatches ||
        !n_keys)
        return ORBFE_E_ARG;
    if (geom->two_cams || geom->nlevels <= 0 || !geom->scale_factors) return ORBFE_E_ARG;
    if (!cam_model_ok(cam)) return ORBFE_E_ARG;
    for (int f = 0; f < nframes; f++) {
        const orbfe_track_job& j = jobs[f];
        if (j.n_pts < 0 || (j.n_pts > 0 && !j.pts) || j.Tcw.kind != ORBFE_SE3) return ORBFE_E_ARG;
    }
    // nLastOctave addresses mvScaleFactors (as the single call checks)
    for (int f = 0; f < nframes; f++)
        for (int k = 0; k < jobs[f].n_pts; k++) {
            const orbfe_last_point& p = jobs[f].pts[k];
            if (p.valid && (p.octave < 0 || p.octave >= geom->nlevels)) return ORBFE_E_ARG;
        }
    for (int f = 0; f < nframes; f++)
        if (jobs[f].n_pts > MT_BLOCK_MAXQ) return ORBFE_E_CAPACITY;
    // the workgroup's LDS frame is sized for the largest frame it takes: min(cap, 2048) keypoints
    const int nmax = std::min<int>(cap, MT_BAND_MAXN);
    orbfe_frame G = *geom;
    G.n = nmax;
    BlkGeom gm;
    if (!blk_geom(&G, gm)) return ORBFE_E_CAPACITY;
    if (!slab_rows_ok(nframes, cap)) return ORBFE_E_CAPACITY;
    // one upload for the call: the scale factors, every job's points, the job table and the zeroed
    // completion counter
    Plan p;
    const size_t o_scale = p.upload(geom->scale_factors, (size_t)geom->nlevels * 4);
    std::vector<TrkJob> tj(nframes);
    for (int f = 0; f < nframes; f++) {
        TrkJob& t = tj[f];
        memset(&t, 0, sizeof(t));
        t.nq = jobs[f].n_pts;
        t.th = jobs[f].th;
        t.fwd = jobs[f].bForward ? 1 : 0;
        t.bwd = jobs[f].bBackward ? 1 : 0;
        t.T = jobs[f].Tcw;
        if (t.nq > 0) t.o_pts = p.upload(jobs[f].pts, (size_t)t.nq * sizeof(orbfe_last_point));
    }
    const size_t o_jobs = p.upload(tj.data(), (size_t)nframes * sizeof(TrkJob));
    const size_t o_done = ms_plan_done(p);
    const size_t nrow = (size_t)nframes * cap, nout = nrow + 3 * (size_t)nframes;   // the rows, then the counts
    const size_t o_rows = p.scratch(nrow * 4);
    TrkIn in;
    memset(&in, 0, sizeof(in));
    MSCHK(ms_batch_prepare(p, nout, o_done, in.end));
    MatchScratch& m = t_ms;
    hipStream_t s = m.stream;
    MSCHK(ms_after_caller(stream));
    MsTimer timer(s);
    const FrameDev fr = ms_geom_frame(geom, o_scale);
    in.sl = SlabView{(const OrbKeyPoint*)d_kps, d_desc, d_counts, d_uright, cap, base, step, nmax};
    in.jobs = ms_ptr<const TrkJob>(o_jobs);
    in.arena = ms_ptr<const uint8_t>(0);
    in.rows = ms_ptr<int32_t>(o_rows);
    in.mvp_out = m.ho_dev;
    in.counts_out = m.ho_dev + nrow;
    in.checkOri = checkOri ? 1 : 0;
    in.cam = make_cam_model(cam);
    // one workgroup per frame, each with k_sbp_block's LDS frame for nmax keypoints
    hipLaunchKernelGGL(k_sbp_track_batch, dim3(nframes), dim3(MT_BLK_NT), blk_lds(nmax, geom->nlevels, gm), s, fr, gm,
                       in);
    HIPCHK(hipGetLastError());
    timer.end();
    MSCHK(ms_wait_seq(s, in.end.seq));
    memcpy(mvp_out, m.ho, nrow * 4);   // complete: the sequence word comes after every workgroup's release
    for (int f = 0; f < nframes; f++) {
        const int* co = m.ho + nrow + 3 * (size_t)f;
        const int N = co[2];
        nmatches[f] = co[0] < 0 ? co[0] : co[0] - co[1];
        n_keys[f] = N;
        if (jobs[f].n_pts == 0 || N == 0) t_track_batch[1]++;
        else if (co[0] < 0) t_track_batch[2]++;
        else t_track_batch[0]++;
    }
    return ORBFE_OK;
}

int orbfe_matcher_last_track_batch(int32_t* out) {
    if (!out) return ORBFE_E_ARG;
    for (int i = 0; i < 3; i++) out[i] = t_track_batch[i];
    return ORBFE_OK;
}

}  // extern "C"
