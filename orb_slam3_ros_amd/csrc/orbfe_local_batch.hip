// TrackLocalMap's SearchLocalPoints (Tracking.cc:3382-3452) for the frames of a batch extraction in ONE
// launch, read where orbfe_extract_batch and orbfe_stereo_match_batch left them (included into
// orbfe_engine.hip's translation unit after orbfe_track_batch.hip; the slab addressing, the completion and
// the host scaffold are orbfe_matcher.hip's SlabView, mt_batch_end and ms_* helpers).
//
// Workgroup f = frame f = image base + f * step of the slabs, in two phases:
//   A  Frame::isInFrustum + MapPoint::PredictScale over the job's points (mt_frustum_single, the code
//      k_frustum runs), 1,024 points per trip; the points in view are compacted IN ARRAY ORDER into at most
//      MT_BLOCK_MAXQ records in the frame's HBM scratch (a wave ballot, the waves' totals through LDS, a
//      running base). A point outside the view is a `continue` of the reference loop, so leaving it out
//      changes no result, and the order of the rest is the order the fixed point depends on.
//   B  blk_search<0> on those records with the frame staged from the slab pointers: k_sbp_block<0>'s search.
// Frames are independent: each has its own pose, points (or a shared upload with its own skip bitset), th
// and slot row.
#pragma once

#define LOC_MAX_POINTS ORBFE_LOCAL_BATCH_MAX_POINTS

// Frame f's job on the device. o_pts / o_skip / o_recs: offsets into the call's arena (LocIn::arena);
// o_skip: one bit per point (this frame's ORBFE_MP_SKIP), ~0 when the job has no skip list; view: the
// first word of the job's in_view bitset in the pinned out block (whole 64-point groups), -1: not wanted.
struct LocJob {
    CamDev cd;
    size_t o_pts, o_skip, o_recs;
    int n_pts, view;
    float th;
};
// rows_in / obs_in: the uploaded mvp_in / mvp_obs [nframes][cap]; rows: the working rows in HBM; mvp_out:
// the same rows in mapped pinned memory, each slot stored once, after the search. counts_out:
// [nframes][4] = {assigned (ORBFE_E_CAPACITY: more keypoints or more points in view than the workgroup
// holds), dropped, N, nToMatch}. sl: the extractor's batch outputs; end: the call's completion
// (mt_batch_end).
struct LocIn {
    SlabView sl;
    const LocJob* jobs;
    uint8_t* arena;
    const int32_t* rows_in;
    const int32_t* obs_in;
    int32_t* rows;
    int32_t* mvp_out;
    int* counts_out;
    int32_t* view_out;
    BatchEnd end;
    int bFar;
    float thFar, nnratio;
};
__global__ __launch_bounds__(MT_BLK_NT) void k_local_batch(FrameDev fr0, BlkGeom gm, LocIn in) {
    extern __shared__ __attribute__((aligned(16))) uint8_t mt_sm[];
    __shared__ int s_wtot[MT_BLK_NT / 64];
    const int tid = threadIdx.x, f = blockIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cap = in.sl.cap, img = in.sl.image(f);
    const int N = in.sl.count(img);   // (uniform over the workgroup)
    const LocJob& jb = in.jobs[f];
    const int np = jb.n_pts;
    // the row starts as mvp_in's (a search leaves the slots it does not assign alone), -1 beyond the frame
    int32_t* row = in.rows + (size_t)f * cap;
    const int32_t* row_in = in.rows_in + (size_t)f * cap;
    const int nheld = min(max(N, 0), cap);
    for (int k = tid; k < cap; k += MT_BLK_NT) row[k] = k < nheld ? row_in[k] : -1;
    // ---- phase A: the points in view, compacted in array order ----
    const orbfe_map_point_3d* pts = (const orbfe_map_point_3d*)(in.arena + jb.o_pts);
    const uint32_t* skip = jb.o_skip != ~(size_t)0 ? (const uint32_t*)(in.arena + jb.o_skip) : nullptr;
    orbfe_map_point* recs = (orbfe_map_point*)(in.arena + jb.o_recs);
    int nview = 0;   // points in view so far (uniform)
    for (int b0 = 0; b0 < np; b0 += MT_BLK_NT) {
        const int i = b0 + tid;
        bool inv = false;
        orbfe_map_point t;
        if (i < np) {
            orbfe_map_point_3d p = pts[i];
            if (skip && ((skip[i >> 5] >> (i & 31)) & 1u)) p.flags |= ORBFE_MP_SKIP;
            mt_track_init(p, t);
            inv = mt_frustum_single(jb.cd, p, t);
        }
        const unsigned long long m = __ballot(inv);
        if (jb.view >= 0 && lane == 0 && b0 + wave * 64 < np) {   // the group's 64 mbTrackInView bits
            in.view_out[jb.view + 2 * ((b0 >> 6) + wave)] = (int)(unsigned)m;
            in.view_out[jb.view + 2 * ((b0 >> 6) + wave) + 1] = (int)(unsigned)(m >> 32);
        }
        if (lane == 0) s_wtot[wave] = (int)__popcll(m);
        SYNC();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < MT_BLK_NT / 64; w++) {
            const int c = s_wtot[w];
            before += w < wave ? c : 0;
            all += c;
        }
        const int slot = nview + before + (int)__popcll(m & ((1ull << lane) - 1ull));
        if (inv && slot < MT_BLOCK_MAXQ) recs[slot] = t;
        nview += all;
        SYNC();   // s_wtot is rewritten by the next trip
    }
    const bool over = in.sl.over(N) || nview > MT_BLOCK_MAXQ;
    const int* cnt = nullptr;
    // the row's fill and the records are complete before any thread reads them
    __builtin_amdgcn_s_waitcnt(0);
    SYNC();
    // ---- phase B: SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints) on the records ----
    if (nview > 0 && N > 0 && !over) {
        const FrameDev fr = in.sl.frame(fr0, f, img, N);
        const float th = jb.th;
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
            if (q >= nview) continue;
            qid[i] = recs[q].id;
            QS[i] = blk_load<0>(fr, recs, q, th, in.bFar, 0, in.thFar);
        }
        const BlkIO io{row, in.obs_in + (size_t)f * cap, row, 0, 0, 0, 0, nullptr, nullptr, 0, nullptr, nullptr};
        blk_search<0>(fr, gm, QS, qid, qang, nview, in.nnratio, 0, 1, io, mt_sm,
                      [&](int q) { return blk_load<0>(fr, recs, q, th, in.bFar, 0, in.thFar); }, cnt);
    }
    // the row to the host, each slot once (blk_search ended with its stores complete and a barrier)
    int32_t* out = in.mvp_out + (size_t)f * cap;
    for (int k = tid; k < cap; k += MT_BLK_NT) out[k] = row[k];
    __builtin_amdgcn_s_waitcnt(0);
    SYNC();
    if (tid == 0) {
        volatile int* co = in.counts_out + 4 * f;
        co[0] = over && np > 0 ? ORBFE_E_CAPACITY : cnt ? cnt[0] : 0;
        co[1] = cnt ? cnt[1] : 0;
        co[2] = N;
        co[3] = nview;
        mt_batch_end(in.end);   // this workgroup's row, view bits and counts are released before it is counted
    }
}

namespace {
// orbfe_matcher_last_local_batch: frames searched, skipped, over capacity (host record)
thread_local int t_local_batch[3] = {0, 0, 0};
// the thread's last call: distinct point arrays uploaded (jobs with one pts pointer and n_pts share one)
thread_local int t_local_uploads = 0;
}  // namespace

extern "C" {

int orbfe_search_local_points_slabs(const orbfe_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_counts,
                                    int32_t cap, int32_t base, int32_t step, const float* d_uright,
                                    const orbfe_frame* geom, const orbfe_camera_model* model,
                                    const orbfe_local_job* jobs, int32_t nframes, const int32_t* mvp_in,
                                    const int32_t* mvp_obs, int32_t bFarPoints, float thFarPoints, float nnratio,
                                    int32_t* mvp_out, int32_t* nmatches, int32_t* n_to_match, int32_t* n_keys,
                                    void* stream) {
    t_local_batch[0] = t_local_batch[1] = t_local_batch[2] = 0;
    t_local_uploads = 0;
    // every refusal below comes before any device work and before any write to the outputs
    if (nframes < 0) return ORBFE_E_ARG;
    if (nframes == 0) return ORBFE_OK;
    if (!slabs_ok(d_kps, d_desc, d_counts, cap, base, step) || !geom || !jobs || !mvp_in || !mvp_obs || !mvp_out ||
        !nmatches || !n_to_match || !n_keys)
        return ORBFE_E_ARG;
    if (geom->two_cams || geom->nlevels <= 0 || !geom->scale_factors) return ORBFE_E_ARG;
    if (model && !cam_model_ok(model)) return ORBFE_E_ARG;
    for (int f = 0; f < nframes; f++) {
        const orbfe_local_job& j = jobs[f];
        if (j.n_pts < 0 || j.n_skip < 0 || (j.n_pts > 0 && !j.pts) || (j.n_skip > 0 && !j.skip)) return ORBFE_E_ARG;
        for (int k = 0; k < j.n_skip; k++)
            if (j.skip[k] < 0 || j.skip[k] >= j.n_pts) return ORBFE_E_ARG;
    }
    for (int f = 0; f < nframes; f++)
        if (jobs[f].n_pts > LOC_MAX_POINTS) return ORBFE_E_CAPACITY;
    // the workgroup's LDS frame is sized for the largest frame it takes: min(cap, 2048) keypoints
    const int nmax = std::min<int>(cap, MT_BAND_MAXN);
    orbfe_frame G = *geom;
    G.n = nmax;
    BlkGeom gm;
    if (!blk_geom(&G, gm)) return ORBFE_E_CAPACITY;
    if (!slab_rows_ok(nframes, cap)) return ORBFE_E_CAPACITY;
    // one upload for the call: the scale factors, every distinct point array, the skip bitsets, the slot
    // rows and their Observations, the job table and the zeroed completion counter
    orbfe_stereo_rig rig;
    memset(&rig, 0, sizeof(rig));
    if (model) rig.left = *model;
    Plan p;
    const size_t o_scale = p.upload(geom->scale_factors, (size_t)geom->nlevels * 4);
    std::vector<LocJob> lj(nframes);
    std::vector<std::vector<uint32_t>> bits(nframes);
    UploadOnce shared;
    size_t nview_words = 0;
    for (int f = 0; f < nframes; f++) {
        const orbfe_local_job& j = jobs[f];
        LocJob& t = lj[f];
        memset(&t, 0, sizeof(t));
        if (!make_camdev(geom, &j.cam, model ? &rig : nullptr, t.cd)) return ORBFE_E_ARG;
        t.n_pts = j.n_pts;
        t.th = j.th;
        t.o_skip = ~(size_t)0;
        t.view = -1;
        if (j.n_pts == 0) continue;
        t.o_pts = shared(p, j.pts, (uintptr_t)j.n_pts, (size_t)j.n_pts * sizeof(orbfe_map_point_3d));
        if (j.n_skip > 0) {
            bits[f].assign(((size_t)j.n_pts + 31) / 32, 0u);
            for (int k = 0; k < j.n_skip; k++) bits[f][j.skip[k] >> 5] |= 1u << (j.skip[k] & 31);
            t.o_skip = p.upload(bits[f].data(), bits[f].size() * 4);
        }
        if (j.in_view) {
            t.view = (int)nview_words;
            nview_words += 2 * (((size_t)j.n_pts + 63) / 64);
        }
    }
    const size_t nrow = (size_t)nframes * cap;
    const size_t o_rows_in = p.upload(mvp_in, nrow * 4);
    const size_t o_obs_in = p.upload(mvp_obs, nrow * 4);
    const size_t o_done = ms_plan_done(p);
    // (the job table is uploaded last: it holds the scratch offsets, which follow every upload)
    const size_t o_jobs = p.upload(lj.data(), (size_t)nframes * sizeof(LocJob));
    const size_t o_rows = p.scratch(nrow * 4);
    for (int f = 0; f < nframes; f++)
        if (lj[f].n_pts > 0)
            lj[f].o_recs = p.scratch((size_t)std::min<int>(lj[f].n_pts, MT_BLOCK_MAXQ) * sizeof(orbfe_map_point));
    const size_t nout = nrow + 4 * (size_t)nframes + nview_words;   // the rows, the counts, the view bits
    LocIn in;
    memset(&in, 0, sizeof(in));
    MSCHK(ms_batch_prepare(p, nout, o_done, in.end));
    t_local_uploads = (int)shared.seen.size();
    MatchScratch& m = t_ms;
    hipStream_t s = m.stream;
    MSCHK(ms_after_caller(stream));
    MsTimer timer(s);
    const FrameDev fr = ms_geom_frame(geom, o_scale);
    in.sl = SlabView{(const OrbKeyPoint*)d_kps, d_desc, d_counts, d_uright, cap, base, step, nmax};
    in.jobs = ms_ptr<const LocJob>(o_jobs);
    in.arena = ms_ptr<uint8_t>(0);
    in.rows_in = ms_ptr<const int32_t>(o_rows_in);
    in.obs_in = ms_ptr<const int32_t>(o_obs_in);
    in.rows = ms_ptr<int32_t>(o_rows);
    in.mvp_out = m.ho_dev;
    in.counts_out = m.ho_dev + nrow;
    in.view_out = m.ho_dev + nrow + 4 * (size_t)nframes;
    in.bFar = bFarPoints ? 1 : 0;
    in.thFar = thFarPoints;
    in.nnratio = nnratio;
    // one workgroup per frame, each with k_sbp_block's LDS frame for nmax keypoints
    hipLaunchKernelGGL(k_local_batch, dim3(nframes), dim3(MT_BLK_NT), blk_lds(nmax, geom->nlevels, gm), s, fr, gm, in);
    HIPCHK(hipGetLastError());
    timer.end();
    MSCHK(ms_wait_seq(s, in.end.seq));
    memcpy(mvp_out, m.ho, nrow * 4);   // complete: the sequence word comes after every workgroup's release
    for (int f = 0; f < nframes; f++) {
        const int* co = m.ho + nrow + 4 * (size_t)f;
        const int N = co[2];
        nmatches[f] = co[0] < 0 ? co[0] : co[0] - co[1];
        n_to_match[f] = co[3];
        n_keys[f] = N;
        if (co[0] < 0) t_local_batch[2]++;
        else if (jobs[f].n_pts == 0 || N == 0 || co[3] == 0) t_local_batch[1]++;
        else t_local_batch[0]++;
        if (jobs[f].in_view) {
            const uint32_t* w = (const uint32_t*)(m.ho + nrow + 4 * (size_t)nframes + lj[f].view);
            for (int k = 0; k < jobs[f].n_pts; k++) jobs[f].in_view[k] = (uint8_t)((w[k >> 5] >> (k & 31)) & 1u);
        }
    }
    return ORBFE_OK;
}

int orbfe_matcher_last_local_batch(int32_t* out) {
    if (!out) return ORBFE_E_ARG;
    for (int i = 0; i < 3; i++) out[i] = t_local_batch[i];
    return ORBFE_OK;
}

int orbfe_matcher_last_local_uploads(void) { return t_local_uploads; }

}  // extern "C"
