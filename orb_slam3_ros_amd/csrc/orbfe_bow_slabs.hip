// TrackReferenceKeyFrame's and Relocalization's SearchByBoW(pKF, F, vpMapPointMatches) (Tracking.cc:2836,
// :3680-3701) for many (frame, keyframe) jobs in ONE launch, the frames read where orbfe_extract_batch left
// them and their FeatureVectors where orbfe_vocabulary_transform_batch left them (included into
// orbfe_engine.hip's translation unit after orbfe_local_batch.hip; the slab addressing, the completion and
// the host scaffold are orbfe_matcher.hip's SlabView, mt_batch_end and ms_* helpers).
//
// Workgroup j = job j = (frame f = image base + f * step, resident keyframe). N and the FeatureVector's
// {bow_n, fv_n} are read on the device, so is the decision how the job runs:
//   LDS form  the frame's FeatureVector row and descriptors, the keyframe pack, kf_mp and the F -> KF match
//             state staged in LDS, laid out by the actual N and fv_n (k_bow_batch's layout, frame side first);
//   HBM form  a job that does not fit the call's LDS request keeps only the match state and F's node ids and
//             offsets in LDS and walks with the descriptors, the index lists, the pack and kf_mp read in place.
// Both forms are one function (bow_join_match, k_bow_batch's, with nleft = -1). The pointers differ, not the
// algorithm.
#pragma once

#define BOWS_FORM_LDS 0
#define BOWS_FORM_EMPTY 1
#define BOWS_FORM_HBM 2
#define BOWS_FORM_REFUSED 3
#define BOWS_NMAX (MT_BOW_FR * MT_BOW_NT)   // bow_commit_rows' row limit

// Job j on the device. live == 0: a NULL keyframe, or one without features or FeatureVector (the row is
// empty whatever the frame holds). o_mp: kf_mp's offset in the call's arena.
struct BowSlabJob {
    const uint4* pack;
    size_t o_mp;
    int nvec, o_off, o_idx, o_ang, o_desc;
    int nn, kf_n;
    int frame, live;
};
// sl: the extractor's batch outputs (no uright; nmax: min(cap, BOWS_NMAX)); fv_* / bcounts: the
// orbfe_bow_batch rows of the same images (row stride cap, offsets cap + 1). out: [n_jobs][cap] rows in mapped
// pinned memory, each slot stored once; res: [n_jobs][3] = {nmatches (or the refusal's code), N, form}. lds:
// the launch's dynamic LDS bytes. end: the call's completion (mt_batch_end).
struct BowSlabIn {
    SlabView sl;
    const uint32_t* fv_nid;
    const int* fv_off;
    const uint32_t* fv_idx;
    const int* bcounts;
    const BowSlabJob* jobs;
    const uint8_t* arena;
    int32_t* out;
    int* res;
    BatchEnd end;
    int checkOri;
    unsigned lds;
    float nnratio;
};
__host__ __device__ inline size_t bows_a16(size_t b) { return (b + 15) & ~(size_t)15; }
// LDS bytes of F's node ids and offsets (both forms keep them) and of the two forms as a whole
__host__ __device__ inline size_t bows_meta_lds(int fvn) {
    return bows_a16((size_t)fvn * 4) + bows_a16(((size_t)fvn + 1) * 4);
}
__host__ __device__ inline size_t bows_lds_full(int fvn, int nidx, int n, int nvec, int kf_n) {
    return bows_meta_lds(fvn) + bows_a16((size_t)nidx * 4) + (size_t)n * 32 + (size_t)nvec * 16 +
           (size_t)((kf_n + 3) / 4) * 16 + (size_t)n * 4;
}
__host__ __device__ inline size_t bows_lds_hbm(int fvn, int n) { return bows_meta_lds(fvn) + (size_t)n * 4; }

__global__ __launch_bounds__(MT_BOW_NT) void k_bow_slabs(BowSlabIn in) {
    extern __shared__ __attribute__((aligned(16))) uint8_t bs_sm[];
    __shared__ int s_hist[MT_HISTO];
    __shared__ unsigned s_keep;
    __shared__ int s_n;
    const int tid = threadIdx.x, j = blockIdx.x;
    // every lane reads the same record and the same counts: the form and every branch and trip count below
    // are workgroup-uniform, so the whole workgroup reaches every SYNC() of the path it takes
    const BowSlabJob jb = in.jobs[j];
    const int cap = in.sl.cap, img = in.sl.image(jb.frame);
    const int N = in.sl.count(img);
    const int bown = in.bcounts[2 * img], fvn = in.bcounts[2 * img + 1];
    const int* g_fo = in.fv_off + (size_t)img * ((size_t)cap + 1);
    int* out = in.out + (size_t)j * cap;
    int form, nm = 0, nidx = 0;
    const bool over = in.sl.over(N) || bown < 0 || fvn < 0;
    if (!jb.live || (!over && (N == 0 || fvn == 0))) {
        form = BOWS_FORM_EMPTY;
    } else if (over) {
        form = BOWS_FORM_REFUSED;
        nm = ORBFE_E_CAPACITY;
    } else if (fvn > N || (nidx = g_fo[fvn]) < 0 || nidx > N) {   // not a FeatureVector of this frame
        form = BOWS_FORM_REFUSED;
        nm = ORBFE_E_ARG;
    } else if (bows_lds_full(fvn, nidx, N, jb.nvec, jb.kf_n) <= (size_t)in.lds) {
        form = BOWS_FORM_LDS;
    } else if (bows_lds_hbm(fvn, N) <= (size_t)in.lds) {
        form = BOWS_FORM_HBM;
    } else {
        form = BOWS_FORM_REFUSED;
        nm = ORBFE_E_CAPACITY;
    }
    if (form == BOWS_FORM_LDS || form == BOWS_FORM_HBM) {
        // F's angles for the commit, loaded now (their latency hides under the staging and the walks)
        const OrbKeyPoint* fkeys = in.sl.keys_of(img);
        float fang[MT_BOW_FR];
#pragma unroll
        for (int u = 0; u < MT_BOW_FR; u++) {
            const int i = tid + u * MT_BOW_NT;
            fang[u] = i < N ? fkeys[i].angle : 0.f;
        }
        const uint32_t* g_fnid = in.fv_nid + (size_t)img * cap;
        const uint32_t* g_fi = in.fv_idx + (size_t)img * cap;
        const uint4* g_fd = (const uint4*)in.sl.desc_of(img);
        const int* g_mp = (const int*)(in.arena + jb.o_mp);
        const uint8_t* pk = (const uint8_t*)jb.pack;
        unsigned* s_fnid = (unsigned*)bs_sm;
        int* s_fo = (int*)(bs_sm + bows_a16((size_t)fvn * 4));
        uint8_t* s_rest = bs_sm + bows_meta_lds(fvn);
        int bad = 0;   // an offset or index that leaves the row: the job is refused, nothing follows it
        for (int i = tid; i < fvn; i += MT_BOW_NT) s_fnid[i] = g_fnid[i];
        for (int i = tid; i <= fvn; i += MT_BOW_NT) {
            const int o = g_fo[i];
            s_fo[i] = o;
            bad |= (o < 0 || o > nidx || (i < fvn && g_fo[i + 1] < o)) ? 1 : 0;
        }
        if (tid < MT_HISTO) s_hist[tid] = 0;
        if (tid == 0) s_n = 0;
        if (form == BOWS_FORM_LDS) {
            int* s_fi = (int*)s_rest;
            uint4* s_fd = (uint4*)(s_rest + bows_a16((size_t)nidx * 4));
            uint4* s_kf = s_fd + 2 * N;
            uint4* s_mpw = s_kf + jb.nvec;
            int* s_src = (int*)(s_mpw + (jb.kf_n + 3) / 4);   // F index -> matched KF index (-1)
#pragma unroll 4
            for (int i = tid; i < jb.nvec; i += MT_BOW_NT) s_kf[i] = jb.pack[i];
#pragma unroll 4
            for (int i = tid; i < 2 * N; i += MT_BOW_NT) s_fd[i] = g_fd[i];
            for (int i = tid; i < nidx; i += MT_BOW_NT) {
                const uint32_t v = g_fi[i];
                s_fi[i] = (int)v;
                bad |= v >= (uint32_t)N ? 1 : 0;
            }
            for (int i = tid; i < (jb.kf_n + 3) / 4; i += MT_BOW_NT) s_mpw[i] = ((const uint4*)g_mp)[i];
            for (int i = tid; i < N; i += MT_BOW_NT) s_src[i] = -1;
            bad = __syncthreads_or(bad);
            if (!bad) {
                const uint8_t* sk = (const uint8_t*)s_kf;
                bow_join_match((const unsigned*)sk, (const int*)(sk + jb.o_off), (const int*)(sk + jb.o_idx),
                               (const float*)(sk + jb.o_ang), (const uint4*)(sk + jb.o_desc), (const int*)s_mpw, jb.nn,
                               s_fnid, s_fo, s_fi, s_fd, s_src, fvn, N, -1, fang, in.nnratio, in.checkOri, out, s_hist,
                               &s_keep, &s_n);
            }
        } else {
            int* s_src = (int*)s_rest;
            for (int i = tid; i < nidx; i += MT_BOW_NT) bad |= g_fi[i] >= (uint32_t)N ? 1 : 0;
            for (int i = tid; i < N; i += MT_BOW_NT) s_src[i] = -1;
            bad = __syncthreads_or(bad);
            if (!bad)
                bow_join_match((const unsigned*)pk, (const int*)(pk + jb.o_off), (const int*)(pk + jb.o_idx),
                               (const float*)(pk + jb.o_ang), (const uint4*)(pk + jb.o_desc), g_mp, jb.nn, s_fnid, s_fo,
                               (const int*)g_fi, g_fd, s_src, fvn, N, -1, fang, in.nnratio, in.checkOri, out, s_hist,
                               &s_keep, &s_n);
        }
        if (bad) {
            form = BOWS_FORM_REFUSED;
            nm = ORBFE_E_ARG;
        } else {
            nm = s_n;
            for (int i = N + tid; i < cap; i += MT_BOW_NT) out[i] = -1;
        }
    }
    if (form == BOWS_FORM_EMPTY || form == BOWS_FORM_REFUSED)
        for (int i = tid; i < cap; i += MT_BOW_NT) out[i] = -1;
    // every wave's row stores complete, the barrier, then this workgroup's release (mt_batch_end)
    __builtin_amdgcn_s_waitcnt(0);
    SYNC();
    if (tid == 0) {
        volatile int* co = in.res + 3 * (size_t)j;
        co[0] = nm;
        co[1] = N;
        co[2] = form;
        mt_batch_end(in.end);
    }
}

namespace {
// orbfe_matcher_last_bow_slabs: jobs in the LDS form, with an empty row, in the HBM form, refused
thread_local int t_bow_slabs[4] = {0, 0, 0, 0};
constexpr size_t kBowSlabsLdsMax = 150 * 1024;       // orbfe_search_by_bow_batch's bound
}  // namespace

extern "C" {

int orbfe_search_by_bow_slabs(const orbfe_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_counts,
                              int32_t cap, int32_t base, int32_t step, const orbfe_bow_batch* bows,
                              const orbfe_bow_job* jobs, int32_t n_jobs, int32_t nframes, float nnratio,
                              int32_t checkOri, int32_t* out, int32_t* nmatches, int32_t* n_keys, void* stream) {
    t_bow_slabs[0] = t_bow_slabs[1] = t_bow_slabs[2] = t_bow_slabs[3] = 0;
    // every refusal below comes before any device work and before any write to the outputs
    if (n_jobs < 0 || nframes < 0) return ORBFE_E_ARG;
    if (!slabs_ok(d_kps, d_desc, d_counts, cap, base, step) || !bows || !bows->fv_node_ids || !bows->fv_offsets ||
        !bows->fv_indices || !bows->counts || !out || !nmatches || !n_keys || (n_jobs > 0 && !jobs))
        return ORBFE_E_ARG;
    if ((uintptr_t)d_desc & 15) return ORBFE_E_ARG;   // staged with 16-byte loads
    bool any = false;
    for (int j = 0; j < n_jobs; j++) {
        const orbfe_bow_job& b = jobs[j];
        if (b.frame < 0 || b.frame >= nframes) return ORBFE_E_ARG;
        if (b.kf && b.kf->n > 0 && !b.kf_mp) return ORBFE_E_ARG;
        any = any || b.kf;
    }
    if (cap > BB_MAXN) return ORBFE_E_CAPACITY;
    if (!slab_rows_ok(n_jobs, cap)) return ORBFE_E_CAPACITY;
    if (n_jobs == 0) return ORBFE_OK;
    if (any) {   // a handle belongs to its create's device
        int dev = 0;
        HIPCHK(hipGetDevice(&dev));
        for (int j = 0; j < n_jobs; j++)
            if (jobs[j].kf && jobs[j].kf->device != dev) return ORBFE_E_ARG;
    }
    // one upload for the call: every distinct (kf_mp, keyframe) once, the job table and the zeroed completion
    // counter. The LDS request is that of the largest keyframe against a frame of min(cap, 4096) features
    // with one node per feature, up to the bound of orbfe_search_by_bow_batch.
    const int nmax = std::min<int>(cap, BOWS_NMAX);
    Plan p;
    std::vector<BowSlabJob> bj(n_jobs);
    UploadOnce shared;
    int max_nvec = 0, max_kfn = 0;
    for (int j = 0; j < n_jobs; j++) {
        const orbfe_keyframe* k = jobs[j].kf;
        BowSlabJob& t = bj[j];
        memset(&t, 0, sizeof(t));
        t.frame = jobs[j].frame;
        if (!k || !k->bow) continue;   // NULL, no features or an empty FeatureVector: the empty row
        t.pack = (const uint4*)k->pack;
        t.o_mp = shared(p, jobs[j].kf_mp, (uintptr_t)k, (size_t)k->n * 4);
        t.nvec = k->nvec;
        t.o_off = k->o_off; t.o_idx = k->o_idx; t.o_ang = k->o_ang; t.o_desc = k->o_desc;
        t.nn = k->nn;
        t.kf_n = k->n;
        t.live = 1;
        max_nvec = std::max(max_nvec, k->nvec);
        max_kfn = std::max(max_kfn, k->n);
    }
    const size_t o_jobs = p.upload(bj.data(), (size_t)n_jobs * sizeof(BowSlabJob));
    const size_t o_done = ms_plan_done(p);
    const size_t lds = std::min(kBowSlabsLdsMax, bows_lds_full(nmax, nmax, nmax, max_nvec, max_kfn));
    const size_t nrow = (size_t)n_jobs * cap, nout = nrow + 3 * (size_t)n_jobs;   // the rows, then {nm, N, form}
    BowSlabIn in;
    memset(&in, 0, sizeof(in));
    MSCHK(ms_batch_prepare(p, nout, o_done, in.end));
    MatchScratch& m = t_ms;
    hipStream_t s = m.stream;
    MSCHK(ms_lds_optin<k_bow_slabs>(m.device, lds, kBowSlabsLdsMax));
    MSCHK(ms_after_caller(stream));   // the slabs and the FeatureVectors were written on the caller's stream
    MsTimer timer(s);
    in.sl = SlabView{(const OrbKeyPoint*)d_kps, d_desc, d_counts, nullptr, cap, base, step, nmax};
    in.fv_nid = bows->fv_node_ids;
    in.fv_off = bows->fv_offsets;
    in.fv_idx = bows->fv_indices;
    in.bcounts = bows->counts;
    in.jobs = ms_ptr<const BowSlabJob>(o_jobs);
    in.arena = ms_ptr<const uint8_t>(0);
    in.out = m.ho_dev;
    in.res = m.ho_dev + nrow;
    in.checkOri = checkOri ? 1 : 0;
    in.lds = (unsigned)lds;
    in.nnratio = nnratio;
    // one workgroup per job
    hipLaunchKernelGGL(k_bow_slabs, dim3(n_jobs), dim3(MT_BOW_NT), lds, s, in);
    HIPCHK(hipGetLastError());
    timer.end();
    MSCHK(ms_wait_seq(s, in.end.seq));
    memcpy(out, m.ho, nrow * 4);   // complete: the sequence word comes after every workgroup's release
    for (int j = 0; j < n_jobs; j++) {
        const int* co = m.ho + nrow + 3 * (size_t)j;
        nmatches[j] = co[0];
        n_keys[j] = co[1];
        if (co[2] >= 0 && co[2] < 4) t_bow_slabs[co[2]]++;
    }
    return ORBFE_OK;
}

int orbfe_matcher_last_bow_slabs(int32_t* out) {
    if (!out) return ORBFE_E_ARG;
    for (int i = 0; i < 4; i++) out[i] = t_bow_slabs[i];
    return ORBFE_OK;
}

}  // extern "C"
