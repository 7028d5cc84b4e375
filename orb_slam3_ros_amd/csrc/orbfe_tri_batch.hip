// LocalMapping's new-point search on CDNA4 (included into orbfe_engine.hip last: it uses the matcher's
// per-thread arena, the resident orbfe_keyframe with geometry, tri_walk / k_tri and the BoW commit).
//  * orbfe_search_for_triangulation_batch: SearchForTriangulation(KF1, KF2[c]) (ORBmatcher.cc:907-1146)
//    for every covisible neighbour c of LocalMapping::CreateNewMapPoints (LocalMapping.cc:388-470) in
//    one launch over resident keyframes.
#pragma once

// One neighbour of the batch: its resident pack (KfBowSide; lim is not used here), its geometry block,
// and the fundamental matrix and epipole of the pair.
struct TriJobDev {
    KfBowSide s;         // s.mode 0: match here; 1: the row is -1; 2: k_tri + k_bow_commit write this row
    const uint4* geom;   // [n keypoint records | scale_factors | level_sigma2]
    int gvec;            // 16-byte words of it
    int nlevels, two;
    float F[9], ep[2];
};
struct TriBatchIn {
    const TriJobDev* jobs;
    KfBowSide k1;        // read in HBM
    const float4* geom1;
    int two1, nki1;      // KF1: second camera; entries of its FeatureVector
    const uint4* mp_base;
    int bOnlyStereo, bCoarse, checkOri;
    int* out;   // [n_jobs][k1.n]
    int* nm;    // [n_jobs]
};
// LDS bytes of one workgroup: the neighbour's pack, its geometry block, its map-point presence and
// KF1 index -> matched KF2 index (the host's fit test and the kernel's layout)
__host__ __device__ inline size_t tri_batch_lds(int n1, int nvec2, int gvec2, int n2) {
    return ((size_t)nvec2 + (size_t)gvec2 + (size_t)((n2 + 3) / 4)) * 16 + (size_t)n1 * 4;
}

// SearchForTriangulation(KF1, KF2[c]) in one workgroup per neighbour c: KF2's pack, geometry block and
// mp2 staged in LDS with 16-byte loads; KF1 (the same for every workgroup, so L2-resident) read in HBM,
// once per FeatureVector entry. One lane per KF1 entry: its node from KF1's offsets, that node among
// KF2's node ids by binary search, then tri_walk through the KF2 node in order (vbMatched2 is never set
// by the reference, so the entries are independent, and a KF1 index sits in one node only, checked at
// create, so s_m12[i1] has one writer). The rotation commit runs in the block; the row holds the KF2
// index itself; nm[c] is written last and read after a stream synchronisation.
__global__ __launch_bounds__(MT_BOW_NT) void k_tri_batch(TriBatchIn in) {
    extern __shared__ __attribute__((aligned(16))) uint8_t tb_sm[];
    __shared__ int s_hist[MT_HISTO];
    __shared__ unsigned s_keep;
    __shared__ int s_n;
    const int tid = threadIdx.x, c = blockIdx.x;
    // every lane reads the same record: the branches and trip counts ahead of each SYNC() are
    // workgroup-uniform, so the whole workgroup leaves here or reaches every barrier
    const TriJobDev jd = in.jobs[c];
    const KfBowSide& cd = jd.s;
    const int n1 = in.k1.n;
    if (cd.mode == 2) return;
    int* out = in.out + (size_t)c * n1;
    if (cd.mode != 0) {
        for (int i = tid; i < n1; i += MT_BOW_NT) out[i] = -1;
        if (tid == 0) in.nm[c] = 0;
        return;
    }
    uint4* s_p2 = (uint4*)tb_sm;
    uint4* s_g2 = s_p2 + cd.nvec;
    uint4* s_mp2w = s_g2 + jd.gvec;
    int* s_m12 = (int*)(s_mp2w + (cd.n + 3) / 4);   // KF1 index -> matched KF2 index (-1)
    const uint4* g_mp2 = in.mp_base + cd.mp_vec;
#pragma unroll 4
    for (int i = tid; i < cd.nvec; i += MT_BOW_NT) s_p2[i] = cd.pack[i];
#pragma unroll 4
    for (int i = tid; i < jd.gvec; i += MT_BOW_NT) s_g2[i] = jd.geom[i];
    for (int i = tid; i < (cd.n + 3) / 4; i += MT_BOW_NT) s_mp2w[i] = g_mp2[i];
    for (int i = tid; i < n1; i += MT_BOW_NT) s_m12[i] = -1;
    if (tid < MT_HISTO) s_hist[tid] = 0;
    if (tid == 0) s_n = 0;
    SYNC();
    const uint8_t* p1 = (const uint8_t*)in.k1.pack;
    const unsigned* g_nid1 = (const unsigned*)p1;
    const int* g_o1 = (const int*)(p1 + in.k1.o_off);
    const uint32_t* g_i1 = (const uint32_t*)(p1 + in.k1.o_idx);
    const float* g_ang1 = (const float*)(p1 + in.k1.o_ang);
    const uint32_t* g_d1 = (const uint32_t*)(p1 + in.k1.o_desc);
    const int32_t* g_mp1 = (const int32_t*)(in.mp_base + in.k1.mp_vec);
    const unsigned* s_nid2 = (const unsigned*)s_p2;
    const int* s_o2 = (const int*)((const uint8_t*)s_p2 + cd.o_off);
    const uint32_t* s_i2 = (const uint32_t*)((const uint8_t*)s_p2 + cd.o_idx);
    const float* s_ang2 = (const float*)((const uint8_t*)s_p2 + cd.o_ang);
    const uint32_t* s_d2 = (const uint32_t*)((const uint8_t*)s_p2 + cd.o_desc);
    const float* s_scale2 = (const float*)(s_g2 + cd.n);
    const float* s_sigma2 = s_scale2 + 4 * kf_geom_lvec(jd.nlevels);
    TriArgs a;
#pragma unroll
    for (int k = 0; k < 9; k++) a.F[k] = jd.F[k];
    a.ep[0] = jd.ep[0];
    a.ep[1] = jd.ep[1];
    a.bOnlyStereo = in.bOnlyStereo;
    a.bCoarse = in.bCoarse;
    a.two1 = in.two1;
    a.two2 = jd.two;
    for (int e = tid; e < in.nki1; e += MT_BOW_NT) {
        int lo = 0, hi = in.k1.nn;   // the node of entry e: the last na with off1[na] <= e (off1[0] = 0)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (g_o1[mid] <= e) lo = mid;
            else hi = mid;
        }
        const unsigned id = g_nid1[lo];
        int b = 0;   // lower_bound of the node id among KF2's
        hi = cd.nn;
        while (b < hi) {
            const int mid = (b + hi) >> 1;
            if (s_nid2[mid] < id) b = mid + 1;
            else hi = mid;
        }
        if (b >= cd.nn || s_nid2[b] != id) continue;
        const unsigned i1 = g_i1[e];
        const int best = tri_walk(i1, s_o2[b], s_o2[b + 1], s_i2, TriKeysGeom{in.geom1}, TriKeysGeom{(const float4*)s_g2},
                                  g_d1, s_d2, g_mp1, (const int32_t*)s_mp2w, s_scale2, s_sigma2, a);
        if (best >= 0) s_m12[i1] = best;
    }
    SYNC();
    bow_commit_rows<true>(n1, s_m12, [&](int, int i) { return g_ang1[i]; }, AngFlat{s_ang2}, RowIndex{}, in.checkOri,
                          out, s_hist, &s_keep, &s_n);
    SYNC();
    if (tid == 0) in.nm[c] = s_n;   // the host reads the rows after a stream synchronisation
}

namespace {
// orbfe_matcher_last_tri_batch: one workgroup, empty row, HBM fallback (host record)
thread_local int t_tri_batch[3] = {0, 0, 0};
}  // namespace

extern "C" {

int orbfe_search_for_triangulation_batch(const orbfe_keyframe* kf1, const int32_t* mp1, const orbfe_tri_job* jobs,
                                         int32_t n_jobs, int32_t bOnlyStereo, int32_t bCoarse, int32_t checkOri,
                                         int32_t* matches12, int32_t* nmatches) {
    t_tri_batch[0] = t_tri_batch[1] = t_tri_batch[2] = 0;
    // every refusal below comes before any device work and before any write to matches12 / nmatches
    if (n_jobs < 0 || !matches12 || !nmatches) return ORBFE_E_ARG;
    if (n_jobs == 0) return ORBFE_OK;
    if (!kf1 || !jobs) return ORBFE_E_ARG;
    const int n1 = kf1->n;
    if (!kf1->has_geom || (n1 > 0 && !mp1) || !kf1->unique || (kf1->two && !bCoarse)) return ORBFE_E_ARG;
    bool any = false;
    for (int c = 0; c < n_jobs; c++) {
        const orbfe_keyframe* k = jobs[c].kf2;
        if (!k) continue;
        if (!k->has_geom || (k->n > 0 && !jobs[c].mp2) || !k->unique || (k->two && !bCoarse)) return ORBFE_E_ARG;
        any = any || k->bow;
    }
    if ((size_t)n_jobs * (size_t)n1 + (size_t)n_jobs > ((size_t)1 << 28)) return ORBFE_E_CAPACITY;
    const bool live = any && kf1->bow;   // else every row is empty and the call needs no device
    if (live) {   // a handle belongs to its create's device
        int dev = 0;
        HIPCHK(hipGetDevice(&dev));
        if (kf1->device != dev) return ORBFE_E_ARG;
        for (int c = 0; c < n_jobs; c++)
            if (jobs[c].kf2 && jobs[c].kf2->device != dev) return ORBFE_E_ARG;
    }
    for (int c = 0; c < n_jobs; c++) nmatches[c] = 0;
    for (size_t i = 0; i < (size_t)n_jobs * n1; i++) matches12[i] = -1;
    t_tri_batch[1] = n_jobs;   // the rows above are the result of a call that ends before the launch
    if (!live) return ORBFE_OK;
    // per neighbour: mp2 is the only upload; one that shares no node with KF1 gets the empty row; one
    // that does not fit a workgroup keeps its node pairs as k_tri's item list for the HBM fallback
    Plan p;
    const size_t o_mp1 = p.upload(mp1, (size_t)n1 * 4);
    std::vector<TriJobDev> jd(n_jobs);
    std::vector<size_t> o_mp2(n_jobs, 0), o_items(n_jobs, 0), o_oi(n_jobs, 0);
    std::vector<std::vector<int2>> items(n_jobs);
    std::vector<int32_t> pairs;
    const size_t lds_max = 150 * 1024;
    size_t lds = 0;
    int nlive = 0;
    const int32_t* off1 = kf1->offs.data();
    for (int c = 0; c < n_jobs; c++) {
        const orbfe_keyframe* k = jobs[c].kf2;
        TriJobDev& j = jd[c];
        memset(&j, 0, sizeof(j));
        j.s.mode = 1;
        if (!k || !k->bow) continue;
        pairs.clear();
        fv_join(kf1->node_ids.data(), kf1->nn, k->node_ids.data(), k->nn, pairs);
        if (pairs.empty()) continue;
        o_mp2[c] = p.upload(jobs[c].mp2, (size_t)k->n * 4);
        j.s = KfBowSide{(const uint4*)k->pack, k->nvec, k->o_off, k->o_idx, k->o_ang, k->o_desc, k->nn, k->n, k->n, 0, 0};
        j.geom = (const uint4*)k->geom;
        j.gvec = k->gvec;
        j.nlevels = k->nlevels;
        j.two = k->two ? 1 : 0;
        memcpy(j.F, jobs[c].F12, sizeof(j.F));
        j.ep[0] = jobs[c].ep[0];
        j.ep[1] = jobs[c].ep[1];
        const size_t need = tri_batch_lds(n1, k->nvec, k->gvec, k->n) + 16;
        if (need <= lds_max && n1 <= MT_BOW_FR * MT_BOW_NT) {
            lds = std::max(lds, need);
            nlive++;
            continue;
        }
        // k_tri's items: one per KF1 entry of a shared node (KF1 CSR position, KF2 node)
        j.s.mode = 2;
        for (size_t q = 0; q < pairs.size(); q += 2)
            for (int ia = off1[pairs[q]]; ia < off1[pairs[q] + 1]; ia++) items[c].push_back(make_int2(ia, pairs[q + 1]));
        if (items[c].empty()) {   // the shared nodes hold no KF1 entry
            j.s.mode = 1;
            continue;
        }
        o_items[c] = p.upload(items[c].data(), items[c].size() * sizeof(int2));
    }
    for (int c = 0; c < n_jobs; c++) jd[c].s.mp_vec = (int)(o_mp2[c] / 16);
    t_tri_batch[1] = 0;
    for (int c = 0; c < n_jobs; c++) t_tri_batch[jd[c].s.mode]++;
    if (t_tri_batch[1] == n_jobs) return ORBFE_OK;   // no neighbour shares a node: the rows are written
    const size_t o_jobs = p.upload(jd.data(), (size_t)n_jobs * sizeof(TriJobDev));
    for (int c = 0; c < n_jobs; c++)
        if (jd[c].s.mode == 2) o_oi[c] = p.scratch((size_t)n1 * 4);
    int rc = ms_prepare(p);
    if (rc) return rc;
    const size_t nout = (size_t)n_jobs * n1 + (size_t)n_jobs;   // the rows, then nmatches
    MSCHK(ms_out_rows(nout));
    MatchScratch& m = t_ms;
    MsTimer timer;
    hipStream_t s = m.stream;
    int* d_out = m.ho_dev;
    int* d_nm = m.ho_dev + (size_t)n_jobs * n1;
    for (int c = 0; c < n_jobs; c++) {
        if (jd[c].s.mode != 2) continue;
        const orbfe_keyframe* k = jobs[c].kf2;
        const int nitems = (int)items[c].size();
        TriArgs ta;
        memcpy(ta.F, jd[c].F, sizeof(ta.F));
        ta.ep[0] = jd[c].ep[0];
        ta.ep[1] = jd[c].ep[1];
        ta.bOnlyStereo = bOnlyStereo != 0;
        ta.bCoarse = bCoarse != 0;
        ta.two1 = kf1->two ? 1 : 0;
        ta.two2 = k->two ? 1 : 0;
        const float* tab2 = (const float*)(k->geom + (size_t)k->n * 16);
        fill(ms_ptr<int>(o_oi[c]), n1, -1);
        hipLaunchKernelGGL((k_tri<TriKeysGeom, TriKeysGeom>), dim3((nitems + MT_NT - 1) / MT_NT), dim3(MT_NT), 0, s,
                           ms_ptr<const int2>(o_items[c]), nitems, (const uint32_t*)(kf1->pack + kf1->o_idx),
                           (const int*)(k->pack + k->o_off), (const uint32_t*)(k->pack + k->o_idx),
                           TriKeysGeom{(const float4*)kf1->geom}, TriKeysGeom{(const float4*)k->geom},
                           (const uint32_t*)(kf1->pack + kf1->o_desc), (const uint32_t*)(k->pack + k->o_desc),
                           ms_ptr<const int32_t>(o_mp1), ms_ptr<const int32_t>(o_mp2[c]), tab2,
                           tab2 + 4 * kf_geom_lvec(k->nlevels), ta, ms_ptr<int>(o_oi[c]));
        hipLaunchKernelGGL((k_bow_commit<true, AngFlat, AngFlat>), dim3(1), dim3(1024), 0, s,
                           AngFlat{(const float*)(kf1->pack + kf1->o_ang)}, AngFlat{(const float*)(k->pack + k->o_ang)},
                           n1, (const int32_t*)nullptr, checkOri, ms_ptr<const int>(o_oi[c]), d_out + (size_t)c * n1,
                           d_nm + c);
    }
    // one workgroup per neighbour; the dynamic LDS is the largest fitting neighbour's. A batch whose
    // live neighbours all took the fallback still runs it for the empty rows (no LDS then).
    TriBatchIn in;
    in.jobs = ms_ptr<const TriJobDev>(o_jobs);
    in.k1 = KfBowSide{(const uint4*)kf1->pack, kf1->nvec, kf1->o_off, kf1->o_idx, kf1->o_ang, kf1->o_desc, kf1->nn, n1,
                      n1, (int)(o_mp1 / 16), 0};
    in.geom1 = (const float4*)kf1->geom;
    in.two1 = kf1->two ? 1 : 0;
    in.nki1 = kf1->nki;
    in.mp_base = ms_ptr<const uint4>(0);
    in.bOnlyStereo = bOnlyStereo != 0;
    in.bCoarse = bCoarse != 0;
    in.checkOri = checkOri ? 1 : 0;
    in.out = d_out;
    in.nm = d_nm;
    hipLaunchKernelGGL(k_tri_batch, dim3(n_jobs), dim3(MT_BOW_NT), nlive ? lds : 0, s, in);
    HIPCHK(hipGetLastError());
    timer.end();
    // completion: every workgroup's stores (and the fallback kernels') are visible in the mapped pinned
    // block once the stream has drained
    HIPCHK(hipStreamSynchronize(s));
    memcpy(matches12, m.ho, (size_t)n_jobs * n1 * 4);
    memcpy(nmatches, m.ho + (size_t)n_jobs * n1, (size_t)n_jobs * 4);
    return ORBFE_OK;
}

int orbfe_matcher_last_tri_batch(int32_t* out) {
    if (!out) return ORBFE_E_ARG;
    for (int i = 0; i < 3; i++) out[i] = t_tri_batch[i];
    return ORBFE_OK;
}

}  // extern "C"
