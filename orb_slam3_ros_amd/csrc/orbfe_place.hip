// Loop-closure place recognition on CDNA4 (included into orbfe_engine.hip last: it uses the matcher's
// per-thread arena, the resident orbfe_keyframe, k_bow_kfkf and the keyframe database's query).
//  * orbfe_search_by_bow_kf_batch: SearchByBoW(KF1, KF2[c]) (ORBmatcher.cc:765-903) for every
//    candidate c of LoopClosing::DetectCommonRegionsFromBoW (LoopClosing.cc:1596-1705) in one launch
//    over resident keyframes.
//  * orbfe_kfdb_detect_nbest: KeyFrameDatabase::DetectNBestCandidates (KeyFrameDatabase.cc:604-730)
//    on the database's device query, the tail on the host.
#pragma once

// One side of a KF-KF search: a resident pack (orbfe_keyframe), its map-point handles in the call's
// upload range and the index limit of a two-camera keyframe.
struct KfBowSide {
    const uint4* pack;   // node ids at byte 0, then the arrays at the offsets below
    int nvec;            // 16-byte words of the pack
    int o_off, o_idx, o_ang, o_desc;
    int nn, n;           // nodes, features
    int lim;             // indices >= lim take no part (NLeft of a two-camera keyframe, else n)
    int mp_vec;          // map-point handles: 16-byte word index from KfBowBatchIn::mp_base
    int mode;            // KF2 only. 0: match here; 1: the row is -1; 2: the multi-launch path writes this row
};
struct KfBowBatchIn {
    const KfBowSide* cands;
    KfBowSide k1;
    const uint4* mp_base;
    int checkOri;
    float nnratio;
    int* out;   // [n_kfs][k1.n]
    int* nm;    // [n_kfs]
};
// LDS bytes of one workgroup: both packs, both handle arrays, KF1 index -> matched KF2 index, and a
// "matched" byte per KF2 index (the host's fit test and the kernel's layout)
__host__ __device__ inline size_t kf_bow_batch_lds(int nvec1, int n1, int nvec2, int n2) {
    return ((size_t)nvec1 + (size_t)nvec2 + (size_t)((n1 + 3) / 4) + (size_t)((n2 + 3) / 4)) * 16 + (size_t)n1 * 4 +
           (((size_t)n2 + 15) & ~(size_t)15);
}

// SearchByBoW(KF1, KF2[c]) in one workgroup per candidate c: both packs, both handle arrays and the
// match state staged in LDS; one quad of lanes per KF1 node, its KF2 node found by binary search of
// KF2's node ids; the node walked by bow_walk_node under BowRulesKfKf (a KF2 index belongs to one node
// only, checked at create, so vbMatched2 is private to the quad); the row vpMatches12[idx1] =
// mp2[bestIdx2] committed in the block; nm[c] written last and read after a stream synchronisation.
__global__ __launch_bounds__(MT_BOW_NT) void k_bow_kfkf_batch(KfBowBatchIn in) {
    extern __shared__ __attribute__((aligned(16))) uint8_t kb_sm[];
    __shared__ int s_hist[MT_HISTO];
    __shared__ unsigned s_keep;
    __shared__ int s_n;
    const int tid = threadIdx.x, c = blockIdx.x;
    // every lane reads the same record: the branches and trip counts below are workgroup-uniform, so
    // the whole workgroup leaves here or reaches every SYNC()
    const KfBowSide cd = in.cands[c];
    const int n1 = in.k1.n;
    if (cd.mode == 2) return;
    int* out = in.out + (size_t)c * n1;
    if (cd.mode != 0) {
        for (int i = tid; i < n1; i += MT_BOW_NT) out[i] = -1;
        if (tid == 0) in.nm[c] = 0;
        return;
    }
    uint4* s_p1 = (uint4*)kb_sm;
    uint4* s_p2 = s_p1 + in.k1.nvec;
    uint4* s_mp1w = s_p2 + cd.nvec;
    uint4* s_mp2w = s_mp1w + (n1 + 3) / 4;
    int* s_m12 = (int*)(s_mp2w + (cd.n + 3) / 4);   // KF1 index -> matched KF2 index (-1)
    uint8_t* s_taken = (uint8_t*)(s_m12 + n1);      // vbMatched2 of the nodes walked in LDS
    const uint4* g_mp1 = in.mp_base + in.k1.mp_vec;
    const uint4* g_mp2 = in.mp_base + cd.mp_vec;
#pragma unroll 4
    for (int i = tid; i < in.k1.nvec; i += MT_BOW_NT) s_p1[i] = in.k1.pack[i];
#pragma unroll 4
    for (int i = tid; i < cd.nvec; i += MT_BOW_NT) s_p2[i] = cd.pack[i];
    for (int i = tid; i < (n1 + 3) / 4; i += MT_BOW_NT) s_mp1w[i] = g_mp1[i];
    for (int i = tid; i < (cd.n + 3) / 4; i += MT_BOW_NT) s_mp2w[i] = g_mp2[i];
    for (int i = tid; i < n1; i += MT_BOW_NT) s_m12[i] = -1;
    for (int i = tid; i < (cd.n + 15) / 16 * 4; i += MT_BOW_NT) ((int*)s_taken)[i] = 0;
    if (tid < MT_HISTO) s_hist[tid] = 0;
    if (tid == 0) s_n = 0;
    SYNC();
    const unsigned* s_nid1 = (const unsigned*)s_p1;
    const int* s_o1 = (const int*)((const uint8_t*)s_p1 + in.k1.o_off);
    const int* s_i1 = (const int*)((const uint8_t*)s_p1 + in.k1.o_idx);
    const float* s_ang1 = (const float*)((const uint8_t*)s_p1 + in.k1.o_ang);
    const uint4* s_d1 = (const uint4*)((const uint8_t*)s_p1 + in.k1.o_desc);
    const unsigned* s_nid2 = (const unsigned*)s_p2;
    const int* s_o2 = (const int*)((const uint8_t*)s_p2 + cd.o_off);
    const int* s_i2 = (const int*)((const uint8_t*)s_p2 + cd.o_idx);
    const float* s_ang2 = (const float*)((const uint8_t*)s_p2 + cd.o_ang);
    const uint4* s_d2 = (const uint4*)((const uint8_t*)s_p2 + cd.o_desc);
    const int* s_mp1 = (const int*)s_mp1w;
    const int* s_mp2 = (const int*)s_mp2w;
    const BowRulesKfKf rules{s_mp1, s_mp2, s_m12, s_taken, in.k1.lim, cd.lim, in.nnratio};
    for (int a = tid >> 2; a < in.k1.nn; a += MT_BOW_NT / 4) {
        const unsigned id = s_nid1[a];
        int b = 0, hi = cd.nn;   // lower_bound of the node id among KF2's (the quad's lanes agree)
        while (b < hi) {
            const int mid = (b + hi) >> 1;
            if (s_nid2[mid] < id) b = mid + 1;
            else hi = mid;
        }
        if (b >= cd.nn || s_nid2[b] != id) continue;
        bow_walk_node(s_o1[a], s_o1[a + 1], s_o2[b], s_o2[b + 1], s_i1, s_i2, s_d1, s_d2, tid & 3, rules);
    }
    SYNC();
    bow_commit_rows<true>(n1, s_m12, [&](int, int i) { return s_ang1[i]; }, AngFlat{s_ang2}, s_mp2, in.checkOri, out,
                          s_hist, &s_keep, &s_n);
    SYNC();
    if (tid == 0) in.nm[c] = s_n;   // the host reads the rows after a stream synchronisation
}

namespace {
// orbfe_matcher_last_bow_kf_batch: one workgroup, empty row, multi-launch (host record)
thread_local int t_bow_kf_batch[3] = {0, 0, 0};
}  // namespace

extern "C" {

int orbfe_search_by_bow_kf_batch(const orbfe_keyframe* kf1, const int32_t* mp1, int32_t nleft1,
                                 const orbfe_keyframe* const* kfs2, const int32_t* const* mp2, const int32_t* nleft2,
                                 int32_t n_kfs, int32_t* out12, int32_t* nmatches, float nnratio, int32_t checkOri) {
    t_bow_kf_batch[0] = t_bow_kf_batch[1] = t_bow_kf_batch[2] = 0;
    // every refusal below comes before any device work and before any write to out12 / nmatches
    if (n_kfs < 0 || !out12 || !nmatches) return ORBFE_E_ARG;
    if (n_kfs == 0) return ORBFE_OK;
    if (!kf1 || !kfs2 || !mp2) return ORBFE_E_ARG;
    const int n1 = kf1->n;
    if ((n1 > 0 && !mp1) || nleft1 < -1 || nleft1 > n1 || !kf1->unique) return ORBFE_E_ARG;
    bool any = false;
    for (int c = 0; c < n_kfs; c++) {
        const orbfe_keyframe* k = kfs2[c];
        if (!k) continue;
        if ((k->n > 0 && !mp2[c]) || !k->unique) return ORBFE_E_ARG;
        if (nleft2 && (nleft2[c] < -1 || nleft2[c] > k->n)) return ORBFE_E_ARG;
        any = any || k->bow;
    }
    if ((size_t)n_kfs * (size_t)n1 + (size_t)n_kfs > ((size_t)1 << 28)) return ORBFE_E_CAPACITY;
    const bool live = any && kf1->bow;   // else every row is empty and the call needs no device
    if (live) {   // a handle belongs to its create's device
        int dev = 0;
        HIPCHK(hipGetDevice(&dev));
        if (kf1->device != dev) return ORBFE_E_ARG;
        for (int c = 0; c < n_kfs; c++)
            if (kfs2[c] && kfs2[c]->device != dev) return ORBFE_E_ARG;
    }
    for (int c = 0; c < n_kfs; c++) nmatches[c] = 0;
    for (size_t i = 0; i < (size_t)n_kfs * n1; i++) out12[i] = -1;
    t_bow_kf_batch[1] = n_kfs;   // the rows above are the result of a call that ends before the launch
    if (!live) return ORBFE_OK;
    // per candidate: mp2[c] is the only upload; one that shares no node with KF1 gets the empty row; one
    // that does not fit a workgroup (the bounds of orbfe_search_by_bow_batch) keeps its node pairs for
    // the multi-launch path
    Plan p;
    const size_t o_mp1 = p.upload(mp1, (size_t)n1 * 4);
    std::vector<KfBowSide> cands(n_kfs);
    std::vector<size_t> o_mp2(n_kfs, 0), o_pairs(n_kfs, 0), o_m2(n_kfs, 0), o_oi(n_kfs, 0);
    std::vector<std::vector<int32_t>> pairs(n_kfs);
    const size_t lds_max = 150 * 1024;
    size_t lds = 0;
    int nlive = 0;
    auto side = [](const orbfe_keyframe* k, int nleft) {
        return KfBowSide{(const uint4*)k->pack, k->nvec, k->o_off, k->o_idx, k->o_ang, k->o_desc, k->nn, k->n,
                         nleft >= 0 ? nleft : k->n, 0, 0};
    };
    for (int c = 0; c < n_kfs; c++) {
        const orbfe_keyframe* k = kfs2[c];
        KfBowSide& cd = cands[c];
        memset(&cd, 0, sizeof(cd));
        cd.mode = 1;
        if (!k || !k->bow) continue;
        fv_join(kf1->node_ids.data(), kf1->nn, k->node_ids.data(), k->nn, pairs[c]);
        if (pairs[c].empty()) continue;
        o_mp2[c] = p.upload(mp2[c], (size_t)k->n * 4);
        cd = side(k, nleft2 ? nleft2[c] : -1);
        const size_t need = kf_bow_batch_lds(kf1->nvec, n1, k->nvec, k->n) + 16;
        if (need <= lds_max && n1 <= MT_BOW_FR * MT_BOW_NT) {
            lds = std::max(lds, need);
            nlive++;
            std::vector<int32_t>().swap(pairs[c]);
            continue;
        }
        cd.mode = 2;
        o_pairs[c] = p.upload(pairs[c].data(), pairs[c].size() * 4);
    }
    for (int c = 0; c < n_kfs; c++) cands[c].mp_vec = (int)(o_mp2[c] / 16);
    t_bow_kf_batch[1] = 0;
    for (int c = 0; c < n_kfs; c++) t_bow_kf_batch[cands[c].mode]++;
    if (t_bow_kf_batch[1] == n_kfs) return ORBFE_OK;   // no candidate shares a node: the rows are written
    const size_t o_cands = p.upload(cands.data(), (size_t)n_kfs * sizeof(KfBowSide));
    for (int c = 0; c < n_kfs; c++)
        if (cands[c].mode == 2) {
            o_m2[c] = p.scratch((size_t)kfs2[c]->n * 4);
            o_oi[c] = p.scratch((size_t)n1 * 4);
        }
    int rc = ms_prepare(p);
    if (rc) return rc;
    const size_t nout = (size_t)n_kfs * n1 + (size_t)n_kfs;   // the rows, then nmatches
    MSCHK(ms_out_rows(nout));
    MatchScratch& m = t_ms;
    MsTimer timer;
    hipStream_t s = m.stream;
    int* d_out = m.ho_dev;
    int* d_nm = m.ho_dev + (size_t)n_kfs * n1;
    const int lim1 = nleft1 >= 0 ? nleft1 : n1;
    for (int c = 0; c < n_kfs; c++) {
        if (cands[c].mode != 2) continue;
        const orbfe_keyframe* k = kfs2[c];
        const int npairs = (int)pairs[c].size() / 2;
        fill(ms_ptr<int>(o_m2[c]), k->n, 0);
        fill(ms_ptr<int>(o_oi[c]), n1, -1);
        hipLaunchKernelGGL(k_bow_kfkf, dim3((npairs + MT_NT - 1) / MT_NT), dim3(MT_NT), 0, s,
                           ms_ptr<const int>(o_pairs[c]), npairs, (const int*)(kf1->pack + kf1->o_off),
                           (const uint32_t*)(kf1->pack + kf1->o_idx), (const int*)(k->pack + k->o_off),
                           (const uint32_t*)(k->pack + k->o_idx), ms_ptr<const int32_t>(o_mp1),
                           ms_ptr<const int32_t>(o_mp2[c]), (const uint32_t*)(kf1->pack + kf1->o_desc),
                           (const uint32_t*)(k->pack + k->o_desc), nnratio, ms_ptr<int>(o_m2[c]), ms_ptr<int>(o_oi[c]),
                           lim1, cands[c].lim);
        hipLaunchKernelGGL((k_bow_commit<true, AngFlat, AngFlat>), dim3(1), dim3(1024), 0, s,
                           AngFlat{(const float*)(kf1->pack + kf1->o_ang)}, AngFlat{(const float*)(k->pack + k->o_ang)},
                           n1, ms_ptr<const int32_t>(o_mp2[c]), checkOri, ms_ptr<const int>(o_oi[c]),
                           d_out + (size_t)c * n1, d_nm + c);
    }
    // one workgroup per candidate; the dynamic LDS is the largest fitting candidate's. A batch whose
    // live candidates all took the multi-launch path still runs it for the empty rows (no LDS then).
    KfBowBatchIn in;
    in.cands = ms_ptr<const KfBowSide>(o_cands);
    in.k1 = side(kf1, nleft1);
    in.k1.mp_vec = (int)(o_mp1 / 16);
    in.mp_base = ms_ptr<const uint4>(0);
    in.checkOri = checkOri ? 1 : 0;
    in.nnratio = nnratio;
    in.out = d_out;
    in.nm = d_nm;
    hipLaunchKernelGGL(k_bow_kfkf_batch, dim3(n_kfs), dim3(MT_BOW_NT), nlive ? lds : 0, s, in);
    HIPCHK(hipGetLastError());
    timer.end();
    // completion: every workgroup's stores (and the multi-launch kernels') are visible in the mapped
    // pinned block once the stream has drained
    HIPCHK(hipStreamSynchronize(s));
    memcpy(out12, m.ho, (size_t)n_kfs * n1 * 4);
    memcpy(nmatches, m.ho + (size_t)n_kfs * n1, (size_t)n_kfs * 4);
    return ORBFE_OK;
}

int orbfe_matcher_last_bow_kf_batch(int32_t* out) {
    if (!out) return ORBFE_E_ARG;
    for (int i = 0; i < 3; i++) out[i] = t_bow_kf_batch[i];
    return ORBFE_OK;
}

int orbfe_kfdb_detect_nbest(orbfe_kfdb* db, const uint32_t* q_word_ids, const double* q_weights, int32_t q_n,
                            const int32_t* connected_ids, int32_t n_connected, int32_t map_id,
                            const int32_t* bad_map_ids, int32_t n_bad_maps, int32_t n_candidates, orbfe_kf_info_fn info,
                            void* ctx, int32_t* loop_ids, int32_t* n_loop, int32_t* merge_ids, int32_t* n_merge) {
    if (!n_loop || !n_merge || n_candidates < 0 || (n_candidates > 0 && (!loop_ids || !merge_ids))) return ORBFE_E_ARG;
    if (n_connected < 0 || (n_connected > 0 && !connected_ids) || n_bad_maps < 0 || (n_bad_maps > 0 && !bad_map_ids))
        return ORBFE_E_ARG;
    if (!kfdb_query_args(db, q_word_ids, q_weights, q_n)) return ORBFE_E_ARG;
    std::lock_guard<std::mutex> lock(db->mu);
    KfdbQuery q;
    MSCHK(kfdb_query(db, q_word_ids, q_weights, q_n, q));
    const size_t n_ent = db->ent.size();
    // spConnectedKF: a connected keyframe never enters lKFsSharingWords (:626), so it is out of
    // maxCommonWords and carries no stamp. stamp[e]: mnPlaceRecognitionQuery == pKF->mnId.
    std::vector<uint8_t> stamp(q.shares);
    stamp.resize(n_ent, 0);
    for (int i = 0; i < n_connected; i++) {
        const auto it = db->index.find(connected_ids[i]);
        if (it != db->index.end()) stamp[it->second] = 0;
    }
    int maxCommonWords = 0;
    for (size_t i = 0; i < q.list.size(); i++)
        if (stamp[q.list[i]] && q.words[i] > maxCommonWords) maxCommonWords = q.words[i];
    const int minCommonWords = (int)(maxCommonWords * 0.8f);
    // this query's scores beside the stored ones; committed only when the call succeeds
    std::vector<float> ps(n_ent);
    for (size_t e = 0; e < n_ent; e++) ps[e] = db->ent[e].place_score;
    std::vector<int> sc;   // lScoreAndMatch as positions in q.list
    for (size_t i = 0; i < q.list.size(); i++)
        if (stamp[q.list[i]] && q.words[i] > minCommonWords) {
            ps[q.list[i]] = q.score[i];
            sc.push_back((int)i);
        }
    if (sc.empty()) {
        *n_loop = *n_merge = 0;
        return ORBFE_OK;
    }
    struct Info {
        int32_t n, map;
        int32_t nb[10];
    };
    std::unordered_map<int32_t, Info> cache;   // info is asked at most once per keyframe id
    bool bad_info = false;
    auto ask = [&](int32_t id) -> const Info& {
        auto it = cache.find(id);
        if (it != cache.end()) return it->second;
        Info in;
        in.n = 0;
        in.map = map_id;
        if (info) {
            in.n = info(ctx, id, in.nb, &in.map);
            if (in.n < 0 || in.n > 10) { bad_info = true; in.n = 0; }
        }
        return cache.emplace(id, in).first->second;
    };
    // accumulate score by covisibility (:675-700)
    std::vector<std::pair<float, int>> acc;   // (accScore, pBestKF as an entry)
    for (int i : sc) {
        const int ei = q.list[i];
        const Info& in = ask(db->ent[ei].id);
        float bestScore = q.score[i];
        float accScore = bestScore;
        int best = ei;
        for (int k = 0; k < in.n; k++) {
            const auto it = db->index.find(in.nb[k]);
            if (it == db->index.end() || !stamp[it->second]) continue;   // mnPlaceRecognitionQuery != pKF->mnId
            const float s2 = ps[it->second];
            accScore += s2;
            if (s2 > bestScore) {
                best = it->second;
                bestScore = s2;
            }
        }
        acc.emplace_back(accScore, best);
    }
    // lAccScoreAndMatch.sort(compFirst): std::list::sort is stable
    std::stable_sort(acc.begin(), acc.end(),
                     [](const std::pair<float, int>& a, const std::pair<float, int>& b) { return a.first > b.first; });
    // the selection walk (:707-729)
    std::vector<int32_t> loop, merge;
    std::vector<uint8_t> added(n_ent, 0);
    for (size_t i = 0; i < acc.size() && ((int)loop.size() < n_candidates || (int)merge.size() < n_candidates); i++) {
        const int e = acc[i].second;
        if (added[e]) continue;
        const int32_t id = db->ent[e].id;
        const int32_t map = ask(id).map;
        if (map == map_id && (int)loop.size() < n_candidates) {
            loop.push_back(id);
        } else if (map != map_id && (int)merge.size() < n_candidates) {
            bool bad = false;
            for (int k = 0; k < n_bad_maps; k++) bad = bad || bad_map_ids[k] == map;
            if (!bad) merge.push_back(id);
        }
        added[e] = 1;
    }
    if (bad_info) return ORBFE_E_ARG;
    for (int i : sc) db->ent[q.list[i]].place_score = q.score[i];   // pKFi->mPlaceRecognitionScore = si
    *n_loop = (int32_t)loop.size();
    *n_merge = (int32_t)merge.size();
    if (!loop.empty()) memcpy(loop_ids, loop.data(), loop.size() * 4);
    if (!merge.empty()) memcpy(merge_ids, merge.data(), merge.size() * 4);
    return ORBFE_OK;
}

}  // extern "C"
