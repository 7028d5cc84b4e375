// Batched Frame::ComputeBoW on device-resident frames (included into orbfe_engine.hip after
// orbfe_kfdb.hip): TemplatedVocabulary::transform(features, v, fv, levelsup) for nimg images laid out
// as the extractor's batch outputs, the counts read on the device, no host wait; and the path from
// such a batch into the keyframe database. Same semantics, bit for bit, as k_bow_descend /
// k_bow_assemble (orbfe_bow.hip), whose sort it shares.
//
// k_bowb_descend: a group of G lanes (G = the power of two >= k, 4..64) per descriptor. At every level
// lane j takes child j's 32 bytes and, beside them, that child's own child range, so a level costs two
// dependent loads (child id, then descriptor + range) instead of k serial ones; the minimum of
// (distance << 6 | j) across the group is the FIRST child with the strictly smallest distance. Nodes
// with more than G children are walked in chunks of G (strict < between chunks). The leaf and the
// node at level L - levelsup go to the image's fv_indices / fv_node_ids rows, which are scratch until
// the assemble overwrites them: no per-feature state lives outside the caller's buffers.
// k_bowb_assemble: one workgroup per image. (word, feature) keys of the features whose leaf weight is
// > 0 are compacted into LDS and sorted; run heads are ranked with a block scan; one lane per word run
// sums its weights in key order (= feature order, addWeight) or keeps the first (addIfNotExist); the
// L1 / L2 norm is ONE left-to-right double chain in word order (wave 0: 64 terms per load, added lane
// by lane); the division is parallel. The FeatureVector is the same again with (node, feature) keys.
// Weights are looked up again through the leaf node (8192 keys fill the first 64 KB of LDS).
#pragma once

#define BB_DNT 256
#define BB_ANT 1024
#define BB_MAXN MT_GRID_MAXN
#define BB_LDS_TAIL 256   // behind the keys: [0] compaction counter, [1..16] wave sums, +128 the norm

__global__ __launch_bounds__(BB_DNT) void k_bowb_descend(const uint32_t* __restrict__ vdesc, const int* __restrict__ coff,
                                                         const int* __restrict__ child,
                                                         const uint8_t* __restrict__ fdesc,
                                                         const int* __restrict__ counts, int count_stride, int cap,
                                                         int nid_level, int gshift, uint32_t* o_leaf, uint32_t* o_nid) {
    const int img = blockIdx.x;
    const int n = counts[(size_t)img * count_stride];
    if (n < 0 || n > cap) return;   // k_bowb_assemble reports it
    const int G = 1 << gshift, lane = threadIdx.x & 63, j = lane & (G - 1);
    const int i = blockIdx.y * (BB_DNT >> gshift) + ((int)threadIdx.x >> gshift);
    if (i >= n) return;   // whole groups leave: the shuffles below stay inside a group
    const uint32_t* fp = reinterpret_cast<const uint32_t*>(fdesc + ((size_t)img * cap + i) * 32);
    unsigned long long f[4];
#pragma unroll
    for (int w = 0; w < 4; w++) f[w] = (unsigned long long)fp[2 * w] | ((unsigned long long)fp[2 * w + 1] << 32);
    int fin = 0, nid = 0, level = 0;   // nid_level <= 0 -> root; a level never reached leaves 0
    int c0 = coff[0], c1 = coff[1];
    while (c1 > c0) {   // !isLeaf()
        ++level;
        int best_d = MT_INF, best = 0, b0 = 0, b1 = 0;
        for (int cb = c0; cb < c1; cb += G) {
            const int c = cb + j;
            int key = MT_INF, id = 0, o0 = 0, o1 = 0;
            if (c < c1) {
                id = child[c];
                const uint4* vp = reinterpret_cast<const uint4*>(vdesc + 8 * (size_t)id);
                const uint4 a = vp[0], b = vp[1];
                o0 = coff[id];
                o1 = coff[id + 1];
                const int d = __popcll(f[0] ^ ((unsigned long long)a.x | ((unsigned long long)a.y << 32))) +
                              __popcll(f[1] ^ ((unsigned long long)a.z | ((unsigned long long)a.w << 32))) +
                              __popcll(f[2] ^ ((unsigned long long)b.x | ((unsigned long long)b.y << 32))) +
                              __popcll(f[3] ^ ((unsigned long long)b.z | ((unsigned long long)b.w << 32)));
                key = (d << 6) | j;   // d <= 256
            }
            int m = key;
            for (int o = G >> 1; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o));
            const int src = (lane & ~(G - 1)) | (m & 63);
            const int wid = __shfl(id, src), w0 = __shfl(o0, src), w1 = __shfl(o1, src);
            if ((m >> 6) < best_d) { best_d = m >> 6; best = wid; b0 = w0; b1 = w1; }
        }
        fin = best;
        c0 = b0;
        c1 = b1;
        if (level == nid_level) nid = fin;
    }
    if (j == 0) {
        o_leaf[(size_t)img * cap + i] = (uint32_t)fin;
        o_nid[(size_t)img * cap + i] = (uint32_t)nid;
    }
}

// Thread t owns the sorted keys [t R, t R + R). Returns the rank of its first run head (a key whose
// high word differs from its predecessor's) and the number of heads in all m keys. Every thread calls.
__device__ int bowb_head_scan(const unsigned long long* a, int m, int R, int* s_w, int& total) {
    const int j0 = threadIdx.x * R, j1 = min(m, j0 + R);
    int c = 0;
    for (int j = j0; j < j1; j++) c += (j == 0 || (uint32_t)(a[j - 1] >> 32) != (uint32_t)(a[j] >> 32)) ? 1 : 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = c;
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) s_w[wave] = x;
    SYNC();
    int base = 0, tot = 0;
    for (int w = 0; w < BB_ANT / 64; w++) {
        const int v = s_w[w];
        if (w < wave) base += v;
        tot += v;
    }
    SYNC();   // s_w may be written again
    total = tot;
    return base + x - c;
}

// keys (hi << 32 | feature) of the kept features (leaf weight > 0) into s_a, any order; returns their count
__device__ int bowb_compact(unsigned long long* s_a, int* s_cnt, int n, const uint32_t* leaf_row, const uint32_t* nid_row,
                            const int* __restrict__ vword, const double* __restrict__ vweight) {
    if (threadIdx.x == 0) *s_cnt = 0;
    SYNC();
    const int lane = threadIdx.x & 63;
    for (int base = 0; base < n; base += BB_ANT) {   // uniform trip count: the ballot sees whole waves
        const int i = base + threadIdx.x;
        bool keep = false;
        unsigned long long key = 0;
        if (i < n) {
            const uint32_t leaf = leaf_row[i];
            if (vweight[leaf] > 0) {
                keep = true;
                const uint32_t hi = nid_row ? nid_row[i] : (uint32_t)vword[leaf];
                key = ((unsigned long long)hi << 32) | (uint32_t)i;
            }
        }
        const unsigned long long mask = __ballot(keep);
        int wb = 0;
        if (lane == 0 && mask) wb = atomicAdd(s_cnt, (int)__popcll(mask));
        wb = __shfl(wb, 0);
        if (keep) s_a[wb + (int)__popcll(mask & ((1ull << lane) - 1ull))] = key;
    }
    SYNC();
    return *s_cnt;
}

__global__ __launch_bounds__(BB_ANT) void k_bowb_assemble(const int* __restrict__ vword, const double* __restrict__ vweight,
                                                          const int* __restrict__ counts_in, int count_stride, int cap,
                                                          int pcap, int weighting, int must, int norm_l1, int empty,
                                                          uint32_t* bow_ids, double* bow_w, uint32_t* fv_ids, int* fv_off,
                                                          uint32_t* fv_idx, int* counts_out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t bb_sm[];
    unsigned long long* s_a = reinterpret_cast<unsigned long long*>(bb_sm);
    int* s_i = reinterpret_cast<int*>(bb_sm + (size_t)pcap * 8);
    double* s_norm = reinterpret_cast<double*>(bb_sm + (size_t)pcap * 8 + 128);
    const int img = blockIdx.x;
    int* cnt = counts_out + 2 * (size_t)img;
    if (empty) {   // TemplatedVocabulary::empty(): v and fv cleared
        if (threadIdx.x == 0) cnt[0] = cnt[1] = 0;
        return;
    }
    const int n = counts_in[(size_t)img * count_stride];
    if (n < 0 || n > cap) {   // nothing else of this image is read or written
        if (threadIdx.x == 0) cnt[0] = cnt[1] = -1;
        return;
    }
    uint32_t* bid = bow_ids + (size_t)img * cap;
    double* bw = bow_w + (size_t)img * cap;
    uint32_t* fid = fv_ids + (size_t)img * cap;      // k_bowb_descend left the node at L - levelsup here
    uint32_t* fidx = fv_idx + (size_t)img * cap;     // and the leaf node here
    int* foff = fv_off + (size_t)img * ((size_t)cap + 1);
    const int lane = threadIdx.x & 63;

    // ---- BowVector ----
    const int m = bowb_compact(s_a, s_i, n, fidx, nullptr, vword, vweight);
    bow_sort_u64(s_a, m);
    const int R = (m + BB_ANT - 1) / BB_ANT;
    int nb = 0;
    int rank = bowb_head_scan(s_a, m, R, s_i + 1, nb);
    const bool tf = weighting == ORBFE_TF_IDF || weighting == ORBFE_TF;
    {
        const double nd = (double)nb;
        const int j0 = threadIdx.x * R, j1 = min(m, j0 + R);
        for (int j = j0; j < j1; j++) {
            const uint32_t w = (uint32_t)(s_a[j] >> 32);
            if (j > 0 && (uint32_t)(s_a[j - 1] >> 32) == w) continue;
            // this lane owns the whole run: key order within a word is feature order
            double sum = vweight[fidx[(uint32_t)(s_a[j] & 0xffffffffu)]];
            if (tf) {
                for (int q = j + 1; q < m && (uint32_t)(s_a[q] >> 32) == w; q++)
                    sum += vweight[fidx[(uint32_t)(s_a[q] & 0xffffffffu)]];   // addWeight
                if (!must) sum /= nd;
            }                                                                  // else addIfNotExist keeps the first
            bid[rank] = w;
            bw[rank] = sum;
            rank++;
        }
    }
    if (must) {   // BowVector::normalize: the norm is one chain in ascending word order
        SYNC();   // the sums are visible to wave 0
        if (threadIdx.x < 64) {
            double norm = 0.0;
            double cur = lane < nb ? bw[lane] : 0.0;
            for (int base = 0; base < nb; base += 64) {
                const double nxt = base + 64 + lane < nb ? bw[base + 64 + lane] : 0.0;   // in flight during the chain
                const double term = norm_l1 ? fabs(cur) : cur * cur;
                const int t_lo = __double2loint(term), t_hi = __double2hiint(term);
                const int cn = min(64, nb - base);
                for (int l = 0; l < cn; l++)
                    norm += __hiloint2double(__builtin_amdgcn_readlane(t_hi, l), __builtin_amdgcn_readlane(t_lo, l));
                cur = nxt;
            }
            if (!norm_l1) norm = sqrt(norm);
            if (lane == 0) *s_norm = norm;
        }
        SYNC();
        const double norm = *s_norm;
        if (norm > 0.0)
            for (int j = threadIdx.x; j < nb; j += BB_ANT) bw[j] /= norm;
    }

    // ---- FeatureVector ---- (bowb_compact's first barrier ends every read of the word keys)
    const int m2 = bowb_compact(s_a, s_i, n, fidx, fid, vword, vweight);
    // from here the leaf / node rows are outputs: every read of them is behind the barrier above
    bow_sort_u64(s_a, m2);
    for (int j = threadIdx.x; j < m2; j += BB_ANT) fidx[j] = (uint32_t)(s_a[j] & 0xffffffffu);
    int nf = 0;
    rank = bowb_head_scan(s_a, m2, R, s_i + 1, nf);
    {
        const int j0 = threadIdx.x * R, j1 = min(m2, j0 + R);
        for (int j = j0; j < j1; j++) {
            const uint32_t nd = (uint32_t)(s_a[j] >> 32);
            if (j > 0 && (uint32_t)(s_a[j - 1] >> 32) == nd) continue;
            fid[rank] = nd;
            foff[rank] = j;
            rank++;
        }
    }
    if (threadIdx.x == 0) {
        foff[nf] = m2;
        cnt[0] = nb;
        cnt[1] = nf;
    }
}

namespace {

// both launches on s; arguments validated by the caller, the vocabulary's device is current
int bowb_launch(const orbfe_vocabulary* voc, const uint8_t* d_desc, const int32_t* d_counts, int count_stride, int nimg,
                int cap, int levelsup, const orbfe_bow_batch* out, hipStream_t s) {
    int pcap = 1;
    while (pcap < cap) pcap <<= 1;
    const size_t lds = (size_t)pcap * 8 + BB_LDS_TAIL;
    MSCHK(ms_lds_optin<k_bowb_assemble>(voc->device, lds, BB_MAXN * 8 + BB_LDS_TAIL));
    const int empty = voc->n_words == 0 ? 1 : 0;
    int must = 1, norm_l1 = 1;   // ScoringObject.h:74-89
    if (voc->scoring == ORBFE_L2_NORM) norm_l1 = 0;
    if (voc->scoring == ORBFE_DOT_PRODUCT) must = 0;
    if (!empty) {
        int gshift = 2;
        while ((1 << gshift) < voc->k && gshift < 6) gshift++;
        const int per_block = BB_DNT >> gshift;
        hipLaunchKernelGGL(k_bowb_descend, dim3((unsigned)nimg, (unsigned)((cap + per_block - 1) / per_block)),
                           dim3(BB_DNT), 0, s, voc->d_desc, voc->d_child_off, voc->d_child, d_desc, d_counts,
                           count_stride, cap, voc->L - levelsup, gshift, out->fv_indices, out->fv_node_ids);
    }
    hipLaunchKernelGGL(k_bowb_assemble, dim3((unsigned)nimg), dim3(BB_ANT), lds, s, voc->d_word, voc->d_weight, d_counts,
                       count_stride, cap, pcap, voc->weighting, must, norm_l1, empty, out->bow_word_ids,
                       out->bow_weights, out->fv_node_ids, out->fv_offsets, out->fv_indices, out->counts);
    HIPCHK(hipGetLastError());
    return ORBFE_OK;
}

bool bowb_batch_ok(const orbfe_bow_batch* b) {
    return b && b->bow_word_ids && b->bow_weights && b->fv_node_ids && b->fv_offsets && b->fv_indices && b->counts &&
           !(((uintptr_t)b->bow_word_ids | (uintptr_t)b->fv_node_ids | (uintptr_t)b->fv_offsets |
              (uintptr_t)b->fv_indices | (uintptr_t)b->counts) & 3) && !((uintptr_t)b->bow_weights & 7);
}

// orbfe_frame_compute_bow's pinned read-back block, one per thread (never freed, as MatchScratch)
struct BowHost {
    int device = -1;
    uint8_t* h = nullptr;
    size_t cap = 0;
};
thread_local BowHost t_bowh;

}  // namespace

extern "C" {

int orbfe_vocabulary_transform_batch(const orbfe_vocabulary* voc, const uint8_t* d_desc, const int32_t* d_counts,
                                     int32_t count_stride, int32_t nimg, int32_t cap, int32_t levelsup,
                                     const orbfe_bow_batch* out, void* stream) {
    if (!voc || !d_desc || !d_counts || nimg < 0 || cap <= 0 || count_stride < 1 || !bowb_batch_ok(out) ||
        (((uintptr_t)d_desc | (uintptr_t)d_counts) & 3))
        return ORBFE_E_ARG;
    if (cap > BB_MAXN) return ORBFE_E_CAPACITY;
    if (nimg == 0) return ORBFE_OK;
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    if (dev != voc->device) return ORBFE_E_ARG;
    return bowb_launch(voc, d_desc, d_counts, count_stride, nimg, cap, levelsup, out, (hipStream_t)stream);
}

int orbfe_frame_compute_bow(const orbfe_vocabulary* voc, const orbfe_frame* F, int32_t levelsup,
                            uint32_t* bow_word_ids, double* bow_weights, int32_t* bow_n,
                            uint32_t* fv_node_ids, int32_t* fv_offsets, uint32_t* fv_indices, int32_t* fv_n) {
    if (!voc || !F || F->n < 0 ||
        (F->n > 0 && (!F->desc || !bow_word_ids || !bow_weights || !fv_node_ids || !fv_indices)) || !bow_n || !fv_n ||
        !fv_offsets)
        return ORBFE_E_ARG;
    const int n = F->n;
    if (voc->n_words != 0 && n > BB_MAXN) return ORBFE_E_CAPACITY;   // refused before any output is written
    *bow_n = 0;
    *fv_n = 0;
    fv_offsets[0] = 0;
    if (voc->n_words == 0 || n == 0) return ORBFE_OK;   // empty(): v and fv cleared
    if (F->device && ((uintptr_t)F->desc & 3)) return ORBFE_E_ARG;
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    if (dev != voc->device) return ORBFE_E_ARG;
    Plan p;
    const size_t o_d = F->device ? 0 : p.upload(F->desc, (size_t)n * 32);
    const size_t o_n = p.upload(&n, 4);
    // one block for everything that goes back: [counts | bow ids | fv ids | fv offsets | fv indices | bow weights]
    const size_t b_bid = 16, b_fid = b_bid + (size_t)n * 4, b_foff = b_fid + (size_t)n * 4;
    const size_t b_fidx = b_foff + ((size_t)n + 1) * 4, b_bw = (b_fidx + (size_t)n * 4 + 7) & ~(size_t)7;
    const size_t bytes = b_bw + (size_t)n * 8;
    const size_t o_blk = p.scratch(bytes);
    MSCHK(ms_prepare(p));
    BowHost& bh = t_bowh;
    if (bh.device != dev || bh.cap < bytes) {
        if (bh.h && bh.device == dev) HIPCHK(hipHostFree(bh.h));
        bh = BowHost();
        const size_t hc = std::max<size_t>(bytes + bytes / 2, 64 * 1024);
        HIPCHK(hipHostMalloc((void**)&bh.h, hc, hipHostMallocDefault));
        bh.device = dev;
        bh.cap = hc;
    }
    hipStream_t s = t_ms.stream;
    uint8_t* blk = ms_ptr<uint8_t>(o_blk);
    orbfe_bow_batch ob;
    ob.counts = reinterpret_cast<int32_t*>(blk);
    ob.bow_word_ids = reinterpret_cast<uint32_t*>(blk + b_bid);
    ob.fv_node_ids = reinterpret_cast<uint32_t*>(blk + b_fid);
    ob.fv_offsets = reinterpret_cast<int32_t*>(blk + b_foff);
    ob.fv_indices = reinterpret_cast<uint32_t*>(blk + b_fidx);
    ob.bow_weights = reinterpret_cast<double*>(blk + b_bw);
    {
        MsTimer timer;
        MSCHK(bowb_launch(voc, F->device ? F->desc : ms_ptr<const uint8_t>(o_d), ms_ptr<const int32_t>(o_n), 1, 1, n,
                          levelsup, &ob, s));
        timer.end();
        // the one host wait: the whole block, not counts and then payload
        HIPCHK(hipMemcpyAsync(bh.h, blk, bytes, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    int cnt[2];
    memcpy(cnt, bh.h, 8);
    const int nb = cnt[0], nf = cnt[1];
    if (nb < 0 || nb > n || nf < 0 || nf > n) return ORBFE_E_DEVICE;
    memcpy(bow_word_ids, bh.h + b_bid, (size_t)nb * 4);
    memcpy(bow_weights, bh.h + b_bw, (size_t)nb * 8);
    memcpy(fv_node_ids, bh.h + b_fid, (size_t)nf * 4);
    memcpy(fv_offsets, bh.h + b_foff, ((size_t)nf + 1) * 4);
    const int nidx = fv_offsets[nf];
    if (nidx < 0 || nidx > n) return ORBFE_E_DEVICE;
    memcpy(fv_indices, bh.h + b_fidx, (size_t)nidx * 4);
    *bow_n = nb;
    *fv_n = nf;
    return ORBFE_OK;
}

int orbfe_kfdb_add_batch(orbfe_kfdb* db, const orbfe_vocabulary* voc, const int32_t* kf_ids,
                         const orbfe_bow_batch* bows, int32_t nimg, int32_t cap, void* stream) {
    if (!db || !voc || !kf_ids || !bows || !bows->bow_word_ids || !bows->bow_weights || !bows->counts || nimg < 0 ||
        cap <= 0)
        return ORBFE_E_ARG;
    bool any = false;
    {
        std::vector<int32_t> ids;
        for (int i = 0; i < nimg; i++)
            if (kf_ids[i] >= 0) ids.push_back(kf_ids[i]);
        std::sort(ids.begin(), ids.end());
        if (std::adjacent_find(ids.begin(), ids.end()) != ids.end()) return ORBFE_E_ARG;
        any = !ids.empty();
    }
    if (voc->n_words != db->n_words) return ORBFE_E_ARG;
    if ((size_t)nimg * (size_t)cap > (size_t)0x7fffffff) return ORBFE_E_CAPACITY;   // k_kfdb_move's int offsets
    if (!any) return ORBFE_OK;
    std::lock_guard<std::mutex> lock(db->mu);
    size_t n_add = 0;
    for (int i = 0; i < nimg; i++) {
        if (kf_ids[i] < 0) continue;
        if (db->index.count(kf_ids[i])) return ORBFE_E_ARG;
        n_add++;
    }
    if (db->ent.size() + n_add > ((size_t)1 << 30)) return ORBFE_E_CAPACITY;
    MSCHK(kfdb_device(db));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));   // the batch is complete
    std::vector<int32_t> cnt((size_t)nimg * 2);
    HIPCHK(hipMemcpy(cnt.data(), bows->counts, cnt.size() * 4, hipMemcpyDeviceToHost));
    size_t total = 0;
    for (int i = 0; i < nimg; i++) {
        if (kf_ids[i] < 0) continue;
        const int c = cnt[2 * (size_t)i];
        if (c < 0 || c > cap) return ORBFE_E_ARG;   // {-1, -1}: that image's input count was bad
        total += (size_t)c;
    }
    if (db->used_words + total > db->cap_words) {
        // room first from the tombstones, then from a larger arena: once for the whole batch
        const size_t live = db->used_words - db->dead_words;
        MSCHK(kfdb_rebuild(db, kfdb_cap_for(live + total)));
    }
    std::vector<int4> moves;
    size_t at = db->used_words;
    for (int i = 0; i < nimg; i++) {
        const int c = kf_ids[i] < 0 ? 0 : cnt[2 * (size_t)i];
        if (c > 0) moves.push_back(make_int4((int)((size_t)i * cap), (int)at, c, 0));
        at += (size_t)c;
    }
    if (!moves.empty()) {
        int4* d_moves = nullptr;
        HIPCHK(hipMalloc((void**)&d_moves, moves.size() * sizeof(int4)));
        struct G2 { void* p; ~G2() { (void)hipFree(p); } } g2{d_moves};
        HIPCHK(hipMemcpyAsync(d_moves, moves.data(), moves.size() * sizeof(int4), hipMemcpyHostToDevice, db->stream));
        hipLaunchKernelGGL(k_kfdb_move, dim3((unsigned)moves.size()), dim3(KFDB_MOVE_NT), 0, db->stream,
                           bows->bow_word_ids, bows->bow_weights, db->d_ids, db->d_w, d_moves);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(db->stream));   // the batch's arrays are free on return
    }
    const size_t first = db->ent.size();
    at = db->used_words;
    for (int i = 0; i < nimg; i++) {
        if (kf_ids[i] < 0) continue;
        const int c = cnt[2 * (size_t)i];
        db->index[kf_ids[i]] = (int)db->ent.size();
        db->ent.push_back(orbfe_kfdb::Entry{kf_ids[i], 0.f, true});
        db->h_ent.push_back(make_int2((int)at, c));
        at += (size_t)c;
    }
    db->used_words = at;
    kfdb_mark_dirty(db, first, db->ent.size());
    if (total > 0) MSCHK(kfdb_flush_entries(db));   // entries of empty BowVectors wait for the next device call
    return ORBFE_OK;
}

}  // extern "C"
