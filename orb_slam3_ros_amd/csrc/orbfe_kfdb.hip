// KeyFrameDatabase for relocalisation on CDNA4 (included into orbfe_engine.hip after orbfe_bow.hip;
// the matcher provides MsTimer): KeyFrameDatabase::add / erase / clear (KeyFrameDatabase.cc:39-77)
// and DetectRelocalizationCandidates (:733-845) with L1Scoring::score (ScoringObject.cpp:23-68).
//
// Storage: every added keyframe's BowVector sits in one growing HBM arena as CSR, word ids (u32) and
// weights (f64) in separate arrays, with a device table of (offset, length) per entry. The table is
// append-only and compaction keeps its order, so an entry's position IS its add sequence: erase then
// add moves a keyframe to the back, as the inverted file's push_back does. Ids and reloc_score stay
// beside the table on the host, where the gate and the covisibility tail read them.
//
// k_kfdb_query: one wave per keyframe in single-wave workgroups, each striding over the table
// (uneven lengths: no wave waits for another's longest keyframe, and a finished wave gives its LDS
// back at once). Lanes take 64 consecutive keyframe words, binary-search the query's ascending ids
// (staged in LDS when they fit), ballot gives the shared count and the first shared word; the matched terms
// fabs(vi - wi) - fabs(vi) - fabs(wi) are then added in lane (= word) order into ONE double chain,
// as the reference's merge loop adds them. No tree, no atomics on the sum.
#pragma once

#include <memory>
#include <unordered_map>

#define KFDB_NT 64                   // k_kfdb_query: one wave per workgroup
#define KFDB_MOVE_NT 256
#define KFDB_LDS_WORDS 4096          // query words staged in LDS (12 B each: 48 KB of a CU's 160 KB, under the 64 KB a launch gets by default)
#define KFDB_INIT_WORDS (1u << 15)   // initial arena capacity
#define KFDB_MAX_WORDS (1u << 30)

template <bool LDSQ>
__global__ __launch_bounds__(KFDB_NT) void k_kfdb_query(const uint32_t* __restrict__ a_ids,
                                                        const double* __restrict__ a_w, const int2* __restrict__ ent,
                                                        int n_ent, const double* __restrict__ q_w,
                                                        const uint32_t* __restrict__ q_ids, int qn, int4* out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t kfdb_sm[];
    double* s_w = reinterpret_cast<double*>(kfdb_sm);
    uint32_t* s_ids = reinterpret_cast<uint32_t*>(kfdb_sm + (size_t)qn * 8);
    if constexpr (LDSQ) {
        for (int i = threadIdx.x; i < qn; i += KFDB_NT) {
            s_w[i] = q_w[i];
            s_ids[i] = q_ids[i];
        }
        SYNC();   // one wave: orders its own LDS writes before the reads below
    }
    const int lane = threadIdx.x;
    // e depends on the block index alone, so the loop's trip count is the same for all 64 lanes
    for (int e = blockIdx.x; e < n_ent; e += gridDim.x) {
        const int2 en = ent[e];   // (offset, length); length 0: a tombstone or an empty BowVector
        int count = 0, first = -1;
        double sum = 0.0;   // L1Scoring::score's `double score = 0`
        for (int base = 0; base < en.y; base += 64) {
            const int k = base + lane;
            int j = -1;
            double term = 0.0;
            if (k < en.y) {
                const uint32_t w = a_ids[(size_t)en.x + k];
                int lo = 0, hi = qn;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    const uint32_t q = LDSQ ? s_ids[mid] : q_ids[mid];
                    if (q < w) lo = mid + 1; else hi = mid;
                }
                if (lo < qn && (LDSQ ? s_ids[lo] : q_ids[lo]) == w) {
                    j = lo;
                    const double vi = LDSQ ? s_w[lo] : q_w[lo];   // v1 = F.mBowVec
                    const double wi = a_w[(size_t)en.x + k];       // v2 = KF.mBowVec
                    term = fabs(vi - wi) - fabs(vi) - fabs(wi);
                }
            }
            unsigned long long m = __ballot(j >= 0);   // uniform: the reads below name their lane from it
            if (m) {
                if (first < 0) first = __builtin_amdgcn_readlane(j, (int)__builtin_ctzll(m));
                count += (int)__popcll(m);
                // ascending lanes are ascending word ids: one left-to-right chain, the same in every lane
                const int t_lo = __double2loint(term), t_hi = __double2hiint(term);
                for (; m; m &= m - 1) {
                    const int l = (int)__builtin_ctzll(m);
                    sum += __hiloint2double(__builtin_amdgcn_readlane(t_hi, l), __builtin_amdgcn_readlane(t_lo, l));
                }
            }
        }
        if (lane == 0) out[e] = make_int4(count, first, __float_as_int((float)(-sum / 2.0)), 0);
    }
}

// compaction / growth into a fresh arena: block b copies move b = (src offset, dst offset, length)
__global__ __launch_bounds__(KFDB_MOVE_NT) void k_kfdb_move(const uint32_t* __restrict__ s_ids, const double* __restrict__ s_w,
                                                       uint32_t* __restrict__ d_ids, double* __restrict__ d_w,
                                                       const int4* __restrict__ moves) {
    const int4 mv = moves[blockIdx.x];
    for (int i = threadIdx.x; i < mv.z; i += KFDB_MOVE_NT) {
        d_ids[(size_t)mv.y + i] = s_ids[(size_t)mv.x + i];
        d_w[(size_t)mv.y + i] = s_w[(size_t)mv.x + i];
    }
}

struct orbfe_kfdb {
    std::mutex mu;   // KeyFrameDatabase::mMutex
    int n_words = 0;
    int device = -1;   // the device current at create (-1: none was visible)
    hipStream_t stream = nullptr;
    int n_cu = 0;
    // arena
    uint32_t* d_ids = nullptr;
    double* d_w = nullptr;
    size_t cap_words = 0, used_words = 0, dead_words = 0;
    // entry table: host mirror, its device copy and the mirror's range not uploaded yet
    struct Entry {
        int32_t id;
        float reloc_score;   // KeyFrame::mRelocScore
        bool live;
        float place_score = 0.f;   // KeyFrame::mPlaceRecognitionScore (orbfe_kfdb_detect_nbest; apart from reloc_score)
    };
    std::vector<Entry> ent;
    std::vector<int2> h_ent;
    int2* d_ent = nullptr;
    size_t cap_ent = 0;
    size_t dirty_lo = 0, dirty_hi = 0;
    std::unordered_map<int32_t, int> index;   // live kf id -> entry
    // query staging (pinned) and its device copy: [weights | ids]
    uint8_t* h_q = nullptr;
    uint8_t* d_q = nullptr;
    size_t qcap = 0;
    // results: mapped pinned, one int4 per entry
    int4* h_out = nullptr;
    int4* h_out_dev = nullptr;
    size_t ocap = 0;
};

namespace {

bool kfdb_ascending(const uint32_t* ids, int n, int n_words) {
    for (int i = 0; i < n; i++)
        if (ids[i] >= (uint32_t)n_words || (i > 0 && ids[i] <= ids[i - 1])) return false;
    return true;
}

// the handle's device is current and its stream exists
int kfdb_device(orbfe_kfdb* db) {
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    if (db->device < 0) return ORBFE_E_DEVICE;
    if (dev != db->device) return ORBFE_E_ARG;   // a handle belongs to its create's device
    if (!db->stream) {
        HIPCHK(hipDeviceGetAttribute(&db->n_cu, hipDeviceAttributeMultiprocessorCount, dev));
        HIPCHK(hipStreamCreateWithFlags(&db->stream, hipStreamNonBlocking));
    }
    return ORBFE_OK;
}

void kfdb_mark_dirty(orbfe_kfdb* db, size_t lo, size_t hi) {
    if (db->dirty_lo == db->dirty_hi) { db->dirty_lo = lo; db->dirty_hi = hi; return; }
    db->dirty_lo = std::min(db->dirty_lo, lo);
    db->dirty_hi = std::max(db->dirty_hi, hi);
}

// upload the entry table's changed range (queued on the handle's stream)
int kfdb_flush_entries(orbfe_kfdb* db) {
    const size_t n = db->h_ent.size();
    if (n > db->cap_ent) {
        const size_t cap = std::max<size_t>(n + n / 2, 1024);
        int2* d = nullptr;
        HIPCHK(hipMalloc((void**)&d, cap * sizeof(int2)));
        HIPCHK(hipStreamSynchronize(db->stream));
        if (db->d_ent) HIPCHK(hipFree(db->d_ent));
        db->d_ent = d;
        db->cap_ent = cap;
        db->dirty_lo = 0;
        db->dirty_hi = n;
    }
    db->dirty_hi = std::min(db->dirty_hi, n);
    if (db->dirty_lo < db->dirty_hi) {
        HIPCHK(hipMemcpyAsync(db->d_ent + db->dirty_lo, db->h_ent.data() + db->dirty_lo,
                              (db->dirty_hi - db->dirty_lo) * sizeof(int2), hipMemcpyHostToDevice, db->stream));
        HIPCHK(hipStreamSynchronize(db->stream));   // h_ent may change as soon as the caller returns
    }
    db->dirty_lo = db->dirty_hi = 0;
    return ORBFE_OK;
}

// A fresh arena of `cap` words holding the live entries in table order (device to device); the
// tombstones leave the table. With no tombstone this is plain growth: one copy of the used range.
int kfdb_rebuild(orbfe_kfdb* db, size_t cap) {
    const size_t live = db->used_words - db->dead_words;
    if (cap < live || cap > KFDB_MAX_WORDS) return ORBFE_E_CAPACITY;
    uint32_t* n_ids = nullptr;
    double* n_w = nullptr;
    HIPCHK(hipMalloc((void**)&n_ids, std::max<size_t>(cap, 4) * 4));
    struct Guard {
        void* a;
        void* b;
        ~Guard() { if (a) (void)hipFree(a); if (b) (void)hipFree(b); }
    } guard{n_ids, nullptr};
    HIPCHK(hipMalloc((void**)&n_w, std::max<size_t>(cap, 4) * 8));
    guard.b = n_w;
    std::vector<orbfe_kfdb::Entry> ent;
    std::vector<int2> h_ent;
    bool dead = false;
    for (const auto& e : db->ent) dead = dead || !e.live;
    if (!dead) {
        if (db->used_words) {
            HIPCHK(hipMemcpyAsync(n_ids, db->d_ids, db->used_words * 4, hipMemcpyDeviceToDevice, db->stream));
            HIPCHK(hipMemcpyAsync(n_w, db->d_w, db->used_words * 8, hipMemcpyDeviceToDevice, db->stream));
            HIPCHK(hipStreamSynchronize(db->stream));
        }
    } else {
        std::vector<int4> moves;
        size_t at = 0;
        for (size_t i = 0; i < db->ent.size(); i++) {
            if (!db->ent[i].live) continue;
            const int2 o = db->h_ent[i];
            ent.push_back(db->ent[i]);
            h_ent.push_back(make_int2((int)at, o.y));
            if (o.y > 0) moves.push_back(make_int4(o.x, (int)at, o.y, 0));
            at += (size_t)o.y;
        }
        if (at != live) return ORBFE_E_DEVICE;   // the host mirror disagrees with itself: move nothing
        if (!moves.empty()) {
            int4* d_moves = nullptr;
            HIPCHK(hipMalloc((void**)&d_moves, moves.size() * sizeof(int4)));
            struct G2 { void* p; ~G2() { (void)hipFree(p); } } g2{d_moves};
            HIPCHK(hipMemcpyAsync(d_moves, moves.data(), moves.size() * sizeof(int4), hipMemcpyHostToDevice, db->stream));
            hipLaunchKernelGGL(k_kfdb_move, dim3((unsigned)moves.size()), dim3(KFDB_MOVE_NT), 0, db->stream, db->d_ids,
                               db->d_w, n_ids, n_w, d_moves);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(db->stream));
        }
        db->ent.swap(ent);
        db->h_ent.swap(h_ent);
        db->index.clear();
        for (size_t i = 0; i < db->ent.size(); i++) db->index[db->ent[i].id] = (int)i;
        db->used_words = live;
        db->dead_words = 0;
        db->dirty_lo = 0;
        db->dirty_hi = db->h_ent.size();
    }
    if (db->d_ids) HIPCHK(hipFree(db->d_ids));
    if (db->d_w) HIPCHK(hipFree(db->d_w));
    db->d_ids = n_ids;
    db->d_w = n_w;
    db->cap_words = cap;
    guard.a = guard.b = nullptr;
    return ORBFE_OK;
}

size_t kfdb_cap_for(size_t words) {
    size_t cap = KFDB_INIT_WORDS;
    while (cap < words) cap *= 2;
    return cap;
}

struct KfdbQuery {
    std::vector<int> list;         // lKFsSharingWords as entry indices, in the reference's list order
    std::vector<int> words;        // mnRelocWords per list element
    std::vector<float> score;      // si per list element (every sharing keyframe is scored on the device)
    std::vector<uint8_t> shares;   // per entry: mnRelocQuery == F->mnId
    int max_common = 0, min_common = 0;
};

// stage 1+2 (:735-787) for the locked handle; writes no state
int kfdb_query(orbfe_kfdb* db, const uint32_t* f_ids, const double* f_w, int f_n, KfdbQuery& q) {
    q.max_common = q.min_common = 0;
    if (f_n == 0 || db->used_words == db->dead_words) return ORBFE_OK;
    MSCHK(kfdb_device(db));
    MSCHK(kfdb_flush_entries(db));
    const size_t n_ent = db->h_ent.size();
    const size_t qbytes = (size_t)f_n * 12;
    if (qbytes > db->qcap) {
        if (db->h_q) HIPCHK(hipHostFree(db->h_q));
        db->h_q = nullptr;
        if (db->d_q) HIPCHK(hipFree(db->d_q));
        db->d_q = nullptr;
        db->qcap = 0;
        const size_t cap = std::max<size_t>(qbytes + qbytes / 2, 64 * 1024);
        HIPCHK(hipHostMalloc((void**)&db->h_q, cap, hipHostMallocDefault));
        HIPCHK(hipMalloc((void**)&db->d_q, cap));
        db->qcap = cap;
    }
    if (n_ent > db->ocap) {
        if (db->h_out) HIPCHK(hipHostFree(db->h_out));
        db->h_out = nullptr;
        db->ocap = 0;
        const size_t cap = std::max<size_t>(n_ent + n_ent / 2, 1024);
        HIPCHK(hipHostMalloc((void**)&db->h_out, cap * sizeof(int4), hipHostMallocMapped | hipHostMallocCoherent));
        HIPCHK(hipHostGetDevicePointer((void**)&db->h_out_dev, db->h_out, 0));
        db->ocap = cap;
    }
    hipStream_t s = db->stream;
    memcpy(db->h_q, f_w, (size_t)f_n * 8);
    memcpy(db->h_q + (size_t)f_n * 8, f_ids, (size_t)f_n * 4);
    HIPCHK(hipMemcpyAsync(db->d_q, db->h_q, qbytes, hipMemcpyHostToDevice, s));
    {
        MsTimer timer(s);
        const int blocks = (int)std::min<size_t>(n_ent, (size_t)std::max(db->n_cu, 1) * 8);
        const double* q_w = (const double*)db->d_q;
        const uint32_t* q_ids = (const uint32_t*)(db->d_q + (size_t)f_n * 8);
        if (f_n <= KFDB_LDS_WORDS)
            hipLaunchKernelGGL(k_kfdb_query<true>, dim3(blocks), dim3(KFDB_NT), (qbytes + 15) & ~(size_t)15, s, db->d_ids,
                               db->d_w, db->d_ent, (int)n_ent, q_w, q_ids, f_n, db->h_out_dev);
        else
            hipLaunchKernelGGL(k_kfdb_query<false>, dim3(blocks), dim3(KFDB_NT), 0, s, db->d_ids, db->d_w, db->d_ent,
                               (int)n_ent, q_w, q_ids, f_n, db->h_out_dev);
        HIPCHK(hipGetLastError());
        timer.end();
        // the one host wait: every wave's store is visible in the mapped block once the stream has drained
        HIPCHK(hipStreamSynchronize(s));
    }
    // F's words ascending, each word's list in push_back order: a stable counting sort of the sharing
    // entries (table order = add sequence) by the query position of their first shared word
    const int4* out = db->h_out;
    std::vector<int> start((size_t)f_n + 1, 0);
    size_t nsh = 0;
    q.shares.assign(n_ent, 0);
    for (size_t e = 0; e < n_ent; e++) {
        if (out[e].x <= 0) continue;
        if (out[e].y < 0 || out[e].y >= f_n) return ORBFE_E_DEVICE;
        q.shares[e] = 1;
        start[out[e].y + 1]++;
        nsh++;
    }
    for (int i = 0; i < f_n; i++) start[i + 1] += start[i];
    q.list.assign(nsh, 0);
    for (size_t e = 0; e < n_ent; e++)
        if (q.shares[e]) q.list[start[out[e].y]++] = (int)e;
    q.words.resize(nsh);
    q.score.resize(nsh);
    for (size_t i = 0; i < nsh; i++) {
        const int4 o = out[q.list[i]];
        q.words[i] = o.x;
        memcpy(&q.score[i], &o.z, 4);
        if (o.x > q.max_common) q.max_common = o.x;
    }
    q.min_common = (int)(q.max_common * 0.8f);   // int minCommonWords = maxCommonWords*0.8f
    return ORBFE_OK;
}

bool kfdb_query_args(const orbfe_kfdb* db, const uint32_t* f_ids, const double* f_w, int f_n) {
    if (!db || f_n < 0 || (f_n > 0 && (!f_ids || !f_w))) return false;
    return kfdb_ascending(f_ids, f_n, db->n_words);
}

}  // namespace

extern "C" {

int orbfe_kfdb_create(int32_t n_words, orbfe_kfdb** out) {
    if (!out) return ORBFE_E_ARG;
    *out = nullptr;
    if (n_words <= 0) return ORBFE_E_ARG;
    orbfe_kfdb* db = new orbfe_kfdb();
    db->n_words = n_words;
    if (hipGetDevice(&db->device) != hipSuccess) db->device = -1;   // device calls will answer ORBFE_E_DEVICE
    *out = db;
    return ORBFE_OK;
}

void orbfe_kfdb_destroy(orbfe_kfdb* db) {
    if (!db) return;
    if (db->stream) (void)hipStreamSynchronize(db->stream);
    void* dev[] = {db->d_ids, db->d_w, db->d_ent, db->d_q};
    for (void* p : dev)
        if (p) (void)hipFree(p);
    if (db->h_q) (void)hipHostFree(db->h_q);
    if (db->h_out) (void)hipHostFree(db->h_out);
    if (db->stream) (void)hipStreamDestroy(db->stream);
    delete db;
}

int orbfe_kfdb_add(orbfe_kfdb* db, int32_t kf_id, const uint32_t* word_ids, const double* weights, int32_t n) {
    if (!db || kf_id < 0 || n < 0 || (n > 0 && (!word_ids || !weights))) return ORBFE_E_ARG;
    if (!kfdb_ascending(word_ids, n, db->n_words)) return ORBFE_E_ARG;
    std::lock_guard<std::mutex> lock(db->mu);
    if (db->index.count(kf_id)) return ORBFE_E_ARG;
    if (db->ent.size() >= ((size_t)1 << 30)) return ORBFE_E_CAPACITY;
    if (n > 0) {
        MSCHK(kfdb_device(db));
        if (db->used_words + (size_t)n > db->cap_words) {
            // room first from the tombstones, then from a larger arena
            const size_t live = db->used_words - db->dead_words;
            MSCHK(kfdb_rebuild(db, kfdb_cap_for(live + (size_t)n)));
        }
        HIPCHK(hipMemcpyAsync(db->d_ids + db->used_words, word_ids, (size_t)n * 4, hipMemcpyHostToDevice, db->stream));
        HIPCHK(hipMemcpyAsync(db->d_w + db->used_words, weights, (size_t)n * 8, hipMemcpyHostToDevice, db->stream));
        HIPCHK(hipStreamSynchronize(db->stream));   // the caller's arrays are free on return
    }
    const size_t idx = db->ent.size();
    db->ent.push_back(orbfe_kfdb::Entry{kf_id, 0.f, true});
    db->h_ent.push_back(make_int2((int)db->used_words, n));
    db->index[kf_id] = (int)idx;
    db->used_words += (size_t)n;
    kfdb_mark_dirty(db, idx, idx + 1);
    if (n > 0) MSCHK(kfdb_flush_entries(db));   // an empty BowVector's entry waits for the next device call
    return ORBFE_OK;
}

int orbfe_kfdb_erase(orbfe_kfdb* db, int32_t kf_id) {
    if (!db || kf_id < 0) return ORBFE_E_ARG;
    std::lock_guard<std::mutex> lock(db->mu);
    const auto it = db->index.find(kf_id);
    if (it == db->index.end()) return ORBFE_E_ARG;
    const size_t idx = (size_t)it->second;
    const int len = db->h_ent[idx].y;
    // the device check comes before any host state changes: a refused erase has erased nothing. A HIP
    // error after it is reported with the keyframe erased on the host; its tombstone stays in the
    // table's dirty range and reaches the device with the next call that flushes.
    if (len > 0) MSCHK(kfdb_device(db));
    db->index.erase(it);
    db->ent[idx].live = false;   // its reloc_score goes with it
    db->h_ent[idx].y = 0;
    db->dead_words += (size_t)len;
    kfdb_mark_dirty(db, idx, idx + 1);
    if (len > 0) {
        if (db->dead_words * 2 > db->used_words)
            MSCHK(kfdb_rebuild(db, kfdb_cap_for(db->used_words - db->dead_words)));
        MSCHK(kfdb_flush_entries(db));
    }
    return ORBFE_OK;
}

int orbfe_kfdb_clear(orbfe_kfdb* db) {
    if (!db) return ORBFE_E_ARG;
    std::lock_guard<std::mutex> lock(db->mu);
    db->ent.clear();
    db->h_ent.clear();
    db->index.clear();
    db->used_words = db->dead_words = 0;   // the arena keeps its capacity
    db->dirty_lo = db->dirty_hi = 0;
    return ORBFE_OK;
}

int orbfe_kfdb_size(const orbfe_kfdb* db) {
    if (!db) return ORBFE_E_ARG;
    std::lock_guard<std::mutex> lock(const_cast<orbfe_kfdb*>(db)->mu);
    return (int)db->index.size();
}

int orbfe_kfdb_shared_words(orbfe_kfdb* db, const uint32_t* f_word_ids, const double* f_weights, int32_t f_n,
                            int32_t* kf_ids, int32_t* words, float* scores, uint8_t* scored, int32_t cap,
                            int32_t* n_out, int32_t* max_common_words) {
    if (!n_out || !max_common_words || cap < 0 || (cap > 0 && (!kf_ids || !words || !scores || !scored)))
        return ORBFE_E_ARG;
    if (!kfdb_query_args(db, f_word_ids, f_weights, f_n)) return ORBFE_E_ARG;
    std::lock_guard<std::mutex> lock(db->mu);
    KfdbQuery q;
    MSCHK(kfdb_query(db, f_word_ids, f_weights, f_n, q));
    const size_t n = q.list.size();
    *n_out = (int32_t)n;
    if (n > (size_t)cap) return ORBFE_E_ARG;
    *max_common_words = q.max_common;
    for (size_t i = 0; i < n; i++) {
        orbfe_kfdb::Entry& e = db->ent[q.list[i]];
        const bool pass = q.words[i] > q.min_common;
        kf_ids[i] = e.id;
        words[i] = q.words[i];
        scored[i] = pass ? 1 : 0;
        scores[i] = pass ? q.score[i] : 0.f;
        if (pass) e.reloc_score = q.score[i];   // pKFi->mRelocScore = si
    }
    return ORBFE_OK;
}

int orbfe_kfdb_detect_reloc(orbfe_kfdb* db, const uint32_t* f_word_ids, const double* f_weights, int32_t f_n,
                            int32_t map_id, orbfe_kf_info_fn info, void* ctx, int32_t* out_ids, int32_t cap,
                            int32_t* n_out) {
    if (!n_out || cap < 0 || (cap > 0 && !out_ids)) return ORBFE_E_ARG;
    if (!kfdb_query_args(db, f_word_ids, f_weights, f_n)) return ORBFE_E_ARG;
    std::lock_guard<std::mutex> lock(db->mu);
    KfdbQuery q;
    MSCHK(kfdb_query(db, f_word_ids, f_weights, f_n, q));
    *n_out = 0;
    if (q.list.empty()) return ORBFE_OK;
    // this query's scores beside the stored ones; committed only when the call succeeds
    std::vector<float> rs(db->ent.size());
    for (size_t e = 0; e < db->ent.size(); e++) rs[e] = db->ent[e].reloc_score;
    std::vector<int> sc;   // lScoreAndMatch as positions in q.list
    for (size_t i = 0; i < q.list.size(); i++)
        if (q.words[i] > q.min_common) {
            rs[q.list[i]] = q.score[i];
            sc.push_back((int)i);
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
    // accumulate score by covisibility (:792-821)
    std::vector<std::pair<float, int>> acc;   // (accScore, pBestKF as an entry)
    float bestAccScore = 0;
    for (int i : sc) {
        const int ei = q.list[i];
        const Info& in = ask(db->ent[ei].id);
        float bestScore = q.score[i];
        float accScore = bestScore;
        int best = ei;
        for (int k = 0; k < in.n; k++) {
            const auto it = db->index.find(in.nb[k]);
            if (it == db->index.end() || !q.shares[it->second]) continue;   // mnRelocQuery != F->mnId
            const float s2 = rs[it->second];
            accScore += s2;
            if (s2 > bestScore) {
                best = it->second;
                bestScore = s2;
            }
        }
        acc.emplace_back(accScore, best);
        if (accScore > bestAccScore) bestAccScore = accScore;
    }
    // keep those above 0.75 * best, in this map, once each (:823-842)
    const float minScoreToRetain = 0.75f * bestAccScore;
    std::vector<int32_t> res;
    std::vector<uint8_t> added(db->ent.size(), 0);
    for (const auto& a : acc) {
        if (!(a.first > minScoreToRetain)) continue;
        const int32_t id = db->ent[a.second].id;
        if (ask(id).map != map_id) continue;
        if (!added[a.second]) {
            res.push_back(id);
            added[a.second] = 1;
        }
    }
    if (bad_info) return ORBFE_E_ARG;
    *n_out = (int32_t)res.size();
    if (res.size() > (size_t)cap) return ORBFE_E_ARG;
    for (int i : sc) db->ent[q.list[i]].reloc_score = q.score[i];
    if (!res.empty()) memcpy(out_ids, res.data(), res.size() * 4);
    return ORBFE_OK;
}

}  // extern "C"
