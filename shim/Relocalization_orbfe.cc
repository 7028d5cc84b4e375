// The first loop of Tracking::Relocalization (orb_slam3/src/Tracking.cc:3680-3692) on top of
// liborbfe.so: SearchByBoW of the current frame against every candidate keyframe in ONE device call
// (orbfe_search_by_bow_batch, one workgroup per candidate) instead of one call per candidate. A
// keyframe's mvKeysUn angles, mDescriptors and mFeatVec never change after its construction, so they
// are copied into HBM once (orbfe_keyframe_create, on the keyframe's first use as a candidate) and
// kept in a cache keyed by KeyFrame*; per call only the candidates' map-point slots cross the link.
// On a negative return the loop runs per candidate through ORBmatcher::SearchByBoW (which itself
// falls back to the CPU body), so a failure never reaches Tracking.
// Built inside the ORB-SLAM3 tree; this repository compiles it with -fsyntax-only against stand-in
// headers (tests/shim_stubs/, tests/test_shim_compile.py). See INTEGRATION.md.
#include "Relocalization_orbfe.h"

#include <cstdio>
#include <cstring>
#include <mutex>
#include <unordered_map>

#include <orbfe.h>

#include "orbfe_glue.h"

#include "Frame.h"
#include "KeyFrame.h"
#include "MapPoint.h"
#include "ORBextractor.h"
#include "ORBmatcher.h"

using namespace std;

namespace ORB_SLAM3 {

namespace {

void flatten(const DBoW2::FeatureVector& fv, vector<uint32_t>& ids, vector<int32_t>& off, vector<uint32_t>& idx) {
    off.push_back(0);
    for (const auto& kv : fv) {
        ids.push_back(kv.first);
        idx.insert(idx.end(), kv.second.begin(), kv.second.end());
        off.push_back((int32_t)idx.size());
    }
}

// KeyFrame* -> its resident features. Handles are immutable and shared by every calling thread.
struct KeyFrameCache {
    mutex mu;
    unordered_map<KeyFrame*, orbfe_keyframe*> map;

    // the handle of pKF, created on first use; nullptr when the library refuses it
    orbfe_keyframe* get(KeyFrame* pKF) {
        {
            lock_guard<mutex> lk(mu);
            auto it = map.find(pKF);
            if (it != map.end()) return it->second;
        }
        // kp of the KF index (ORBmatcher.cc:327-329): mvKeysUn, or by side for a two-camera KF
        vector<cv::KeyPoint> keys;
        if (pKF->mpCamera2) {
            keys.assign(pKF->mvKeys.begin(), pKF->mvKeys.end());
            keys.insert(keys.end(), pKF->mvKeysRight.begin(), pKF->mvKeysRight.end());
        }
        orbfe_frame kf;
        memset(&kf, 0, sizeof(kf));
        kf.n = pKF->N;
        kf.keys = reinterpret_cast<const orbfe_keypoint*>(pKF->mpCamera2 ? keys.data() : pKF->mvKeysUn.data());
        kf.desc = pKF->mDescriptors.data;
        vector<uint32_t> ids, idx;
        vector<int32_t> off;
        flatten(pKF->mFeatVec, ids, off, idx);
        const orbfe_feature_vector fv{(int32_t)ids.size(), ids.data(), off.data(), idx.data()};
        orbfe_keyframe* h = nullptr;
        if (orbfe_keyframe_create(&kf, &fv, &h) != ORBFE_OK) return nullptr;
        lock_guard<mutex> lk(mu);
        auto ins = map.emplace(pKF, h);
        if (!ins.second) {   // another thread created it meanwhile
            orbfe_keyframe_destroy(h);
            h = ins.first->second;
        }
        return h;
    }

    void forget(KeyFrame* pKF) {
        orbfe_keyframe* h = nullptr;
        {
            lock_guard<mutex> lk(mu);
            auto it = map.find(pKF);
            if (it == map.end()) return;
            h = it->second;
            map.erase(it);
        }
        orbfe_keyframe_destroy(h);
    }
};

KeyFrameCache& cache() {
    static KeyFrameCache* c = new KeyFrameCache;   // never destroyed: the HIP runtime may be gone at exit
    return *c;
}

// the reference loop, one SearchByBoW per candidate
void per_candidate(const vector<KeyFrame*>& vpKFs, Frame& F, float nnratio, bool checkOri,
                   vector<vector<MapPoint*>>& vvp, vector<int>& vn) {
    ORBmatcher matcher(nnratio, checkOri);
    for (size_t i = 0; i < vpKFs.size(); i++) {
        vvp[i].clear();
        vn[i] = vpKFs[i]->isBad() ? -1 : matcher.SearchByBoW(vpKFs[i], F, vvp[i]);
    }
}

}  // namespace

void ForgetKeyFrameFeatures(KeyFrame* pKF) { cache().forget(pKF); }

void SearchByBoWCandidates(const vector<KeyFrame*>& vpCandidateKFs, Frame& F, float nnratio, bool checkOri,
                           vector<vector<MapPoint*>>& vvpMapPointMatches, vector<int>& vnMatches) {
    const size_t C = vpCandidateKFs.size();
    vvpMapPointMatches.assign(C, vector<MapPoint*>());
    vnMatches.assign(C, -1);
    if (C == 0) return;
    // candidates: NULL for a bad keyframe; map points as int32 handles into one table, bad ones -1
    // (as ORBmatcher::SearchByBoW in shim/ORBmatcher_orbfe.cc flattens them)
    vector<const orbfe_keyframe*> kfs(C, nullptr);
    vector<vector<int32_t>> mps(C);
    vector<const int32_t*> mp_ptr(C, nullptr);
    vector<MapPoint*> table;
    unordered_map<MapPoint*, int32_t> id;
    for (size_t c = 0; c < C; c++) {
        KeyFrame* pKF = vpCandidateKFs[c];
        if (pKF->isBad()) continue;
        kfs[c] = cache().get(pKF);
        if (!kfs[c]) {
            per_candidate(vpCandidateKFs, F, nnratio, checkOri, vvpMapPointMatches, vnMatches);
            return;
        }
        const vector<MapPoint*> vp = pKF->GetMapPointMatches();
        // a keyframe whose slots no longer match its resident features cannot be searched this way
        if ((int)vp.size() != orbfe_keyframe_n(kfs[c])) {
            per_candidate(vpCandidateKFs, F, nnratio, checkOri, vvpMapPointMatches, vnMatches);
            return;
        }
        mps[c].resize(vp.size());
        for (size_t i = 0; i < vp.size(); i++) {
            MapPoint* p = vp[i];
            if (!p || p->isBad()) {
                mps[c][i] = -1;
                continue;
            }
            auto it = id.find(p);
            if (it == id.end()) {
                it = id.emplace(p, (int32_t)table.size()).first;
                table.push_back(p);
            }
            mps[c][i] = it->second;
        }
        mp_ptr[c] = mps[c].data();
    }
    // the current frame: the host view, or the device view while its extractor still holds it
    vector<cv::KeyPoint> fkeys;
    orbfe_frame fr;
    memset(&fr, 0, sizeof(fr));
    fr.n = F.N;
    if (F.Nleft == -1) {
        fr.keys = reinterpret_cast<const orbfe_keypoint*>(F.mvKeysUn.data());
    } else {
        fkeys.assign(F.mvKeys.begin(), F.mvKeys.end());
        fkeys.insert(fkeys.end(), F.mvKeysRight.begin(), F.mvKeysRight.end());
        fr.keys = reinterpret_cast<const orbfe_keypoint*>(fkeys.data());
        fr.two_cams = 1;
        fr.nleft = F.Nleft;
        fr.l2r = F.mvLeftToRightMatch.data();
        fr.r2l = F.mvRightToLeftMatch.data();
    }
    fr.desc = F.mDescriptors.data;
    fr.min_x = Frame::mnMinX; fr.max_x = Frame::mnMaxX; fr.min_y = Frame::mnMinY; fr.max_y = Frame::mnMaxY;
    fr.nlevels = F.mnScaleLevels;
    fr.scale_factors = F.mvScaleFactors.data();
    fr.mbf = F.mbf;
    vector<uint32_t> fid, fidx;
    vector<int32_t> foff;
    flatten(F.mFeatVec, fid, foff, fidx);
    const orbfe_feature_vector ffv{(int32_t)fid.size(), fid.data(), foff.data(), fidx.data()};
    vector<int32_t> out(C * (size_t)F.N, -1), nm(C, 0);
    orbfe_extractor* hl = F.mpORBextractorLeft ? static_cast<orbfe_extractor*>(F.mpORBextractorLeft->OrbfeHandle()) : nullptr;
    const int rc = orbfe_glue::on_current_frame(hl, F.Nleft == -1 ? F.mnOrbfeFrameId : 0, fr, [&](const orbfe_frame* V) {
        return orbfe_search_by_bow_batch(kfs.data(), mp_ptr.data(), (int32_t)C, V, &ffv, out.data(), nm.data(), nnratio,
                                         checkOri ? 1 : 0);
    });
    if (rc < 0) {
        static once_flag logged;
        call_once(logged, [rc] {
            fprintf(stderr, "[orbfe] orbfe_search_by_bow_batch returned %d; searching per candidate\n", rc);
        });
        per_candidate(vpCandidateKFs, F, nnratio, checkOri, vvpMapPointMatches, vnMatches);
        return;
    }
    for (size_t c = 0; c < C; c++) {
        if (!kfs[c]) continue;   // a bad keyframe: discarded by the caller, no matches vector
        vnMatches[c] = nm[c];
        vvpMapPointMatches[c].assign(F.N, nullptr);
        const int32_t* row = out.data() + c * (size_t)F.N;
        for (int i = 0; i < F.N; i++) vvpMapPointMatches[c][i] = row[i] < 0 ? nullptr : table[row[i]];
    }
}

}  // namespace ORB_SLAM3
