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
#include <set>
#include <unordered_map>

#include <orbfe.h>

#include "orbfe_glue.h"
#include "orbfe_slam_types.h"

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
        // the geometry SearchForTriangulation reads besides (shim/LocalMapping_orbfe.cc): mvuRight, the
        // octaves and the level tables are as immutable as the descriptors
        kf.uright = pKF->mvuRight.empty() ? nullptr : pKF->mvuRight.data();
        kf.nlevels = pKF->mnScaleLevels;
        kf.scale_factors = pKF->mvScaleFactors.data();
        kf.two_cams = pKF->mpCamera2 ? 1 : 0;
        // and what Fuse reads besides (FuseNeighbours_orbfe): the image bounds, mbf and NLeft
        kf.min_x = pKF->mnMinX; kf.max_x = pKF->mnMaxX; kf.min_y = pKF->mnMinY; kf.max_y = pKF->mnMaxY;
        kf.mbf = pKF->mbf;
        kf.nleft = pKF->mpCamera2 ? pKF->NLeft : 0;
        vector<uint32_t> ids, idx;
        vector<int32_t> off;
        flatten(pKF->mFeatVec, ids, off, idx);
        const orbfe_feature_vector fv{(int32_t)ids.size(), ids.data(), off.data(), idx.data()};
        orbfe_keyframe* h = nullptr;
        if ((int)pKF->mvLevelSigma2.size() < kf.nlevels) return nullptr;
        // with its search grid; a keyframe the grid refuses (more than 8,192 features) keeps its geometry
        if (orbfe_keyframe_create_grid(&kf, &fv, pKF->mvLevelSigma2.data(), &h) != ORBFE_OK &&
            orbfe_keyframe_create_geom(&kf, &fv, pKF->mvLevelSigma2.data(), &h) != ORBFE_OK)
            return nullptr;
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

const orbfe_keyframe* ResidentKeyFrame(KeyFrame* pKF) { return cache().get(pKF); }

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

namespace {

// Frame::SetPose (include/Frame.h). The stand-in Frame this repository compiles the shim against
// (tests/shim_stubs/Frame.h) declares no SetPose: there the second overload is chosen and reports it.
template <class Fr>
auto set_pose(Fr& F, const Sophus::SE3f& Tcw, int) -> decltype(F.SetPose(Tcw), true) {
    F.SetPose(Tcw);
    return true;
}
template <class Fr>
bool set_pose(Fr&, const Sophus::SE3f&, long) {
    fprintf(stderr, "[orbfe] Frame has no SetPose: the per-candidate SearchByProjection cannot run\n");
    return false;
}

// the reference calls, one candidate at a time: F takes the candidate's pose and slots for its call
void sbp_per_candidate(Frame& F, const vector<KeyFrame*>& vpKFs, const vector<Sophus::SE3f>& vTcw,
                       const vector<set<MapPoint*>>& vsFound, vector<vector<MapPoint*>>& vvp, float th, int ORBdist,
                       bool checkOri, vector<int>& vn) {
    ORBmatcher matcher(0.9, checkOri);
    const Sophus::SE3f Tcw0 = F.GetPose();
    const vector<MapPoint*> mvp0 = F.mvpMapPoints;
    for (size_t c = 0; c < vpKFs.size(); c++) {
        vn[c] = 0;
        if (!vpKFs[c]) continue;
        if (!set_pose(F, vTcw[c], 0)) break;
        F.mvpMapPoints = vvp[c];
        vn[c] = matcher.SearchByProjection(F, vpKFs[c], vsFound[c], th, ORBdist);
        vvp[c] = F.mvpMapPoints;
    }
    set_pose(F, Tcw0, 0);
    F.mvpMapPoints = mvp0;
}

}  // namespace

void SearchByProjectionCandidates(Frame& F, const vector<KeyFrame*>& vpKFs, const vector<Sophus::SE3f>& vTcw,
                                  const vector<set<MapPoint*>>& vsFound, vector<vector<MapPoint*>>& vvpMapPoints,
                                  float th, int ORBdist, bool checkOri, vector<int>& vnAdditional) {
    const size_t C = vpKFs.size();
    vnAdditional.assign(C, 0);
    if (C == 0) return;
    auto fallback = [&] {
        sbp_per_candidate(F, vpKFs, vTcw, vsFound, vvpMapPoints, th, ORBdist, checkOri, vnAdditional);
    };
    // two-camera frames are not batched (the call refuses them): straight to the per-candidate calls
    if (F.Nleft != -1) return fallback();
    // per candidate: the resident keyframe, CurrentFrame's pose for it, and the map points the reference
    // loop would project (non-NULL, not bad, not in sFound; ORBmatcher.cc:1905-1911) in KF slot order
    vector<const orbfe_keyframe*> kfs(C, nullptr);
    vector<orbfe_kf_camera> cams(C);
    vector<vector<orbfe_map_point_3d>> pts(C);
    vector<vector<int32_t>> idx(C);
    vector<const orbfe_map_point_3d*> pts_ptr(C, nullptr);
    vector<const int32_t*> idx_ptr(C, nullptr);
    vector<int32_t> npts(C, 0);
    vector<MapPoint*> table;
    unordered_map<MapPoint*, int32_t> id;
    auto handle = [&](MapPoint* p) -> int32_t {
        if (!p) return -1;
        auto it = id.find(p);
        if (it == id.end()) {
            it = id.emplace(p, (int32_t)table.size()).first;
            table.push_back(p);
        }
        return it->second;
    };
    memset(cams.data(), 0, C * sizeof(orbfe_kf_camera));
    for (size_t c = 0; c < C; c++) {
        KeyFrame* pKF = vpKFs[c];
        if (!pKF) continue;
        kfs[c] = cache().get(pKF);
        const vector<MapPoint*> vp = pKF->GetMapPointMatches();
        if (!kfs[c] || (int)vp.size() != orbfe_keyframe_n(kfs[c]) || (int)vvpMapPoints[c].size() != F.N) return fallback();
        orbfe_kf_camera& cam = cams[c];
        cam.Tcw = orbfe_shim::pose_of(vTcw[c]);
        const Eigen::Vector3f Ow = vTcw[c].inverse().translation();   // ORBmatcher.cc:1894
        cam.Ow[0] = Ow(0); cam.Ow[1] = Ow(1); cam.Ow[2] = Ow(2);
        cam.log_scale_factor = F.mfLogScaleFactor;
        for (size_t i = 0; i < vp.size(); i++) {
            MapPoint* p = vp[i];
            if (!p || p->isBad() || vsFound[c].count(p)) continue;
            orbfe_map_point_3d r;
            memset(&r, 0, sizeof(r));
            const Eigen::Vector3f x3Dw = p->GetWorldPos();
            r.pos[0] = x3Dw(0); r.pos[1] = x3Dw(1); r.pos[2] = x3Dw(2);
            r.min_dist = p->GetMinDistance();   // accessors INTEGRATION.md §2 adds to MapPoint.h
            r.max_dist = p->GetMaxDistance();
            r.id = handle(p);
            memcpy(r.desc, p->GetDescriptor().ptr<uint8_t>(0), 32);
            pts[c].push_back(r);
            idx[c].push_back((int32_t)i);
        }
        npts[c] = (int32_t)pts[c].size();
        pts_ptr[c] = pts[c].data();
        idx_ptr[c] = idx[c].data();
    }
    const orbfe_camera_model model = orbfe_shim::model_of(F.mpCamera);
    vector<int32_t> mvp(C * (size_t)F.N, -1), nm(C, 0);
    for (size_t c = 0; c < C; c++)
        for (int i = 0; kfs[c] && i < F.N; i++) mvp[c * (size_t)F.N + i] = handle(vvpMapPoints[c][i]);
    orbfe_frame fr;
    memset(&fr, 0, sizeof(fr));
    fr.n = F.N;
    fr.keys = reinterpret_cast<const orbfe_keypoint*>(F.mvKeysUn.data());
    fr.desc = F.mDescriptors.data;
    fr.min_x = Frame::mnMinX; fr.max_x = Frame::mnMaxX; fr.min_y = Frame::mnMinY; fr.max_y = Frame::mnMaxY;
    fr.nlevels = F.mnScaleLevels;
    fr.scale_factors = F.mvScaleFactors.data();
    fr.mbf = F.mbf;
    orbfe_extractor* hl = F.mpORBextractorLeft ? static_cast<orbfe_extractor*>(F.mpORBextractorLeft->OrbfeHandle()) : nullptr;
    const int rc = orbfe_glue::on_current_frame(hl, F.mnOrbfeFrameId, fr, [&](const orbfe_frame* V) {
        return orbfe_search_by_projection_kf_batch(V, kfs.data(), cams.data(), &model, pts_ptr.data(), idx_ptr.data(),
                                                   npts.data(), (int32_t)C, mvp.data(), nm.data(), th, ORBdist,
                                                   checkOri ? 1 : 0);
    });
    if (rc < 0) {
        static once_flag logged;
        call_once(logged, [rc] {
            fprintf(stderr, "[orbfe] orbfe_search_by_projection_kf_batch returned %d; searching per candidate\n", rc);
        });
        return fallback();
    }
    for (size_t c = 0; c < C; c++) {
        if (!kfs[c]) continue;
        vnAdditional[c] = nm[c];
        const int32_t* row = mvp.data() + c * (size_t)F.N;
        for (int i = 0; i < F.N; i++) vvpMapPoints[c][i] = row[i] < 0 ? nullptr : table[row[i]];
    }
}

}  // namespace ORB_SLAM3
