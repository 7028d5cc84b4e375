// The neighbour loop of LocalMapping::CreateNewMapPoints (orb_slam3/src/LocalMapping.cc:388-470) on top
// of liborbfe.so: SearchForTriangulation of the current keyframe against every covisible neighbour in
// ONE device call (orbfe_search_for_triangulation_batch, one workgroup per neighbour) instead of one call,
// two keyframe uploads and one host wait per neighbour. The keyframes are the resident ones of
// shim/Relocalization_orbfe.cc's cache (orbfe_keyframe_create_geom); per call only GetMapPoint presence of
// the current keyframe and of each neighbour crosses the link. The per-neighbour
// ORBmatcher::SearchForTriangulation (shim/ORBmatcher_backend_orbfe.cc, which itself falls back to the CPU
// body) runs when the library returns an error, when a keyframe pair needs the caller-side epipolar test
// (a KannalaBrandt8 camera with bCoarse false), and when the rotation check is on.
// Built inside the ORB-SLAM3 tree; this repository compiles it with -fsyntax-only against stand-in
// headers (tests/shim_stubs/, tests/test_shim_compile.py). See INTEGRATION.md §4.
#include "LocalMapping_orbfe.h"

#include <cstdio>
#include <cstring>
#include <mutex>

#include <orbfe.h>

#include "Relocalization_orbfe.h"
#include "orbfe_slam_types.h"

#include "KeyFrame.h"
#include "MapPoint.h"
#include "ORBmatcher.h"

using namespace std;

namespace ORB_SLAM3 {

namespace {

// the reference loop, one SearchForTriangulation per neighbour
void per_neighbour(KeyFrame* pKF1, const vector<KeyFrame*>& vpKF2, bool bOnlyStereo, bool bCoarse, bool checkOri,
                   vector<vector<pair<size_t, size_t>>>& vvMatched, vector<int>& vn) {
    ORBmatcher matcher(0.6f, checkOri);
    for (size_t c = 0; c < vpKF2.size(); c++) {
        vvMatched[c].clear();
        vn[c] = vpKF2[c] ? matcher.SearchForTriangulation(pKF1, vpKF2[c], vvMatched[c], bOnlyStereo, bCoarse) : 0;
    }
}

void presence(KeyFrame* pKF, vector<int32_t>& mp) {
    mp.resize(pKF->N);
    for (int i = 0; i < pKF->N; i++) mp[i] = pKF->GetMapPoint(i) ? 1 : -1;
}

}  // namespace

void SearchForTriangulationNeighbours(KeyFrame* pKF1, const vector<KeyFrame*>& vpKF2, bool bOnlyStereo, bool bCoarse,
                                      vector<vector<pair<size_t, size_t>>>& vvMatched, vector<int>& vn, bool checkOri) {
    const size_t C = vpKF2.size();
    vvMatched.assign(C, vector<pair<size_t, size_t>>());
    vn.assign(C, 0);
    if (C == 0) return;
    auto fallback = [&] { per_neighbour(pKF1, vpKF2, bOnlyStereo, bCoarse, checkOri, vvMatched, vn); };
    if (checkOri) return fallback();
    // the F12 form serves pinhole pairs, and two-camera keyframes with bCoarse; every other pair takes the
    // camera model's own epipolar test on the host (orbfe_search_for_triangulation_epi), per neighbour
    const bool two1 = pKF1->mpCamera2 != nullptr;
    const bool pin1 = pKF1->mpCamera->GetType() == GeometricCamera::CAM_PINHOLE;
    for (KeyFrame* pKF2 : vpKF2) {
        if (!pKF2) continue;
        const bool two2 = pKF2->mpCamera2 != nullptr;
        const bool pin = pin1 && pKF2->mpCamera->GetType() == GeometricCamera::CAM_PINHOLE;
        if (!bCoarse && (two1 || two2 || !pin)) return fallback();
    }
    const orbfe_keyframe* h1 = ResidentKeyFrame(pKF1);
    if (!h1 || orbfe_keyframe_n(h1) != pKF1->N) return fallback();
    vector<int32_t> mp1;
    presence(pKF1, mp1);
    vector<orbfe_tri_job> jobs(C);
    vector<vector<int32_t>> mp2(C);
    memset(jobs.data(), 0, C * sizeof(orbfe_tri_job));
    // the per-neighbour constants, computed exactly as the reference does (ORBmatcher.cc:913-940,
    // Pinhole.cpp:109-112) and as ORBmatcher::SearchForTriangulation in ORBmatcher_backend_orbfe.cc does
    const Sophus::SE3f T1w = pKF1->GetPose();
    const Eigen::Matrix3f K1 = pKF1->mpCamera->toK_();
    for (size_t c = 0; c < C; c++) {
        KeyFrame* pKF2 = vpKF2[c];
        if (!pKF2) continue;
        const orbfe_keyframe* h2 = ResidentKeyFrame(pKF2);
        if (!h2 || orbfe_keyframe_n(h2) != pKF2->N) return fallback();
        const Sophus::SE3f T2w = pKF2->GetPose(), Tw2 = pKF2->GetPoseInverse();
        const Eigen::Vector3f C2 = T2w * pKF1->GetCameraCenter();
        const Eigen::Vector2f ep = pKF2->mpCamera->project(C2);
        const Sophus::SE3f T12 = T1w * Tw2;
        const Eigen::Matrix3f R12 = T12.rotationMatrix();
        const Eigen::Vector3f t12 = T12.translation();
        const Eigen::Matrix3f K2 = pKF2->mpCamera->toK_();
        const Eigen::Matrix3f F = K1.transpose().inverse() * Sophus::SO3f::hat(t12) * R12 * K2.inverse();
        orbfe_tri_job& j = jobs[c];
        for (int r = 0; r < 3; r++)
            for (int k = 0; k < 3; k++) j.F12[3 * r + k] = F(r, k);
        j.ep[0] = ep(0);
        j.ep[1] = ep(1);
        presence(pKF2, mp2[c]);
        j.kf2 = h2;
        j.mp2 = mp2[c].data();
    }
    const size_t n1 = (size_t)pKF1->N;
    vector<int32_t> rows(C * n1, -1), nm(C, 0);
    const int rc = orbfe_search_for_triangulation_batch(h1, mp1.data(), jobs.data(), (int32_t)C, bOnlyStereo ? 1 : 0,
                                                        bCoarse ? 1 : 0, 0, rows.data(), nm.data());
    if (rc < 0) {
        static once_flag logged;
        call_once(logged, [rc] {
            fprintf(stderr, "[orbfe] orbfe_search_for_triangulation_batch returned %d; searching per neighbour\n", rc);
        });
        return fallback();
    }
    for (size_t c = 0; c < C; c++) {
        if (!vpKF2[c]) continue;
        vn[c] = nm[c];
        vvMatched[c].reserve(nm[c]);
        const int32_t* row = rows.data() + c * n1;
        for (size_t i = 0; i < n1; i++)
            if (row[i] >= 0) vvMatched[c].push_back(make_pair(i, (size_t)row[i]));
    }
}

}  // namespace ORB_SLAM3
