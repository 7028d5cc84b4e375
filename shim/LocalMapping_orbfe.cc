// The neighbour loop of LocalMapping::CreateNewMapPoints (orb_slam3/src/LocalMapping.cc:388-470) on top
// of liborbfe.so: SearchForTriangulation of the current keyframe against every covisible neighbour in
// ONE device call (orbfe_search_for_triangulation_batch, one workgroup per neighbour) instead of one call,
// two keyframe uploads and one host wait per neighbour. The keyframes are the resident ones of
// shim/Relocalization_orbfe.cc's cache (orbfe_keyframe_create_geom); per call only GetMapPoint presence of
// the current keyframe and of each neighbour crosses the link. The per-neighbour
// ORBmatcher::SearchForTriangulation (shim/ORBmatcher_backend_orbfe.cc, which itself falls back to the CPU
// body) runs when the library returns an error, when a keyframe pair needs the caller-side epipolar test
// (a KannalaBrandt8 camera with bCoarse false), and when the rotation check is on.
// FuseNeighbours_orbfe does the same for the Fuse loop of LocalMapping::SearchInNeighbors (:765-775, :802):
// one orbfe_fuse_batch over the resident keyframes' grids, then the reference's commit in its order.
// Built inside the ORB-SLAM3 tree; this repository compiles it with -fsyntax-only against stand-in
// headers (tests/shim_stubs/, tests/test_shim_compile.py). See INTEGRATION.md §4.
#include "LocalMapping_orbfe.h"

#include <cstdio>
#include <cstring>
#include <mutex>
#include <unordered_map>

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

// the reference loop, one Fuse (two for a two-camera keyframe) per target
int fuse_per_keyframe(const vector<KeyFrame*>& vpTargetKFs, const vector<MapPoint*>& vpMapPoints, float th) {
    ORBmatcher matcher;
    int n = 0;
    for (KeyFrame* pKFi : vpTargetKFs) {
        if (!pKFi || pKFi->isBad()) continue;
        n += matcher.Fuse(pKFi, vpMapPoints, th);
        if (pKFi->NLeft != -1) n += matcher.Fuse(pKFi, vpMapPoints, th, true);
    }
    return n;
}

orbfe_kf_camera fuse_camera(KeyFrame* K, const Sophus::SE3f& Tcw, const Eigen::Vector3f& Ow) {
    orbfe_kf_camera c;
    c.Tcw = orbfe_shim::pose_of(Tcw);
    c.Ow[0] = Ow(0); c.Ow[1] = Ow(1); c.Ow[2] = Ow(2);
    c.fx = K->fx; c.fy = K->fy; c.cx = K->cx; c.cy = K->cy;
    c.log_scale_factor = K->mfLogScaleFactor;
    return c;
}

}  // namespace

int FuseNeighbours_orbfe(const vector<KeyFrame*>& vpTargetKFs, const vector<MapPoint*>& vpMapPoints, float th) {
    const size_t n = vpMapPoints.size();
    if (vpTargetKFs.empty() || n == 0) return 0;
    auto fallback = [&] { return fuse_per_keyframe(vpTargetKFs, vpMapPoints, th); };
    // the jobs in the reference's order: a target's left search, then its right one (:772-773)
    struct Target {
        KeyFrame* pKF;
        bool bRight;
    };
    vector<Target> targets;
    vector<orbfe_fuse_job> jobs;
    for (KeyFrame* pKFi : vpTargetKFs) {
        if (!pKFi || pKFi->isBad()) continue;
        const orbfe_keyframe* h = ResidentKeyFrame(pKFi);
        if (!h || orbfe_keyframe_has_grid(h) != 1 || orbfe_keyframe_n(h) != pKFi->N) return fallback();
        for (int side = 0; side < (pKFi->NLeft != -1 ? 2 : 1); side++) {
            orbfe_fuse_job j;
            memset(&j, 0, sizeof(j));
            j.kf = h;
            // pCamera / Tcw / Ow as the reference selects them (ORBmatcher.cc:1154-1163)
            j.model = orbfe_shim::model_of(side ? pKFi->mpCamera2 : pKFi->mpCamera);
            j.cam = side ? fuse_camera(pKFi, pKFi->GetRightPose(), pKFi->GetRightCameraCenter())
                         : fuse_camera(pKFi, pKFi->GetPose(), pKFi->GetCameraCenter());
            j.bRight = side;
            jobs.push_back(j);
            targets.push_back(Target{pKFi, side != 0});
        }
    }
    const size_t J = jobs.size();
    if (J == 0) return 0;
    // a point as the search reads it now; GetMinDistance / GetMaxDistance: the accessors of INTEGRATION.md §2
    auto record = [](MapPoint* p) {
        orbfe_map_point_3d m;
        memset(&m, 0, sizeof(m));
        m.id = p ? 0 : -1;
        if (!p) return m;
        const Eigen::Vector3f X = p->GetWorldPos(), nr = p->GetNormal();
        for (int k = 0; k < 3; k++) { m.pos[k] = X(k); m.normal[k] = nr(k); }
        m.min_dist = p->GetMinDistance();
        m.max_dist = p->GetMaxDistance();
        m.flags = p->isBad() ? ORBFE_MP_BAD : 0;
        m.observations = p->Observations();
        memcpy(m.desc, p->GetDescriptor().data, 32);
        return m;
    };
    // rows [c0, J) of the points `which`, searched in one call with the points and the IsInKeyFrame gates
    // as they are now, written into best
    vector<int32_t> best(J * n, -1);
    auto search = [&](size_t c0, const vector<size_t>& which) {
        const size_t R = J - c0, m = which.size();
        vector<orbfe_map_point_3d> q(m);
        for (size_t k = 0; k < m; k++) q[k] = record(vpMapPoints[which[k]]);
        vector<uint8_t> skip(R * m, 0);
        vector<orbfe_fuse_job> sub(jobs.begin() + c0, jobs.end());
        for (size_t r = 0; r < R; r++) {
            for (size_t k = 0; k < m; k++) {
                MapPoint* p = vpMapPoints[which[k]];
                skip[r * m + k] = p && p->IsInKeyFrame(targets[c0 + r].pKF) ? 1 : 0;
            }
            sub[r].skip = skip.data() + r * m;
        }
        vector<int32_t> b(R * m, -1), d(R * m, -1), nf(R, 0);
        const int rc = orbfe_fuse_batch(sub.data(), (int32_t)R, q.data(), (int32_t)m, th, 0, b.data(), d.data(), nf.data());
        if (rc < 0) {
            static once_flag logged;
            call_once(logged, [rc] { fprintf(stderr, "[orbfe] orbfe_fuse_batch returned %d; fusing per keyframe\n", rc); });
            return false;
        }
        for (size_t r = 0; r < R; r++)
            for (size_t k = 0; k < m; k++) best[(c0 + r) * n + which[k]] = b[r * m + k];
        return true;
    };
    vector<size_t> all(n);
    unordered_map<MapPoint*, size_t> where;
    for (size_t i = 0; i < n; i++) {
        all[i] = i;
        if (vpMapPoints[i]) where.emplace(vpMapPoints[i], i);
    }
    if (!search(0, all)) return fallback();
    // the reference's commit (ORBmatcher.cc:1300-1330), job by job and in point order. A commit moves a later
    // point's isBad() / IsInKeyFrame gate from searched to skipped only, so the gate is re-read here. It
    // changes what a later search reads in one case: Replace ends with ComputeDistinctiveDescriptors() of the
    // surviving point. A survivor that is one of vpMapPoints is searched again, with its new descriptor, in
    // the jobs still to come (one small call for all such points of a job) before the next job commits.
    ORBmatcher matcher;
    int nFused = 0;
    vector<size_t> renewed;
    for (size_t c = 0; c < J; c++) {
        KeyFrame* pKF = targets[c].pKF;
        if (!renewed.empty()) {
            if (!search(c, renewed)) {   // the rest as the reference runs it
                for (size_t r = c; r < J; r++) nFused += matcher.Fuse(targets[r].pKF, vpMapPoints, th, targets[r].bRight);
                return nFused;
            }
            renewed.clear();
        }
        const int32_t* row = best.data() + c * n;
        for (size_t i = 0; i < n; i++) {
            MapPoint* pMP = vpMapPoints[i];
            if (row[i] < 0 || !pMP || pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;
            MapPoint* pMPinKF = pKF->GetMapPoint(row[i]);
            if (pMPinKF) {
                if (!pMPinKF->isBad()) {
                    if (pMPinKF->Observations() > pMP->Observations()) {
                        pMP->Replace(pMPinKF);
                        auto it = where.find(pMPinKF);
                        if (it != where.end()) renewed.push_back(it->second);
                    } else {
                        pMPinKF->Replace(pMP);
                        renewed.push_back(i);
                    }
                }
            } else {
                pMP->AddObservation(pKF, row[i]);
                pKF->AddMapPoint(pMP, row[i]);
            }
            nFused++;
        }
    }
    return nFused;
}

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
