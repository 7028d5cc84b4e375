// The candidates loop of Tracking::Relocalization (Tracking.cc:3680-3692) as one call: see
// shim/Relocalization_orbfe.cc and INTEGRATION.md.
#pragma once
#include <set>
#include <vector>

#include "Frame.h"   // Sophus::SE3f

struct orbfe_keyframe;   // <orbfe.h>

namespace ORB_SLAM3 {

class KeyFrame;
class MapPoint;

// SearchByBoW(vpCandidateKFs[i], F, vvpMapPointMatches[i]) with ORBmatcher(nnratio, checkOri) for
// every candidate, in one device call. vnMatches[i] = nmatches, or -1 for a candidate that isBad()
// (its vvpMapPointMatches[i] stays empty, as in the reference loop).
void SearchByBoWCandidates(const std::vector<KeyFrame*>& vpCandidateKFs, Frame& F, float nnratio, bool checkOri,
                           std::vector<std::vector<MapPoint*>>& vvpMapPointMatches, std::vector<int>& vnMatches);

// The refinement searches of one sweep of Tracking::Relocalization's candidates loop (Tracking.cc:3765:
// th 10, ORBdist 100; :3779: th 3, ORBdist 64) in one device call: for every c with vpKFs[c] != NULL,
// ORBmatcher(0.9, checkOri).SearchByProjection(F, vpKFs[c], vsFound[c], th, ORBdist) as if F had the pose
// vTcw[c] and the slots vvpMapPoints[c] (F.N entries, updated in place); vnAdditional[c] = its nmatches
// (0 for a NULL candidate, whose row stays as it is). F itself is only read (restored after a fallback).
void SearchByProjectionCandidates(Frame& F, const std::vector<KeyFrame*>& vpKFs, const std::vector<Sophus::SE3f>& vTcw,
                                  const std::vector<std::set<MapPoint*>>& vsFound,
                                  std::vector<std::vector<MapPoint*>>& vvpMapPoints, float th, int ORBdist,
                                  bool checkOri, std::vector<int>& vnAdditional);

// Drops pKF's device-resident features (call it where the KeyFrame is deleted or its mFeatVec /
// mDescriptors are rebuilt); must not run while SearchByBoWCandidates uses pKF.
void ForgetKeyFrameFeatures(KeyFrame* pKF);

// pKF's resident features with geometry (orbfe_keyframe_create_geom), created on first use and shared by
// every search of this file and of shim/LocalMapping_orbfe.cc; NULL when the library refuses the keyframe.
const ::orbfe_keyframe* ResidentKeyFrame(KeyFrame* pKF);

}  // namespace ORB_SLAM3
