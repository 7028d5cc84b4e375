// The candidates loop of Tracking::Relocalization (Tracking.cc:3680-3692) as one call: see
// shim/Relocalization_orbfe.cc and INTEGRATION.md.
#pragma once
#include <vector>

namespace ORB_SLAM3 {

class Frame;
class KeyFrame;
class MapPoint;

// SearchByBoW(vpCandidateKFs[i], F, vvpMapPointMatches[i]) with ORBmatcher(nnratio, checkOri) for
// every candidate, in one device call. vnMatches[i] = nmatches, or -1 for a candidate that isBad()
// (its vvpMapPointMatches[i] stays empty, as in the reference loop).
void SearchByBoWCandidates(const std::vector<KeyFrame*>& vpCandidateKFs, Frame& F, float nnratio, bool checkOri,
                           std::vector<std::vector<MapPoint*>>& vvpMapPointMatches, std::vector<int>& vnMatches);

// Drops pKF's device-resident features (call it where the KeyFrame is deleted or its mFeatVec /
// mDescriptors are rebuilt); must not run while SearchByBoWCandidates uses pKF.
void ForgetKeyFrameFeatures(KeyFrame* pKF);

}  // namespace ORB_SLAM3
