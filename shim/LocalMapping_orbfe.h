// The neighbour searches of LocalMapping::CreateNewMapPoints (LocalMapping.cc:388-470) as one call: see
// shim/LocalMapping_orbfe.cc and INTEGRATION.md §4.
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

namespace ORB_SLAM3 {

class KeyFrame;

// ORBmatcher(0.6, checkOri).SearchForTriangulation(pKF1, vpKF2[c], vvMatched[c], bOnlyStereo, bCoarse) for
// every neighbour c, each against pKF1's map points as they are at the call (the snapshot before the
// triangulation loop), in one device call. vpKF2[c] == NULL is a skipped neighbour (the baseline gate):
// vvMatched[c] stays empty and vn[c] = 0. vn[c] = the pairs found. CreateNewMapPoints builds its matcher
// with checkOri false. With checkOri true the per-neighbour ORBmatcher::SearchForTriangulation calls run
// here instead of the batch, and a caller that interleaves AddMapPoint with the searches must keep the
// reference's loop: the rotation histogram depends on which keypoints took part.
void SearchForTriangulationNeighbours(KeyFrame* pKF1, const std::vector<KeyFrame*>& vpKF2, bool bOnlyStereo,
                                      bool bCoarse, std::vector<std::vector<std::pair<size_t, size_t>>>& vvMatched,
                                      std::vector<int>& vn, bool checkOri = false);

}  // namespace ORB_SLAM3
