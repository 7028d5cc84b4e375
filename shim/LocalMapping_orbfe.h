// The neighbour searches of LocalMapping::CreateNewMapPoints (LocalMapping.cc:388-470) as one call: see
// shim/LocalMapping_orbfe.cc and INTEGRATION.md §4.
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

namespace ORB_SLAM3 {

class KeyFrame;
class MapPoint;

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

// matcher.Fuse(vpTargetKFs[c], vpMapPoints, th), and for a two-camera keyframe matcher.Fuse(vpTargetKFs[c],
// vpMapPoints, th, true) after it, for every target c in order: the target loop of
// LocalMapping::SearchInNeighbors (LocalMapping.cc:765-775) with one device call for all the searches
// (orbfe_fuse_batch over the resident keyframes) and then the reference's commit body job by job and point
// by point, each point's isBad() / IsInKeyFrame gate re-read as it commits (INTEGRATION.md §4 says why
// that is the sequential loop's map). The backward Fuse(mpCurrentKeyFrame, vpFuseCandidates) (:802-803) is
// the same call with one target. A NULL or bad target is skipped. Returns the number of fused points over
// all targets. Runs the per-keyframe ORBmatcher::Fuse calls when a handle is missing or the batched call
// returns an error.
int FuseNeighbours_orbfe(const std::vector<KeyFrame*>& vpTargetKFs, const std::vector<MapPoint*>& vpMapPoints,
                         float th = 3.0f);

}  // namespace ORB_SLAM3
