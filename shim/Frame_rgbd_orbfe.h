// Declaration of the RGB-D Frame drop-in (shim/Frame_rgbd_orbfe.cc); include it from Frame.cc.
#pragma once
#include "Frame.h"

namespace ORB_SLAM3 {

// Frame.cc:222-237 (ExtractORB(0, imGray, 0, 0), N, UndistortKeyPoints, ComputeStereoFromRGBD) in one
// library call over the RAW depth image; depthMapFactor = Tracking's mDepthMapFactor (already
// inverted, Tracking.cc:613-617). false: the constructor runs its original lines.
bool ExtractRGBDOrbfe(Frame& F, const cv::Mat& imGray, const cv::Mat& imDepth, float depthMapFactor);

}  // namespace ORB_SLAM3
