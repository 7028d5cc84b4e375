// RGB-D Frame drop-in on top of liborbfe.so (include/orbfe.h): the feature part of
// Frame::Frame(imGray, imDepth, ...) (orb_slam3/src/Frame.cc:200-286) in one library call. Built inside
// the ORB-SLAM3 tree like shim/Frame_orbfe.cc; this repository compiles it with -fsyntax-only against
// stand-in headers (tests/shim_stubs/, tests/test_shim_rgbd_compile.py). A free function over the
// Frame's public members, so Frame.h needs no new member for it (mnOrbfeFrameId is the one
// INTEGRATION.md §2 already adds). The constructor's lines 222-237 become
//
//       const bool fused = ExtractRGBDOrbfe(*this, imGray, imDepth, depthMapFactor);
//       if (!fused) {
//           ExtractORB(0, imGray, 0, 0);
//           N = mvKeys.size();
//           if (mvKeys.empty()) return;
//           UndistortKeyPoints();
//           ComputeStereoFromRGBD(imDepthConverted);   // the caller's convertTo result, see below
//       } else if (mvKeys.empty()) return;
//
// THE DEPTH CONVERSION. Tracking::GrabImageRGBD (Tracking.cc:1576-1577) converts the whole depth image,
// imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor), and the Frame then reads it at ~1000 keypoints.
// The call below takes the RAW imDepth (CV_16UC1 or CV_32FC1, told apart by imDepth.type()) with
// mDepthMapFactor and converts only the values the keypoints read, with the same arithmetic, so
// GrabImageRGBD may drop its convertTo (keeping it only for the fallback above). A caller that keeps
// the convertTo passes the converted CV_32F image with depthMapFactor = 1: ORBFE_DEPTH_F32 with factor
// 1 reads the values untouched.
#include "Frame_rgbd_orbfe.h"

#include <cstdio>
#include <vector>

#include <opencv2/core/hal/interface.h>   // CV_16U, CV_32F
#include <orbfe.h>

#include "ORBextractor.h"
#include "orbfe_glue.h"

namespace ORB_SLAM3 {

namespace {

struct MatRows {   // the cv::Mat descriptor sink of orbfe_glue (as shim/Frame_orbfe.cc)
    cv::Mat m;
    uint8_t* rows(int cap) {
        m.create(cap, 32, CV_8U);
        return m.data;
    }
    void keep(int n) { m = n > 0 ? m.rowRange(0, n) : cv::Mat(); }
};

}  // namespace

bool ExtractRGBDOrbfe(Frame& F, const cv::Mat& imGray, const cv::Mat& imDepth, float depthMapFactor) {
    int depth_type;
    if (imDepth.type() == CV_16UC1) depth_type = ORBFE_DEPTH_U16;
    else if (imDepth.type() == CV_32FC1) depth_type = ORBFE_DEPTH_F32;
    else return false;
    if (imGray.type() != CV_8UC1 || imGray.size() != imDepth.size()) return false;
    const int ndist = F.mDistCoef.rows * F.mDistCoef.cols;   // 4 or 5 in the reference's settings
    if (ndist != 0 && ndist != 4 && ndist != 5 && ndist != 8 && ndist != 12) return false;
    float dist[12] = {0};
    for (int i = 0; i < ndist; i++) dist[i] = F.mDistCoef.at<float>(i);
    const orbfe_rgbd_params p =
        orbfe_glue::rgbd_params(F.mK.at<float>(0, 0), F.mK.at<float>(1, 1), F.mK.at<float>(0, 2), F.mK.at<float>(1, 2),
                                dist, ndist, F.mbf, depthMapFactor);
    orbfe_extractor* h = static_cast<orbfe_extractor*>(F.mpORBextractorLeft->OrbfeHandle());
    MatRows d;
    const int mono = orbfe_glue::frame_rgbd(h, imGray.data, imGray.cols, imGray.rows, (int)imGray.step, imDepth.data,
                                            depth_type, (int)imDepth.step, p, F.mvKeys, F.mvKeysUn, d, F.mvuRight,
                                            F.mvDepth);
    if (mono < 0 && mono != ORBFE_E_EMPTY) {
        static bool logged = false;
        if (!logged) fprintf(stderr, "[orbfe] orbfe_frame_rgbd returned %d; running the CPU implementation\n", mono);
        logged = true;
        return false;
    }
    F.monoLeft = mono;
    F.mDescriptors = d.m;
    F.N = (int)F.mvKeys.size();
    // Tracking's searches on this frame read mvKeysUn / mDescriptors / mvuRight in HBM while the handle
    // still holds them (orbfe_frame_device_view through orbfe_glue::on_current_frame)
    F.mnOrbfeFrameId = F.N > 0 ? orbfe_extractor_frame_id(h) : 0;
    F.mpORBextractorLeft->mvImagePyramid.clear();
    return true;
}

}  // namespace ORB_SLAM3
