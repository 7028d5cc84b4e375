// TEST INFRASTRUCTURE (tests/test_shim_rgbd_compile.py, tests/test_shim_compile.py): stand-in for
// OpenCV's <opencv2/core/hal/interface.h>, the header that defines the depth codes. Only the codes the
// RGB-D shim (shim/Frame_rgbd_orbfe.cc) reads and stub_types.h does not define, with OpenCV's values.
#pragma once
#ifndef CV_16U
#define CV_16U 2
#endif
#ifndef CV_32F
#define CV_32F 5
#endif
#ifndef CV_16UC1
#define CV_16UC1 CV_16U
#endif
#ifndef CV_32FC1
#define CV_32FC1 CV_32F
#endif
