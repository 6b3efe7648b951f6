// Calls only: Frame::ComputeStereoFromRGBD, Frame::ComputeStereoLinesFromRGBD and Frame::ComputeSceneMedianDepth of the
// reference (src/Frame.cc, compiled unmodified into oracle/_ref/libmatchers_ref.so) on a Frame filled from flat arrays.
// Built into a temporary directory by scripts/make_frame_rgbd_golden.py with the include flags of oracle/ref/Makefile's
// matchers target; dev-time only.
#define private public
#define protected public
#include "Frame.h"
#undef private
#undef protected

#include <cstring>

#include "plvs_hip.h"

using namespace PLVS2;

namespace {
cv::Mat depth_mat(const float* depth, int width, int height, int pitch) {
  return cv::Mat(height, width, CV_32F, const_cast<float*>(depth), sizeof(float) * (size_t)pitch);
}
}  // namespace

extern "C" {

// -> mvuRight, mvDepth, mMedianDepth (use_median = mbUseFovCentersKfGenCriterion) and ComputeSceneMedianDepth() called directly
void ref_frame_stereo_from_rgbd(const plvs_keypoint* kps, const plvs_keypoint* kps_un, int n, const float* depth, int width,
                                int height, int pitch, float mbf, int use_median, float* u_right, float* depth_out, float* median2) {
  Frame F;
  F.N = n;
  F.mvKeys.resize(n);
  F.mvKeysUn.resize(n);
  for (int i = 0; i < n; ++i) {
    F.mvKeys[i].pt = cv::Point2f(kps[i].x, kps[i].y);
    F.mvKeysUn[i].pt = cv::Point2f(kps_un[i].x, kps_un[i].y);
  }
  F.mbf = mbf;
  const bool keep = Frame::mbUseFovCentersKfGenCriterion;
  Frame::mbUseFovCentersKfGenCriterion = use_median != 0;
  F.ComputeStereoFromRGBD(depth_mat(depth, width, height, pitch));
  Frame::mbUseFovCentersKfGenCriterion = keep;
  for (int i = 0; i < n; ++i) {
    u_right[i] = F.mvuRight[i];
    depth_out[i] = F.mvDepth[i];
  }
  median2[0] = F.mMedianDepth;
  median2[1] = F.ComputeSceneMedianDepth();
}

void ref_frame_stereo_lines_from_rgbd(const plvs_keyline* kl, const plvs_keyline* kl_un, int n, const float* depth, int width,
                                      int height, int pitch, const float* K4, float mbf, float min_line_length_3d,
                                      float* u_right_start, float* depth_start, float* u_right_end, float* depth_end) {
  static_assert(sizeof(plvs_keyline) == sizeof(cv::line_descriptor_c::KeyLine), "plvs_keyline is KeyLine field for field");
  Frame F;
  F.Nlines = n;
  F.mvKeyLines.resize(n);
  F.mvKeyLinesUn.resize(n);
  if (n) {
    std::memcpy(F.mvKeyLines.data(), kl, sizeof(plvs_keyline) * (size_t)n);
    std::memcpy(F.mvKeyLinesUn.data(), kl_un, sizeof(plvs_keyline) * (size_t)n);
  }
  F.mbf = mbf;
  Frame::fx = K4[0]; Frame::fy = K4[1]; Frame::cx = K4[2]; Frame::cy = K4[3];
  Frame::invfx = 1.0f / Frame::fx;   // as the constructor sets them
  Frame::invfy = 1.0f / Frame::fy;
  const float keep = Frame::skMinLineLength3D;
  Frame::skMinLineLength3D = min_line_length_3d;
  F.ComputeStereoLinesFromRGBD(depth_mat(depth, width, height, pitch));
  Frame::skMinLineLength3D = keep;
  for (int i = 0; i < n; ++i) {
    u_right_start[i] = F.mvuRightLineStart[i];
    depth_start[i] = F.mvDepthLineStart[i];
    u_right_end[i] = F.mvuRightLineEnd[i];
    depth_end[i] = F.mvDepthLineEnd[i];
  }
}

}  // extern "C"
