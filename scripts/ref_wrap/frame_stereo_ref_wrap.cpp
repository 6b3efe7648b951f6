// Calls only: Frame::ComputeStereoLineMatches of the reference (src/Frame.cc with src/LineMatcher.cc, compiled unmodified into
// oracle/_ref/libmatchers_ref.so) on a Frame filled from flat arrays.  Built into a temporary directory by
// scripts/make_frame_stereo_golden.py with the include flags of oracle/ref/Makefile's matchers target; dev-time only.
#define private public
#define protected public
#include "Frame.h"
#undef private
#undef protected

#include <cstring>

#include "plvs_hip.h"

using namespace PLVS2;

namespace {
void fill(std::vector<cv::line_descriptor_c::KeyLine>& dst, const plvs_keyline* src, int n) {
  static_assert(sizeof(plvs_keyline) == sizeof(cv::line_descriptor_c::KeyLine), "plvs_keyline is KeyLine field for field");
  dst.resize(n);
  if (n) std::memcpy(dst.data(), src, sizeof(plvs_keyline) * (size_t)n);
}
cv::Mat rows32(const uint8_t* desc, int n) {
  return n ? cv::Mat(n, 32, CV_8UC1, const_cast<uint8_t*>(desc)).clone() : cv::Mat();
}
}  // namespace

extern "C" {

// A rectified pair: mvKeyLinesUn = mvKeyLines and mvKeyLinesRightUn = mvKeyLinesRight, as UndistortKeyLines leaves them.
// The matcher's arguments are the function's own: LineMatcher(0.7), TH_LOW_STEREO.
void ref_frame_compute_stereo_line_matches(const plvs_keyline* kl, const uint8_t* desc, int n, const plvs_keyline* klr,
                                           const uint8_t* desc_right, int n_right, const float* level_sigma2, int n_levels,
                                           const float* K4, float mbf, float line_stereo_max_dist, float min_line_length_3d,
                                           float* u_right_start, float* depth_start, float* u_right_end, float* depth_end) {
  Frame F;
  F.Nlines = n;
  fill(F.mvKeyLines, kl, n);
  F.mvKeyLinesUn = F.mvKeyLines;
  fill(F.mvKeyLinesRight, klr, n_right);
  F.mvKeyLinesRightUn = F.mvKeyLinesRight;
  F.mLineDescriptors = rows32(desc, n);
  F.mLineDescriptorsRight = rows32(desc_right, n_right);
  F.mvLineLevelSigma2.assign(level_sigma2, level_sigma2 + n_levels);
  F.mbf = mbf;
  Frame::fx = K4[0]; Frame::fy = K4[1]; Frame::cx = K4[2]; Frame::cy = K4[3];
  Frame::invfx = 1.0f / Frame::fx;   // as the constructor sets them
  Frame::invfy = 1.0f / Frame::fy;
  F.mb = F.mbf / Frame::fx;
  const float keep_len = Frame::skMinLineLength3D, keep_dist = Tracking::skLineStereoMaxDist;
  Frame::skMinLineLength3D = min_line_length_3d;
  Tracking::skLineStereoMaxDist = line_stereo_max_dist;
  F.ComputeStereoLineMatches();
  Frame::skMinLineLength3D = keep_len;
  Tracking::skLineStereoMaxDist = keep_dist;
  for (int i = 0; i < n; ++i) {
    u_right_start[i] = F.mvuRightLineStart[i];
    depth_start[i] = F.mvDepthLineStart[i];
    u_right_end[i] = F.mvuRightLineEnd[i];
    depth_end[i] = F.mvDepthLineEnd[i];
  }
}

}  // extern "C"
