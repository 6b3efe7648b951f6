// C++ host-side mirror of the PLVS interfaces that the hot path hides behind (header only, C++14).
//
// plvs_hip.h is the boundary (C ABI).  This header is what a PLVS translation unit includes to keep
// its own class names, argument meaning and error behaviour while the arithmetic runs in
// libplvs_hip.so.  The reference classes take cv::Mat / pcl::PointCloud / Sophus::SE3f; OpenCV,
// PCL, Eigen and Sophus are not part of this repository, so the mirror takes the plain views of
// those types defined below (same memory layout as the originals: a PLVS build passes
// mat.data / mat.step, cloud.points.data(), Twc.matrix3x4().data() — see INTEGRATION.md).
//
//   PLVS2hip::ORBextractor              include/ORBextractor.h:76-113, src/ORBextractor.cc:446, :1245
//   PLVS2hip::LineExtractor             include/LineExtractor.h:48-83, src/LineExtractor.cc:150, :170
//   PLVS2hip::BinaryDescriptorMatcher   binary_descriptor_matcher_custom.cpp:258
//   PLVS2hip::ORBmatcher                include/ORBmatcher.h (DescriptorDistance, SearchByProjection x2, SearchByBoW)
//   PLVS2hip::LineMatcher               src/LineMatcher.cc:156, :303, :454
//   PLVS2hip::ComputeStereoMatches      src/Frame.cc:1780
//   PLVS2hip::UndistortKeyPoints, ComputeImageBounds, UndistortKeyLines, AssignFeaturesToGrid   src/Frame.cc:1507-1778, :716
//   PLVS2hip::ComputeStereoFromRGBD, ComputeStereoLinesFromRGBD, ComputeSceneMedianDepth, rgbd_frame   src/Frame.cc:2251, :2434, :2730, :401
//   PLVS2hip::IsInFrustum, SearchLocalMap   src/Frame.cc:955, :1033 and src/Tracking.cc:4430-4579 (the local-map link of TrackLocalMap)
//   PLVS2hip::StereoSGM                 Thirdparty/libsgm/include/libsgm.h:57 (as src/PointCloudKeyFrame.cc:435 uses it)
//   PLVS2hip::PointCloudGenerator       src/PointCloudMapping.cc:796, :929
//   PLVS2hip::PointCloudMapChisel       include/PointCloudMapChisel.h:61, src/PointCloudMapChisel.cc:76-246
//   PLVS2hip::PointCloudMapVoxblox      include/PointCloudMapVoxblox.h:54, src/PointCloudMapVoxblox.cc:81
//
// Errors of the library surface as std::runtime_error carrying plvs_hip_last_error(); there is no
// CPU fallback anywhere.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "plvs_hip.h"

namespace PLVS2hip {

inline void check(int rc) {
  if (rc != PLVS_OK) throw std::runtime_error(std::string("plvs_hip: ") + plvs_hip_last_error());
}

// ---- views of the reference's argument types
struct Image8U {      // cv::Mat of type CV_8UC1 (or CV_8UC3 for colour): rows, cols, step, data
  int rows = 0, cols = 0;
  size_t step = 0;
  const uint8_t* data = nullptr;
  bool empty() const { return data == nullptr || rows <= 0 || cols <= 0; }
};
struct Image32F {     // cv::Mat of type CV_32FC1 (depth)
  int rows = 0, cols = 0;
  size_t step = 0;    // bytes, like cv::Mat::step
  const float* data = nullptr;
};
using KeyPoint = plvs_keypoint;             // cv::KeyPoint, field for field
using KeyLine = plvs_keyline;               // cv::line_descriptor_c::KeyLine
using PointSurfelSegment = plvs_point_surfel;   // pcl::PointSurfelSegment, 48 bytes
struct DMatch {                             // cv::DMatch
  int queryIdx = -1, trainIdx = -1, imgIdx = 0;
  float distance = 0.f;
};
struct SE3f {                               // Sophus::SE3f as the 3x4 row-major [R|t] the integrators read
  float m[12];
};

// ------------------------------------------------------------------------------------ ORB
class ORBextractor {
 public:
  ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST) : nfeatures_(nfeatures) {
    check(plvs_hip_orb_create(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, &h_));
  }
  ~ORBextractor() { plvs_hip_orb_destroy(h_); }
  ORBextractor(const ORBextractor&) = delete;
  ORBextractor& operator=(const ORBextractor&) = delete;

  // int operator()(InputArray image, InputArray mask /*ignored*/, vector<KeyPoint>&, OutputArray descriptors,
  //                vector<int>& vLappingArea): returns monoIndex, -1 on an empty image (ORBextractor.cc:1254).
  int operator()(const Image8U& image, std::vector<KeyPoint>& keypoints, std::vector<uint8_t>& descriptors,
                 const std::vector<int>& vLappingArea = {0, 0}) {
    keypoints.clear();
    descriptors.clear();
    if (image.empty()) return -1;
    int cap = 2 * nfeatures_ + 1024, n = 0, mono = 0;
    for (;;) {
      keypoints.resize((size_t)cap);
      descriptors.resize((size_t)cap * 32);
      const int lap0 = vLappingArea.size() > 0 ? vLappingArea[0] : 0, lap1 = vLappingArea.size() > 1 ? vLappingArea[1] : 0;
      const int rc = plvs_hip_orb_extract(h_, image.data, image.cols, image.rows, (int)image.step, lap0, lap1,
                                          keypoints.data(), descriptors.data(), cap, &n, &mono);
      if (rc == PLVS_ERR_EMPTY) { keypoints.clear(); descriptors.clear(); return -1; }
      check(rc);
      if (n > cap) { cap = n; continue; }   // nothing was written: call again with room for n
      break;
    }
    keypoints.resize((size_t)n);
    descriptors.resize((size_t)n * 32);
    return mono;
  }
  int GetLevels() { return plvs_hip_orb_get_levels(h_); }
  float GetScaleFactor() { return plvs_hip_orb_get_scale_factor(h_); }
  std::vector<float> GetScaleFactors() { return table(0); }
  std::vector<float> GetInverseScaleFactors() { return table(1); }
  std::vector<float> GetScaleSigmaSquares() { return table(2); }
  std::vector<float> GetInverseScaleSigmaSquares() { return table(3); }
  plvs_orb* handle() { return h_; }

 private:
  std::vector<float> table(int which) {
    const int n = GetLevels();
    std::vector<float> t[4];
    for (auto& v : t) v.resize((size_t)n);
    check(plvs_hip_orb_get_scale_tables(h_, t[0].data(), t[1].data(), t[2].data(), t[3].data()));
    return t[which];
  }
  plvs_orb* h_ = nullptr;
  int nfeatures_;
};

// ------------------------------------------------------------------------------------ lines
struct LSDOptions {   // LSDDetectorC::LSDOptions (descriptor_custom.hpp:928-957); the EDLines path reads the first four
  int numOctaves = 3;
  float scale = 1.2f;
  double min_length = 0.02;
  double lineFitErrThreshold = 1.6;
  int refine = 2;       // cv::LSD_REFINE_ADV — Tracking passes Line.LSD.refine (1), .logEps (1.0), .densityTh (0.6), Tracking.cc:1476-1482
  double sigma_scale = 0.6, quant = 2.0, ang_th = 22.5, log_eps = 0.0, density_th = 0.7;
  int n_bins = 1024;
  plvs_lsd_options c() const { return plvs_lsd_options{refine, (double)scale, sigma_scale, quant, ang_th, log_eps, density_th, n_bins}; }
};

class LineExtractor {
 public:
  // LineExtractor::skUseLsdExtractor (Line.LSD.on): read when an extractor is constructed, as the reference's mLsd is made
  static bool& UseLsdExtractor() { static bool on = false; return on; }
  LineExtractor(int numLinefeatures, const LSDOptions& opts = LSDOptions()) : n_(numLinefeatures), opts_(opts) {
    check(plvs_hip_lines_create(numLinefeatures, opts.numOctaves, opts.scale, opts.min_length, opts.lineFitErrThreshold, &h_));
    if (UseLsdExtractor()) check(plvs_hip_lsd_create(&lsd_));
  }
  ~LineExtractor() { plvs_hip_lines_destroy(h_); plvs_hip_lsd_destroy(lsd_); }
  LineExtractor(const LineExtractor&) = delete;
  LineExtractor& operator=(const LineExtractor&) = delete;

  // void operator()(const cv::Mat& image, std::vector<KeyLine>& keylines, cv::Mat& descriptors): empty outputs
  // (after "no lines!") when nothing is found, LineExtractor.cc:269-273.
  void operator()(const Image8U& image, std::vector<KeyLine>& keylines, std::vector<uint8_t>& descriptors) {
    int cap = 4096, n = 0;
    for (;;) {
      keylines.resize((size_t)cap);
      descriptors.resize((size_t)cap * 32);
      if (lsd_) {
        const plvs_lsd_options o = opts_.c();
        check(plvs_hip_lsd_extract(lsd_, image.data, image.cols, image.rows, (int)image.step, n_, opts_.numOctaves, &o,
                                   opts_.min_length, keylines.data(), descriptors.data(), cap, &n));
      } else {
        check(plvs_hip_lines_extract(h_, image.data, image.cols, image.rows, (int)image.step, keylines.data(),
                                     descriptors.data(), cap, &n));
      }
      if (n <= cap) break;
      cap = n;   // (nfeatures = 0 keeps every line)
    }
    keylines.resize((size_t)n);
    descriptors.resize((size_t)n * 32);
  }
  // SetGaussianPyramid(mpORBextractor->mvImagePyramid, levels, scale) of Frame::PrecomputeGaussianPyramid: the
  // pyramid stays on the device, so the extractor itself is handed over (nullptr = own pyramid again).
  void SetGaussianPyramid(ORBextractor* orb) {
    if (lsd_) throw std::invalid_argument("LineExtractor: Line.pyramidPrecomputation with Line.LSD.on is undefined behaviour in the reference (DESIGN.md 6), not reproduced");
    check(plvs_hip_lines_set_gaussian_pyramid(h_, orb ? orb->handle() : nullptr));
  }
  plvs_lines* handle() { return h_; }

 private:
  plvs_lines* h_ = nullptr;
  plvs_lsd* lsd_ = nullptr;
  int n_;
  LSDOptions opts_;
};

// ------------------------------------------------------------------------------------ matching
class BinaryDescriptorMatcher {
 public:
  // knnMatch(query, train, matches, k, mask, compactResult), k = 2 as LineMatcher calls it; query / train are
  // N x 32 byte rows.  Masked-out queries give an empty entry, dropped when compactResult.
  void knnMatch(const uint8_t* query, int nq, const uint8_t* train, int nt, std::vector<std::vector<DMatch>>& matches,
                int k = 2, const uint8_t* mask = nullptr, bool compactResult = false) const {
    matches.clear();
    if (k != 2) throw std::invalid_argument("BinaryDescriptorMatcher::knnMatch: only k = 2 is on the accelerated path");
    if (nq <= 0 || nt <= 0) return;   // "empty query or train descriptors", :263-266
    std::vector<int32_t> idx((size_t)2 * nq), dist((size_t)2 * nq);
    check(plvs_hip_hamming_knn2(query, nq, train, nt, mask, PLVS_TIE_MIH, idx.data(), dist.data()));
    for (int q = 0; q < nq; ++q) {
      std::vector<DMatch> row;
      for (int j = 0; j < 2; ++j)
        if (idx[2 * q + j] >= 0) {
          DMatch m;
          m.queryIdx = q;
          m.trainIdx = idx[2 * q + j];
          m.distance = (float)dist[2 * q + j];
          row.push_back(m);
        }
      if (!(compactResult && (mask != nullptr && mask[q] == 0))) matches.push_back(row);
    }
  }
};

// The search functions take the arrays the reference functions read of their Frame / MapPoint / KeyFrame
// objects (plvs_frame_view, plvs_mappoint_view, plvs_lastframe_view, plvs_featvec_view of plvs_hip.h) and
// return the reference's return value; `assigned[i]` is what the reference stores per keypoint (an index
// into the other side, -1 = none) — the caller maps it back to its MapPoint* / MapLine*.
class ORBmatcher {
 public:
  static constexpr int TH_LOW = 50, TH_HIGH = 100, HISTO_LENGTH = 12;
  explicit ORBmatcher(float nnratio = 0.6f, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}

  static int DescriptorDistance(const uint8_t* a, const uint8_t* b) {
    const int32_t z = 0;
    int32_t d = 0;
    check(plvs_hip_hamming_pairs(a, 1, b, 1, &z, &z, 1, &d));
    return d;
  }
  // SearchByProjection(Frame& F, const vector<MapPoint*>& vpMapPoints, th, bFarPoints, thFarPoints), ORBmatcher.cc:71
  int SearchByProjection(const plvs_frame_view& F, const plvs_mappoint_view& vpMapPoints, float th, bool bFarPoints,
                         float thFarPoints, const uint8_t* occupied, std::vector<int32_t>& assigned) const {
    assigned.assign((size_t)F.n, -1);
    int n = 0;
    check(plvs_hip_orb_search_by_projection(&F, &vpMapPoints, th, bFarPoints ? 1 : 0, thFarPoints, mfNNratio, occupied,
                                            assigned.data(), &n));
    return n;
  }
  // SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono), ORBmatcher.cc:1774
  int SearchByProjection(const plvs_frame_view& CurrentFrame, const float* curAngles, float mnMaxX, float mnMaxY, float mbf,
                         const plvs_lastframe_view& LastFrame, float th, bool bForward, bool bBackward,
                         const uint8_t* occupied, std::vector<int32_t>& assigned) const {
    assigned.assign((size_t)CurrentFrame.n, -1);
    int n = 0;
    check(plvs_hip_orb_search_by_projection_ff(&CurrentFrame, curAngles, mnMaxX, mnMaxY, mbf, &LastFrame, th, bForward ? 1 : 0,
                                               bBackward ? 1 : 0, mbCheckOrientation ? 1 : 0, occupied, assigned.data(), &n));
    return n;
  }
  // SearchByBoW(KeyFramePtr& pKF, Frame& F, vpMapPointMatches), ORBmatcher.cc:300
  int SearchByBoW(const plvs_featvec_view& kfFeatVec, const uint8_t* kfDescriptors, int kfN, const uint8_t* kfValid,
                  const float* kfAngles, const plvs_featvec_view& fFeatVec, const uint8_t* fDescriptors, int fN,
                  const float* fAngles, std::vector<int32_t>& assigned) const {
    assigned.assign((size_t)fN, -1);
    int n = 0;
    check(plvs_hip_orb_search_by_bow(&kfFeatVec, kfDescriptors, kfN, kfValid, kfAngles, &fFeatVec, fDescriptors, fN, fAngles,
                                     mfNNratio, mbCheckOrientation ? 1 : 0, assigned.data(), &n));
    return n;
  }
  // The search stage of Fuse(KeyFramePtr& pKF, const vector<MapPointPtr>& vpMapPoints, th, bRight = false), ORBmatcher.cc:1244,
  // for every target key frame of LocalMapping::SearchInNeighbors in one call.  skip (keyFrames.size() x vpMapPoints.m, or
  // null): !pMP || isBad() || IsInKeyFrame(pKF).  bestIdx / bestDist / reached: one entry per (key frame, point), see
  // plvs_hip.h; the mutation of :1408-1427 and its replay in the reference's order are the caller's.
  // onHost: plvs_hip_orb_fuse_search_host (no device call: the replay's re-query of a dirty point).  -> candidates found.
  struct FuseResult {
    std::vector<int32_t> bestIdx, bestDist;
    std::vector<uint8_t> reached;
    int32_t stats[3] = {0, 0, 0};
  };
  int FuseSearch(const std::vector<plvs_fuse_keyframe>& keyFrames, const plvs_fuse_points& vpMapPoints, const uint8_t* skip, float th,
                 FuseResult& result, bool onHost = false, void* stream = nullptr) const {
    const size_t pairs = keyFrames.size() * (size_t)vpMapPoints.m;
    result.bestIdx.assign(pairs + 1, -1);   // (+ 1: the entries refuse null outputs, with nothing to report as well)
    result.bestDist.assign(pairs + 1, -1);
    result.reached.assign(pairs + 1, 0);
    const int K = (int)keyFrames.size();
    if (onHost)
      check(plvs_hip_orb_fuse_search_host(keyFrames.data(), K, &vpMapPoints, skip, th, result.bestIdx.data(), result.bestDist.data(),
                                          result.reached.data(), result.stats));
    else
      check(plvs_hip_orb_fuse_search(keyFrames.data(), K, &vpMapPoints, skip, th, result.bestIdx.data(), result.bestDist.data(),
                                     result.reached.data(), result.stats, stream));
    result.bestIdx.resize(pairs);
    result.bestDist.resize(pairs);
    result.reached.resize(pairs);
    int n = 0;
    for (size_t p = 0; p < pairs; ++p) n += result.bestIdx[p] >= 0 ? 1 : 0;
    return n;
  }
  float mfNNratio;
  bool mbCheckOrientation;
};

class LineMatcher {
 public:
  static constexpr int TH_HIGH = 110, TH_LOW = 60, TH_LOW_STEREO = 50, HISTO_LENGTH = 12;   // LineMatcher.cc:87-90
  explicit LineMatcher(float nnratio = 0.6f, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}
  // SearchByKnn(Frame& CurrentFrame, const Frame& LastFrame), LineMatcher.cc:303
  int SearchByKnn(const uint8_t* descLast, int nLast, const uint8_t* validLast, const float* angleLast,
                  const uint8_t* descCur, int nCur, const float* angleCur, std::vector<int32_t>& assigned) const {
    assigned.assign((size_t)nCur, -1);
    int n = 0;
    check(plvs_hip_lines_search_by_knn(descLast, nLast, validLast, angleLast, descCur, nCur, angleCur, mfNNratio,
                                       mbCheckOrientation ? 1 : 0, assigned.data(), &n));
    return n;
  }
  // SearchByKnn(KeyFramePtr& pKF, const Frame& F, vpMapLineMatches), LineMatcher.cc:156
  int SearchByKnnKF(const uint8_t* descKF, int nKF, const uint8_t* validKF, const float* angleKF, const uint8_t* descF,
                    int nF, const float* angleF, std::vector<int32_t>& assigned) const {
    assigned.assign((size_t)nF, -1);
    int n = 0;
    check(plvs_hip_lines_search_by_knn_kf(descKF, nKF, validKF, angleKF, descF, nF, angleF, mfNNratio,
                                          mbCheckOrientation ? 1 : 0, assigned.data(), &n));
    return n;
  }
  // SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, bLargerSearch, bMono), LineMatcher.cc:837 — the
  // per-frame line match of Tracking::TrackWithMotionModel.  The caller hands over the projections of the last
  // frame's map lines into the current frame (see plvs_hip_lines_search_by_projection_ff); direction: 0, 1 forward,
  // 2 backward.  assigned[i2] = last-frame line whose map line the current line i2 takes, -1 = none.
  int SearchByProjection(const plvs_line_frame_view& CurrentFrame, const uint8_t* occupied, int nLast, const uint8_t* valid,
                         const float* proj, const int32_t* octave, const float* angle, const uint8_t* desc,
                         const uint8_t* hasObservations, bool bLargerSearch, int direction,
                         std::vector<int32_t>& assigned) const {
    assigned.assign((size_t)CurrentFrame.n, -1);
    int n = 0;
    check(plvs_hip_lines_search_by_projection_ff(&CurrentFrame, occupied, nLast, valid, proj, octave, angle, desc,
                                                 hasObservations, bLargerSearch ? 1 : 0, direction, mfNNratio,
                                                 mbCheckOrientation ? 1 : 0, assigned.data(), &n));
    return n;
  }
  // SearchByProjection(Frame& F, const std::vector<MapLinePtr>& vpMapLines, bLargerSearch), LineMatcher.cc:1286 —
  // Tracking::SearchLocalLines.  assigned[i2] = map line the frame line i2 takes, -1 = none.
  int SearchByProjection(const plvs_line_frame_view& F, const uint8_t* occupied, int nMapLines, const uint8_t* inView,
                         const float* proj, const int32_t* level, const uint8_t* desc, const uint8_t* hasObservations,
                         bool bLargerSearch, std::vector<int32_t>& assigned) const {
    assigned.assign((size_t)F.n, -1);
    int n = 0;
    check(plvs_hip_lines_search_by_projection(&F, occupied, nMapLines, inView, proj, level, desc, hasObservations,
                                              bLargerSearch ? 1 : 0, mfNNratio, assigned.data(), &n));
    return n;
  }
  // SearchStereoMatchesByKnn(frame, vMatches, vValidMatches, descriptorDist), LineMatcher.cc:454
  int SearchStereoMatchesByKnn(const uint8_t* descLeft, int nLeft, const float* angleLeft, const int32_t* octaveLeft,
                               const uint8_t* descRight, int nRight, const float* angleRight, const int32_t* octaveRight,
                               std::vector<DMatch>& vMatches, std::vector<bool>& vValidMatches,
                               int descriptorDist = TH_LOW_STEREO) const {
    const int cap = nRight > 0 ? nRight : 1;
    std::vector<int32_t> q((size_t)cap), t((size_t)cap);
    std::vector<float> d((size_t)cap);
    std::vector<uint8_t> v((size_t)cap);
    int k = 0, n = 0;
    check(plvs_hip_lines_search_stereo_by_knn(descLeft, nLeft, angleLeft, octaveLeft, descRight, nRight, angleRight,
                                              octaveRight, mfNNratio, mbCheckOrientation ? 1 : 0, descriptorDist, q.data(),
                                              t.data(), d.data(), v.data(), cap, &k, &n));
    vMatches.clear();
    vValidMatches.clear();
    for (int i = 0; i < k; ++i) {
      DMatch m;
      m.queryIdx = q[(size_t)i]; m.trainIdx = t[(size_t)i]; m.distance = d[(size_t)i];
      vMatches.push_back(m);
      vValidMatches.push_back(v[(size_t)i] != 0);
    }
    return n;
  }
  // The search stage of Fuse(KeyFramePtr& pKF, const vector<MapLinePtr>& vpMapLines, th, bRight = false), LineMatcher.cc:2043,
  // for every target key frame of LocalMapping::SearchInNeighbors in one call.  skip (keyFrames.size() x vpMapLines.m, or
  // null): !pML || isBad() || IsInKeyFrame(pKF).  bestIdx / bestDist / reached: one entry per (key frame, line), see
  // plvs_hip.h; the mutation of :2279-2306 and its replay in the reference's order are the caller's.
  // onHost: plvs_hip_line_fuse_search_host (no device call: the replay's re-query of a dirty line).  -> candidates found.
  struct FuseResult {
    std::vector<int32_t> bestIdx, bestDist;
    std::vector<uint8_t> reached;
    int32_t stats[3] = {0, 0, 0};
    void prepare(size_t pairs) {   // (+ 1: the entries refuse null outputs, with nothing to report as well)
      bestIdx.assign(pairs + 1, -1);
      bestDist.assign(pairs + 1, -1);
      reached.assign(pairs + 1, 0);
    }
    int finish(size_t pairs) {
      bestIdx.resize(pairs);
      bestDist.resize(pairs);
      reached.resize(pairs);
      int n = 0;
      for (size_t p = 0; p < pairs; ++p) n += bestIdx[p] >= 0 ? 1 : 0;
      return n;
    }
  };
  int FuseSearch(const std::vector<plvs_line_fuse_keyframe>& keyFrames, const plvs_fuse_lines& vpMapLines, const uint8_t* skip, float th,
                 FuseResult& result, bool onHost = false, void* stream = nullptr) const {
    const size_t pairs = keyFrames.size() * (size_t)vpMapLines.m;
    result.prepare(pairs);
    const int K = (int)keyFrames.size();
    if (onHost)
      check(plvs_hip_line_fuse_search_host(keyFrames.data(), K, &vpMapLines, skip, th, result.bestIdx.data(), result.bestDist.data(),
                                           result.reached.data(), result.stats));
    else
      check(plvs_hip_line_fuse_search(keyFrames.data(), K, &vpMapLines, skip, th, result.bestIdx.data(), result.bestDist.data(),
                                      result.reached.data(), result.stats, stream));
    return result.finish(pairs);
  }
  float mfNNratio;
  bool mbCheckOrientation;
};

// Both halves of LocalMapping::SearchInNeighbors' search (ORBmatcher::FuseSearch and LineMatcher::FuseSearch) in one call with
// ONE device wait: plvs_hip_fuse_search_points_and_lines.  stats: launches, waits.  -> candidates found, points + lines.
inline int FuseSearchPointsAndLines(const std::vector<plvs_fuse_keyframe>& pointKeyFrames, const plvs_fuse_points& vpMapPoints,
                                    const uint8_t* skipPoints, float thPoints, ORBmatcher::FuseResult& points,
                                    const std::vector<plvs_line_fuse_keyframe>& lineKeyFrames, const plvs_fuse_lines& vpMapLines,
                                    const uint8_t* skipLines, float thLines, LineMatcher::FuseResult& lines, int32_t stats[2] = nullptr,
                                    void* stream = nullptr) {
  const size_t pp = pointKeyFrames.size() * (size_t)vpMapPoints.m, lp = lineKeyFrames.size() * (size_t)vpMapLines.m;
  points.bestIdx.assign(pp + 1, -1);
  points.bestDist.assign(pp + 1, -1);
  points.reached.assign(pp + 1, 0);
  lines.prepare(lp);
  check(plvs_hip_fuse_search_points_and_lines(pointKeyFrames.data(), (int)pointKeyFrames.size(), &vpMapPoints, skipPoints, thPoints,
                                              points.bestIdx.data(), points.bestDist.data(), points.reached.data(), points.stats,
                                              lineKeyFrames.data(), (int)lineKeyFrames.size(), &vpMapLines, skipLines, thLines,
                                              lines.bestIdx.data(), lines.bestDist.data(), lines.reached.data(), lines.stats, stats, stream));
  points.bestIdx.resize(pp);
  points.bestDist.resize(pp);
  points.reached.resize(pp);
  int n = lines.finish(lp);
  for (size_t p = 0; p < pp; ++p) n += points.bestIdx[p] >= 0 ? 1 : 0;
  return n;
}

// A key frame resident in HBM (plvs_keyframe): what the Fuse searches read of a KeyFrame that its constructor fixes, copied once.
// Create it where the KeyFrame constructor ends, let it go with the key frame (or on SetBadFlag); the pose travels with each call
// (nothing to do on SetPose).  Move-only; immutable, so any number of threads may search with it; destroying it while another
// thread's call uses it is the caller's error.  hostOnly: no device call, ever (the onHost searches alone take such a handle).
class KeyFrameHandle {
 public:
  KeyFrameHandle() = default;
  KeyFrameHandle(const plvs_fuse_keyframe* points, const plvs_line_fuse_keyframe* lines, bool hostOnly = false) {
    check(plvs_hip_keyframe_create(points, lines, hostOnly ? PLVS_KEYFRAME_HOST_ONLY : 0u, &h_));
  }
  // with the BoW side (what KeyFrame::ComputeBoW fixes; BowSearch below flattens a DBoW2::FeatureVector into `bow`)
  KeyFrameHandle(const plvs_fuse_keyframe* points, const plvs_line_fuse_keyframe* lines, const plvs_keyframe_bow* bow, bool hostOnly = false) {
    check(plvs_hip_keyframe_create_bow(points, lines, bow, hostOnly ? PLVS_KEYFRAME_HOST_ONLY : 0u, &h_));
  }
  ~KeyFrameHandle() { reset(); }
  KeyFrameHandle(KeyFrameHandle&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  KeyFrameHandle& operator=(KeyFrameHandle&& o) noexcept {
    if (this != &o) { reset(); h_ = o.h_; o.h_ = nullptr; }
    return *this;
  }
  KeyFrameHandle(const KeyFrameHandle&) = delete;
  KeyFrameHandle& operator=(const KeyFrameHandle&) = delete;
  void reset() {
    if (h_) (void)plvs_hip_keyframe_destroy(h_);
    h_ = nullptr;
  }
  const plvs_keyframe* get() const { return h_; }
  explicit operator bool() const { return h_ != nullptr; }
  // key points (-1: none), key lines (-1: none), device bytes, host bytes, flags, device id
  struct Info { int64_t nPoints, nLines, deviceBytes, hostBytes, flags, device; };
  Info info() const {
    int64_t v[6];
    check(plvs_hip_keyframe_info(h_, v));
    return Info{v[0], v[1], v[2], v[3], v[4], v[5]};
  }
  // vocabulary nodes (-1: no BoW side), listed features, the longest node list, bytes the side adds to the device allocation
  struct BowInfo { int64_t nodes, listed, longest, deviceBytes; };
  BowInfo bowInfo() const {
    int64_t v[4];
    check(plvs_hip_keyframe_bow_info(h_, v));
    return BowInfo{v[0], v[1], v[2], v[3]};
  }

 private:
  plvs_keyframe* h_ = nullptr;
};

namespace detail {
template <typename Pose>
inline std::vector<const plvs_keyframe*> raw_handles(const std::vector<const KeyFrameHandle*>& keyFrames, const std::vector<Pose>& poses) {
  if (keyFrames.size() != poses.size()) throw std::invalid_argument("FuseSearch: one pose per key frame handle");
  std::vector<const plvs_keyframe*> raw(keyFrames.size() + 1, nullptr);
  for (size_t k = 0; k < keyFrames.size(); ++k) raw[k] = keyFrames[k] ? keyFrames[k]->get() : nullptr;
  return raw;
}
}  // namespace detail

// ORBmatcher::FuseSearch / LineMatcher::FuseSearch / FuseSearchPointsAndLines over resident key frames: key frame k =
// (keyFrames[k], poses[k]); the same handle may be listed more than once.  copyInBytes (may be null): the bytes of the call's one
// host-to-device copy — the per-call table, the map points or lines, skip.  Results as the non-resident overloads'.
inline int FuseSearch(const std::vector<const KeyFrameHandle*>& keyFrames, const std::vector<plvs_keyframe_pose>& poses,
                      const plvs_fuse_points& vpMapPoints, const uint8_t* skip, float th, ORBmatcher::FuseResult& result, bool onHost = false,
                      void* stream = nullptr, int32_t* copyInBytes = nullptr) {
  const std::vector<const plvs_keyframe*> raw = detail::raw_handles(keyFrames, poses);
  const int K = (int)keyFrames.size();
  const size_t pairs = keyFrames.size() * (size_t)vpMapPoints.m;
  result.bestIdx.assign(pairs + 1, -1);
  result.bestDist.assign(pairs + 1, -1);
  result.reached.assign(pairs + 1, 0);
  int32_t st[4] = {0, 0, 0, 0};
  if (onHost)
    check(plvs_hip_orb_fuse_search_kf_host(raw.data(), poses.data(), K, &vpMapPoints, skip, th, result.bestIdx.data(), result.bestDist.data(),
                                           result.reached.data(), st));
  else
    check(plvs_hip_orb_fuse_search_kf(raw.data(), poses.data(), K, &vpMapPoints, skip, th, result.bestIdx.data(), result.bestDist.data(),
                                      result.reached.data(), st, stream));
  for (int s = 0; s < 3; ++s) result.stats[s] = st[s];
  if (copyInBytes) *copyInBytes = st[3];
  result.bestIdx.resize(pairs);
  result.bestDist.resize(pairs);
  result.reached.resize(pairs);
  int n = 0;
  for (size_t p = 0; p < pairs; ++p) n += result.bestIdx[p] >= 0 ? 1 : 0;
  return n;
}
inline int FuseSearch(const std::vector<const KeyFrameHandle*>& keyFrames, const std::vector<plvs_keyframe_pose>& poses,
                      const plvs_fuse_lines& vpMapLines, const uint8_t* skip, float th, LineMatcher::FuseResult& result, bool onHost = false,
                      void* stream = nullptr, int32_t* copyInBytes = nullptr) {
  const std::vector<const plvs_keyframe*> raw = detail::raw_handles(keyFrames, poses);
  const int K = (int)keyFrames.size();
  const size_t pairs = keyFrames.size() * (size_t)vpMapLines.m;
  result.prepare(pairs);
  int32_t st[4] = {0, 0, 0, 0};
  if (onHost)
    check(plvs_hip_line_fuse_search_kf_host(raw.data(), poses.data(), K, &vpMapLines, skip, th, result.bestIdx.data(), result.bestDist.data(),
                                            result.reached.data(), st));
  else
    check(plvs_hip_line_fuse_search_kf(raw.data(), poses.data(), K, &vpMapLines, skip, th, result.bestIdx.data(), result.bestDist.data(),
                                       result.reached.data(), st, stream));
  for (int s = 0; s < 3; ++s) result.stats[s] = st[s];
  if (copyInBytes) *copyInBytes = st[3];
  return result.finish(pairs);
}
// stats (3 entries, may be null): launches, waits, bytes of the copy in
inline int FuseSearchPointsAndLines(const std::vector<const KeyFrameHandle*>& keyFrames, const std::vector<plvs_keyframe_pose>& poses,
                                    const plvs_fuse_points& vpMapPoints, const uint8_t* skipPoints, float thPoints,
                                    ORBmatcher::FuseResult& points, const plvs_fuse_lines& vpMapLines, const uint8_t* skipLines, float thLines,
                                    LineMatcher::FuseResult& lines, int32_t stats[3] = nullptr, void* stream = nullptr) {
  const std::vector<const plvs_keyframe*> raw = detail::raw_handles(keyFrames, poses);
  const size_t pp = keyFrames.size() * (size_t)vpMapPoints.m, lp = keyFrames.size() * (size_t)vpMapLines.m;
  points.bestIdx.assign(pp + 1, -1);
  points.bestDist.assign(pp + 1, -1);
  points.reached.assign(pp + 1, 0);
  lines.prepare(lp);
  int32_t ps[4] = {0, 0, 0, 0}, ls[4] = {0, 0, 0, 0};
  check(plvs_hip_fuse_search_points_and_lines_kf(raw.data(), poses.data(), (int)keyFrames.size(), &vpMapPoints, skipPoints, thPoints,
                                                 points.bestIdx.data(), points.bestDist.data(), points.reached.data(), ps, &vpMapLines,
                                                 skipLines, thLines, lines.bestIdx.data(), lines.bestDist.data(), lines.reached.data(), ls,
                                                 stats, stream));
  for (int s = 0; s < 3; ++s) { points.stats[s] = ps[s]; lines.stats[s] = ls[s]; }
  points.bestIdx.resize(pp);
  points.bestDist.resize(pp);
  points.reached.resize(pp);
  int n = lines.finish(lp);
  for (size_t p = 0; p < pp; ++p) n += points.bestIdx[p] >= 0 ? 1 : 0;
  return n;
}

// The Sim3 Fuse searches of LoopClosing::SearchAndFuse (ORBmatcher::Fuse / LineMatcher::Fuse with Scw, src/ORBmatcher.cc:1437-1553,
// src/LineMatcher.cc:2321-2561) over resident key frames: key frame k = (keyFrames[k], poses[k]), the caller's own decomposition of
// Scw (plvs_hip.h: plvs_keyframe_sim3_pose).  skip: isBad() || spAlreadyFound.count() at the time of the call.  Results, onHost,
// stream and copyInBytes as FuseSearch over handles.
inline int LoopFuseSearch(const std::vector<const KeyFrameHandle*>& keyFrames, const std::vector<plvs_keyframe_sim3_pose>& poses,
                          const plvs_fuse_points& vpPoints, const uint8_t* skip, float th, ORBmatcher::FuseResult& result, bool onHost = false,
                          void* stream = nullptr, int32_t* copyInBytes = nullptr) {
  const std::vector<const plvs_keyframe*> raw = detail::raw_handles(keyFrames, poses);
  const int K = (int)keyFrames.size();
  const size_t pairs = keyFrames.size() * (size_t)vpPoints.m;
  result.bestIdx.assign(pairs + 1, -1);
  result.bestDist.assign(pairs + 1, -1);
  result.reached.assign(pairs + 1, 0);
  int32_t st[4] = {0, 0, 0, 0};
  if (onHost)
    check(plvs_hip_orb_loop_fuse_search_kf_host(raw.data(), poses.data(), K, &vpPoints, skip, th, result.bestIdx.data(), result.bestDist.data(),
                                                result.reached.data(), st));
  else
    check(plvs_hip_orb_loop_fuse_search_kf(raw.data(), poses.data(), K, &vpPoints, skip, th, result.bestIdx.data(), result.bestDist.data(),
                                           result.reached.data(), st, stream));
  for (int s = 0; s < 3; ++s) result.stats[s] = st[s];
  if (copyInBytes) *copyInBytes = st[3];
  result.bestIdx.resize(pairs);
  result.bestDist.resize(pairs);
  result.reached.resize(pairs);
  int n = 0;
  for (size_t p = 0; p < pairs; ++p) n += result.bestIdx[p] >= 0 ? 1 : 0;
  return n;
}
inline int LoopFuseSearch(const std::vector<const KeyFrameHandle*>& keyFrames, const std::vector<plvs_keyframe_sim3_pose>& poses,
                          const plvs_fuse_lines& vpLines, const uint8_t* skip, float th, LineMatcher::FuseResult& result, bool onHost = false,
                          void* stream = nullptr, int32_t* copyInBytes = nullptr) {
  const std::vector<const plvs_keyframe*> raw = detail::raw_handles(keyFrames, poses);
  const int K = (int)keyFrames.size();
  const size_t pairs = keyFrames.size() * (size_t)vpLines.m;
  result.prepare(pairs);
  int32_t st[4] = {0, 0, 0, 0};
  if (onHost)
    check(plvs_hip_line_loop_fuse_search_kf_host(raw.data(), poses.data(), K, &vpLines, skip, th, result.bestIdx.data(), result.bestDist.data(),
                                                 result.reached.data(), st));
  else
    check(plvs_hip_line_loop_fuse_search_kf(raw.data(), poses.data(), K, &vpLines, skip, th, result.bestIdx.data(), result.bestDist.data(),
                                            result.reached.data(), st, stream));
  for (int s = 0; s < 3; ++s) result.stats[s] = st[s];
  if (copyInBytes) *copyInBytes = st[3];
  return result.finish(pairs);
}
// both in one call; stats (3 entries, may be null): launches, waits, bytes of the copy in
inline int LoopFuseSearchPointsAndLines(const std::vector<const KeyFrameHandle*>& keyFrames, const std::vector<plvs_keyframe_sim3_pose>& poses,
                                        const plvs_fuse_points& vpPoints, const uint8_t* skipPoints, float thPoints,
                                        ORBmatcher::FuseResult& points, const plvs_fuse_lines& vpLines, const uint8_t* skipLines, float thLines,
                                        LineMatcher::FuseResult& lines, int32_t stats[3] = nullptr, void* stream = nullptr) {
  const std::vector<const plvs_keyframe*> raw = detail::raw_handles(keyFrames, poses);
  const size_t pp = keyFrames.size() * (size_t)vpPoints.m, lp = keyFrames.size() * (size_t)vpLines.m;
  points.bestIdx.assign(pp + 1, -1);
  points.bestDist.assign(pp + 1, -1);
  points.reached.assign(pp + 1, 0);
  lines.prepare(lp);
  int32_t ps[4] = {0, 0, 0, 0}, ls[4] = {0, 0, 0, 0};
  check(plvs_hip_loop_fuse_search_points_and_lines_kf(raw.data(), poses.data(), (int)keyFrames.size(), &vpPoints, skipPoints, thPoints,
                                                      points.bestIdx.data(), points.bestDist.data(), points.reached.data(), ps, &vpLines,
                                                      skipLines, thLines, lines.bestIdx.data(), lines.bestDist.data(), lines.reached.data(), ls,
                                                      stats, stream));
  for (int s = 0; s < 3; ++s) { points.stats[s] = ps[s]; lines.stats[s] = ls[s]; }
  points.bestIdx.resize(pp);
  points.bestDist.resize(pp);
  points.reached.resize(pp);
  int n = lines.finish(lp);
  for (size_t p = 0; p < pp; ++p) n += points.bestIdx[p] >= 0 ? 1 : 0;
  return n;
}

// Loop detection: the SearchByProjection(pKF, Scw, ...) overloads of ORBmatcher (src/ORBmatcher.cc:509-615, :617-730) and LineMatcher
// (src/LineMatcher.cc:1767-1909, :1913-2037) over resident key frames: key frame k = (keyFrames[k], poses[k]) and ONE list of map
// points or lines (plvs_hip.h has the semantics).  matchIdx[k * m + i]: the key point or key line that vpMatched[...] = vpPoints[i]
// was written to, else -1 — the caller stores vpMatched (and, with the KF overloads, vpMatchedKF) from it.
struct LoopSearchResult {
  std::vector<int32_t> matchIdx, matchDist;   // K x M
  std::vector<uint8_t> reached;               // K x M, PLVS_FUSE_* / PLVS_LINE_FUSE_*
  std::vector<int32_t> nmatches;              // K: the reference's return values
  int32_t stats[5] = {0, 0, 0, 0, 0};         // host-decided pairs, pairs at a window, launches, copy-in bytes, lists recomputed
  void prepare(size_t pairs, size_t kfs) {
    matchIdx.assign(pairs + 1, -1);
    matchDist.assign(pairs + 1, -1);
    reached.assign(pairs + 1, 0);
    nmatches.assign(kfs + 1, 0);
  }
  int finish(size_t pairs, size_t kfs) {
    matchIdx.resize(pairs);
    matchDist.resize(pairs);
    reached.resize(pairs);
    nmatches.resize(kfs);
    int n = 0;
    for (int32_t v : nmatches) n += v;
    return n;
  }
};
namespace detail {
// occupied: empty, or one entry per key frame (an empty entry: NULL — nothing of that key frame's vpMatched is set on entry)
inline std::vector<const uint8_t*> occupied_pointers(const std::vector<std::vector<uint8_t>>& occupied, size_t kfs) {
  if (!occupied.empty() && occupied.size() != kfs) throw std::invalid_argument("LoopSearchByProjection: one occupied entry per key frame, or none");
  std::vector<const uint8_t*> p(occupied.size());
  for (size_t k = 0; k < occupied.size(); ++k) p[k] = occupied[k].empty() ? nullptr : occupied[k].data();
  return p;
}
}  // namespace detail
// projection: PLVS_LOOP_PROJECT_CAMERA (the overload without vpPointsKFs) or PLVS_LOOP_PROJECT_INVZ (the one with).  -> the matches
// of all key frames
inline int LoopSearchByProjection(const std::vector<const KeyFrameHandle*>& keyFrames, const std::vector<plvs_keyframe_sim3_pose>& poses,
                                  const plvs_fuse_points& vpPoints, const uint8_t* skip, const std::vector<std::vector<uint8_t>>& occupied,
                                  float th, float ratioHamming, int projection, LoopSearchResult& result, bool onHost = false,
                                  void* stream = nullptr) {
  const std::vector<const plvs_keyframe*> raw = detail::raw_handles(keyFrames, poses);
  const std::vector<const uint8_t*> occ = detail::occupied_pointers(occupied, keyFrames.size());
  const int K = (int)keyFrames.size();
  const size_t pairs = keyFrames.size() * (size_t)vpPoints.m;
  result.prepare(pairs, keyFrames.size());
  if (onHost)
    check(plvs_hip_orb_loop_search_by_projection_kf_host(raw.data(), poses.data(), K, &vpPoints, skip, occ.empty() ? nullptr : occ.data(), th,
                                                         ratioHamming, projection, result.matchIdx.data(), result.matchDist.data(),
                                                         result.reached.data(), result.nmatches.data(), result.stats));
  else
    check(plvs_hip_orb_loop_search_by_projection_kf(raw.data(), poses.data(), K, &vpPoints, skip, occ.empty() ? nullptr : occ.data(), th,
                                                    ratioHamming, projection, result.matchIdx.data(), result.matchDist.data(),
                                                    result.reached.data(), result.nmatches.data(), result.stats, stream));
  return result.finish(pairs, keyFrames.size());
}
inline int LoopSearchByProjection(const std::vector<const KeyFrameHandle*>& keyFrames, const std::vector<plvs_keyframe_sim3_pose>& poses,
                                  const plvs_fuse_lines& vpLines, const uint8_t* skip, const std::vector<std::vector<uint8_t>>& occupied,
                                  float th, float ratioHamming, LoopSearchResult& result, bool onHost = false, void* stream = nullptr) {
  const std::vector<const plvs_keyframe*> raw = detail::raw_handles(keyFrames, poses);
  const std::vector<const uint8_t*> occ = detail::occupied_pointers(occupied, keyFrames.size());
  const int K = (int)keyFrames.size();
  const size_t pairs = keyFrames.size() * (size_t)vpLines.m;
  result.prepare(pairs, keyFrames.size());
  if (onHost)
    check(plvs_hip_line_loop_search_by_projection_kf_host(raw.data(), poses.data(), K, &vpLines, skip, occ.empty() ? nullptr : occ.data(), th,
                                                          ratioHamming, result.matchIdx.data(), result.matchDist.data(), result.reached.data(),
                                                          result.nmatches.data(), result.stats));
  else
    check(plvs_hip_line_loop_search_by_projection_kf(raw.data(), poses.data(), K, &vpLines, skip, occ.empty() ? nullptr : occ.data(), th,
                                                     ratioHamming, result.matchIdx.data(), result.matchDist.data(), result.reached.data(),
                                                     result.nmatches.data(), result.stats, stream));
  return result.finish(pairs, keyFrames.size());
}
// both in one call (every reference call site passes an all-null vpMatched: no `occupied` here); stats (3 entries, may be null):
// launches, waits, bytes of the copy in
inline int LoopSearchByProjectionPointsAndLines(const std::vector<const KeyFrameHandle*>& keyFrames,
                                                const std::vector<plvs_keyframe_sim3_pose>& poses, const plvs_fuse_points& vpPoints,
                                                const uint8_t* skipPoints, float thPoints, float ratioHammingPoints, int projection,
                                                LoopSearchResult& points, const plvs_fuse_lines& vpLines, const uint8_t* skipLines,
                                                float thLines, float ratioHammingLines, LoopSearchResult& lines, int32_t stats[3] = nullptr,
                                                void* stream = nullptr) {
  const std::vector<const plvs_keyframe*> raw = detail::raw_handles(keyFrames, poses);
  const size_t pp = keyFrames.size() * (size_t)vpPoints.m, lp = keyFrames.size() * (size_t)vpLines.m;
  points.prepare(pp, keyFrames.size());
  lines.prepare(lp, keyFrames.size());
  check(plvs_hip_loop_search_by_projection_points_and_lines_kf(
      raw.data(), poses.data(), (int)keyFrames.size(), &vpPoints, skipPoints, nullptr, thPoints, ratioHammingPoints, projection,
      points.matchIdx.data(), points.matchDist.data(), points.reached.data(), points.nmatches.data(), points.stats, &vpLines, skipLines, nullptr,
      thLines, ratioHammingLines, lines.matchIdx.data(), lines.matchDist.data(), lines.reached.data(), lines.nmatches.data(), lines.stats, stats,
      stream));
  return points.finish(pp, keyFrames.size()) + lines.finish(lp, keyFrames.size());
}

// ORBmatcher::SearchByBoW over resident key frames (plvs_hip.h has the semantics): SearchByBoW(pKF1, pKF2[k], vpMatches12[k]) for
// every covisible of a loop candidate, and SearchByBoW(pKF[k], F, vvpMapPointMatches[k]) for every relocalisation candidate, each in
// one call.  A DBoW2::FeatureVector IS a std::map<NodeId, std::vector<unsigned int>>: the mirror flattens its in-order traversal.
struct FlatFeatureVector {
  std::vector<uint32_t> nodeId;
  std::vector<int32_t> offset;
  std::vector<uint32_t> index;
  FlatFeatureVector() : offset(1, 0) {}
  explicit FlatFeatureVector(const std::map<unsigned int, std::vector<unsigned int>>& featVec) : offset(1, 0) {
    for (const auto& node : featVec) {
      nodeId.push_back(node.first);
      index.insert(index.end(), node.second.begin(), node.second.end());
      offset.push_back((int32_t)index.size());
    }
  }
  plvs_featvec_view view() const { return plvs_featvec_view{(int32_t)nodeId.size(), nodeId.data(), offset.data(), index.data()}; }
};
class BowSearch {
 public:
  BowSearch(float nnratio = 0.6f, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}   // ORBmatcher's constructor
  // the handle of a key frame with its BoW side: mFeatVec and mvKeysUn[i].angle (degrees)
  static KeyFrameHandle MakeKeyFrame(const plvs_fuse_keyframe& points, const plvs_line_fuse_keyframe* lines,
                                     const std::map<unsigned int, std::vector<unsigned int>>& mFeatVec, const std::vector<float>& angles,
                                     bool hostOnly = false) {
    const FlatFeatureVector flat(mFeatVec);
    const plvs_keyframe_bow bow{flat.view(), angles.data()};
    return KeyFrameHandle(&points, lines, &bow, hostOnly);
  }
  struct Result {
    std::vector<int32_t> match, matchDist;   // K x n: matchIdx of the key-frame kind, assigned of the frame kind
    std::vector<int32_t> nmatches;           // K: the reference's return values
    int32_t stats[6] = {0, 0, 0, 0, 0, 0};   // launches, waits, copy-in bytes, jobs, jobs beyond one pass, jobs handed to the host
  };
  // valid1[i], valid2[k][j]: vpMapPoints[i] && !isBad().  result.match[k * n1 + i1]: the key point of keyFrames2[k] whose map point
  // vpMatches12[i1] holds.  -> the matches of all pairs
  int SearchByBoW(const KeyFrameHandle& kf1, const std::vector<uint8_t>& valid1, const std::vector<const KeyFrameHandle*>& keyFrames2,
                  const std::vector<std::vector<uint8_t>>& valid2, Result& result, bool onHost = false, void* stream = nullptr) const {
    if (valid2.size() != keyFrames2.size()) throw std::invalid_argument("SearchByBoW: one validity array per key frame");
    const size_t K = keyFrames2.size(), n1 = (size_t)std::max<int64_t>(kf1.info().nPoints, 0);
    std::vector<const plvs_keyframe*> raw(K + 1, nullptr);
    std::vector<const uint8_t*> valid(K + 1, nullptr);
    for (size_t k = 0; k < K; ++k) { raw[k] = keyFrames2[k] ? keyFrames2[k]->get() : nullptr; valid[k] = valid2[k].data(); }
    prepare(result, K, n1);
    if (onHost)
      check(plvs_hip_orb_search_by_bow_kf_host(kf1.get(), valid1.data(), raw.data(), valid.data(), (int)K, mfNNratio, mbCheckOrientation ? 1 : 0,
                                               result.match.data(), result.matchDist.data(), result.nmatches.data(), result.stats));
    else
      check(plvs_hip_orb_search_by_bow_kf(kf1.get(), valid1.data(), raw.data(), valid.data(), (int)K, mfNNratio, mbCheckOrientation ? 1 : 0,
                                          result.match.data(), result.matchDist.data(), result.nmatches.data(), result.stats, stream));
    return finish(result, K, n1);
  }
  // F: mDescriptors (n x 32), mvKeys[i].angle, mFeatVec.  result.match[k * n + iF]: the key point of keyFrames[k] whose map point goes to
  // vvpMapPointMatches[k][iF]
  int SearchByBoW(const std::vector<const KeyFrameHandle*>& keyFrames, const std::vector<std::vector<uint8_t>>& kfValid,
                  const uint8_t* fDescriptors, const std::vector<float>& fAngles, const std::map<unsigned int, std::vector<unsigned int>>& fFeatVec,
                  Result& result, bool onHost = false, void* stream = nullptr) const {
    if (kfValid.size() != keyFrames.size()) throw std::invalid_argument("SearchByBoW: one validity array per key frame");
    const size_t K = keyFrames.size(), n = fAngles.size();
    const FlatFeatureVector flat(fFeatVec);
    const plvs_bow_frame F{(int32_t)n, fDescriptors, fAngles.data(), flat.view()};
    std::vector<const plvs_keyframe*> raw(K + 1, nullptr);
    std::vector<const uint8_t*> valid(K + 1, nullptr);
    for (size_t k = 0; k < K; ++k) { raw[k] = keyFrames[k] ? keyFrames[k]->get() : nullptr; valid[k] = kfValid[k].data(); }
    prepare(result, K, n);
    if (onHost)
      check(plvs_hip_orb_search_by_bow_frame_kf_host(raw.data(), valid.data(), (int)K, &F, mfNNratio, mbCheckOrientation ? 1 : 0,
                                                     result.match.data(), result.matchDist.data(), result.nmatches.data(), result.stats));
    else
      check(plvs_hip_orb_search_by_bow_frame_kf(raw.data(), valid.data(), (int)K, &F, mfNNratio, mbCheckOrientation ? 1 : 0, result.match.data(),
                                                result.matchDist.data(), result.nmatches.data(), result.stats, stream));
    return finish(result, K, n);
  }

 private:
  static void prepare(Result& r, size_t K, size_t n) {
    r.match.assign(K * n + 1, -1);
    r.matchDist.assign(K * n + 1, -1);
    r.nmatches.assign(K + 1, 0);
  }
  static int finish(Result& r, size_t K, size_t n) {
    r.match.resize(K * n);
    r.matchDist.resize(K * n);
    r.nmatches.resize(K);
    int total = 0;
    for (int32_t v : r.nmatches) total += v;
    return total;
  }
  float mfNNratio;
  bool mbCheckOrientation;
};

// Frame::ComputeStereoMatches: mvuRight / mvDepth of the left keypoints (-1 = none).
inline void ComputeStereoMatches(ORBextractor& left, ORBextractor& right, const std::vector<KeyPoint>& mvKeys,
                                 const std::vector<uint8_t>& mDescriptors, const std::vector<KeyPoint>& mvKeysRight,
                                 const std::vector<uint8_t>& mDescriptorsRight, float mb, float mbf,
                                 std::vector<float>& mvuRight, std::vector<float>& mvDepth) {
  plvs_stereo* s = nullptr;
  check(plvs_hip_stereo_create(left.handle(), right.handle(), &s));
  mvuRight.assign(mvKeys.size(), -1.0f);
  mvDepth.assign(mvKeys.size(), -1.0f);
  int n = 0;
  const int rc = plvs_hip_stereo_matches(s, mvKeys.data(), mDescriptors.data(), (int)mvKeys.size(), mvKeysRight.data(),
                                         mDescriptorsRight.data(), (int)mvKeysRight.size(), mb, mbf, mvuRight.data(),
                                         mvDepth.data(), &n);
  plvs_hip_stereo_destroy(s);
  check(rc);
}

// ------------------------------------------------------------------------------------ frame glue
// What Frame::Frame runs between extraction and the first search (src/Frame.cc:541-580), as free functions over the vectors
// a Frame holds.  K4 = fx, fy, cx, cy; dist = mDistCoef (0, 4, 5 or 8 coefficients; empty / first one zero: no distortion).
inline void UndistortKeyPoints(const std::vector<KeyPoint>& mvKeys, const float* K4, const std::vector<float>& dist,
                               std::vector<KeyPoint>& mvKeysUn) {   // :1507-1552
  mvKeysUn.resize(mvKeys.size());
  check(plvs_hip_frame_undistort_keypoints(mvKeys.data(), (int)mvKeys.size(), K4, dist.data(), (int)dist.size(), mvKeysUn.data()));
}
struct ImageBounds {
  float mnMinX, mnMaxX, mnMinY, mnMaxY, mnMaxDiag;
};
inline ImageBounds ComputeImageBounds(int width, int height, const float* K4, const std::vector<float>& dist) {   // :1749-1778
  float b[5];
  check(plvs_hip_frame_compute_image_bounds(width, height, K4, dist.data(), (int)dist.size(), b));
  return ImageBounds{b[0], b[1], b[2], b[3], b[4]};
}
// mvKeyLines and mLineDescriptors are compacted in place to the lines that stay inside the bounds, as the reference's loop does
inline void UndistortKeyLines(std::vector<KeyLine>& mvKeyLines, std::vector<uint8_t>& mLineDescriptors, const float* K4,
                              const std::vector<float>& dist, const ImageBounds& bounds, std::vector<KeyLine>& mvKeyLinesUn) {   // :1555-1700
  const int n = (int)mvKeyLines.size();
  const float b4[4] = {bounds.mnMinX, bounds.mnMaxX, bounds.mnMinY, bounds.mnMaxY};
  std::vector<int32_t> kept((size_t)n);
  mvKeyLinesUn.resize((size_t)n);
  int m = 0;
  check(plvs_hip_frame_undistort_keylines(mvKeyLines.data(), n, K4, dist.data(), (int)dist.size(), b4, mvKeyLinesUn.data(), kept.data(), &m));
  for (int j = 0; j < m; ++j) {
    mvKeyLines[(size_t)j] = mvKeyLines[(size_t)kept[(size_t)j]];
    std::memmove(mLineDescriptors.data() + 32 * (size_t)j, mLineDescriptors.data() + 32 * (size_t)kept[(size_t)j], 32);
  }
  mvKeyLines.resize((size_t)m);
  mvKeyLinesUn.resize((size_t)m);
  mLineDescriptors.resize(32 * (size_t)m);
}
// mGrid as a CSR: cell = column * 48 + row, cellStart[3073], members in key-point order
inline void AssignFeaturesToGrid(const std::vector<KeyPoint>& mvKeysUn, float mnMinX, float mnMinY, float mfGridElementWidthInv,
                                 float mfGridElementHeightInv, std::vector<int32_t>& cellStart, std::vector<int32_t>& cellItems) {   // :716-746
  cellStart.assign(64 * 48 + 1, 0);
  cellItems.resize(mvKeysUn.size());
  int n = 0;
  check(plvs_hip_frame_assign_features_to_grid(mvKeysUn.data(), (int)mvKeysUn.size(), mnMinX, mnMinY, mfGridElementWidthInv,
                                               mfGridElementHeightInv, cellStart.data(), cellItems.data(), &n));
  cellItems.resize((size_t)n);
}

// ---- RGB-D (src/Frame.cc:549, :572): imDepth is a host image here — these two upload it on every call; a caller that keeps
// the depth in device memory (the buffer of the TSDF depth entries) calls plvs_hip_frame_stereo_from_rgbd_dev or rgbd_frame.
inline void ComputeStereoFromRGBD(const std::vector<KeyPoint>& mvKeys, const std::vector<KeyPoint>& mvKeysUn, const Image32F& imDepth,
                                  float mbf, std::vector<float>& mvuRight, std::vector<float>& mvDepth) {   // :2251-2279
  if (mvKeys.size() != mvKeysUn.size()) throw std::invalid_argument("ComputeStereoFromRGBD: mvKeys / mvKeysUn sizes differ");
  mvuRight.assign(mvKeys.size(), -1.0f);
  mvDepth.assign(mvKeys.size(), -1.0f);
  check(plvs_hip_frame_compute_stereo_from_rgbd(mvKeys.data(), mvKeysUn.data(), (int)mvKeys.size(), imDepth.data, imDepth.cols,
                                                imDepth.rows, (int)(imDepth.step / sizeof(float)), mbf, mvuRight.data(), mvDepth.data()));
}
inline void ComputeStereoLinesFromRGBD(const std::vector<KeyLine>& mvKeyLines, const std::vector<KeyLine>& mvKeyLinesUn,
                                       const Image32F& imDepth, const float* K4, float mbf, std::vector<float>& mvuRightLineStart,
                                       std::vector<float>& mvDepthLineStart, std::vector<float>& mvuRightLineEnd,
                                       std::vector<float>& mvDepthLineEnd, float skMinLineLength3D = 0.01f) {   // :2434-2674
  if (mvKeyLines.size() != mvKeyLinesUn.size()) throw std::invalid_argument("ComputeStereoLinesFromRGBD: mvKeyLines / mvKeyLinesUn sizes differ");
  const size_t n = mvKeyLines.size();
  mvuRightLineStart.assign(n, -1.0f);
  mvDepthLineStart.assign(n, -1.0f);
  mvuRightLineEnd.assign(n, -1.0f);
  mvDepthLineEnd.assign(n, -1.0f);
  check(plvs_hip_frame_compute_stereo_lines_from_rgbd(mvKeyLines.data(), mvKeyLinesUn.data(), (int)n, imDepth.data, imDepth.cols,
                                                      imDepth.rows, (int)(imDepth.step / sizeof(float)), K4, mbf, skMinLineLength3D,
                                                      mvuRightLineStart.data(), mvDepthLineStart.data(), mvuRightLineEnd.data(),
                                                      mvDepthLineEnd.data()));
}
inline float ComputeSceneMedianDepth(const std::vector<float>& mvDepth, float skFovCenterDistance = 1.5f) {   // :2730-2751
  float m = skFovCenterDistance;
  check(plvs_hip_frame_scene_median_depth(mvDepth.data(), (int)mvDepth.size(), skFovCenterDistance, &m));
  return m;
}

// The RGB-D constructor (src/Frame.cc:401-600) in one call.  d_image (8-bit grey, `step` bytes a row) and d_depth (float,
// depthPitch floats a row) are DEVICE pointers (plvs_hip_malloc / plvs_hip_memcpy_h2d, or the caller's own HIP buffers);
// lines may be nullptr.  The members are what a Frame holds after the constructor.
struct RgbdFrame {
  int monoLeft = -1;
  std::vector<KeyPoint> mvKeys, mvKeysUn;
  std::vector<uint8_t> mDescriptors;
  std::vector<float> mvuRight, mvDepth;
  float mMedianDepth = 1.5f;
  std::vector<KeyLine> mvKeyLines, mvKeyLinesUn;
  std::vector<uint8_t> mLineDescriptors;
  std::vector<float> mvuRightLineStart, mvDepthLineStart, mvuRightLineEnd, mvDepthLineEnd;
  std::vector<int32_t> cellStart, cellItems;   // mGrid as a CSR (AssignFeaturesToGrid above)
};
inline void rgbd_frame(ORBextractor& orb, LineExtractor* lines, const uint8_t* d_image, int width, int height, int step,
                       const float* d_depth, int depthPitch, const plvs_rgbd_calib& calib, RgbdFrame& F, int kpCapacity = 8192,
                       int lineCapacity = 4096, void* stream = nullptr) {
  const size_t nc = (size_t)kpCapacity, lc = lines ? (size_t)lineCapacity : 0;
  F.mvKeys.resize(nc); F.mvKeysUn.resize(nc); F.mDescriptors.resize(32 * nc); F.mvuRight.resize(nc); F.mvDepth.resize(nc);
  F.cellStart.assign(64 * 48 + 1, 0); F.cellItems.resize(nc);
  F.mvKeyLines.resize(lc); F.mvKeyLinesUn.resize(lc); F.mLineDescriptors.resize(32 * lc);
  F.mvuRightLineStart.resize(lc); F.mvDepthLineStart.resize(lc); F.mvuRightLineEnd.resize(lc); F.mvDepthLineEnd.resize(lc);
  plvs_rgbd_frame f;
  std::memset(&f, 0, sizeof f);
  f.kp_cap = kpCapacity; f.line_cap = (int)lc;
  f.kps = F.mvKeys.data(); f.kps_un = F.mvKeysUn.data(); f.desc = F.mDescriptors.data(); f.u_right = F.mvuRight.data();
  f.depth = F.mvDepth.data(); f.cell_start = F.cellStart.data(); f.cell_items = F.cellItems.data();
  if (lines) {
    f.keylines = F.mvKeyLines.data(); f.keylines_un = F.mvKeyLinesUn.data(); f.line_desc = F.mLineDescriptors.data();
    f.u_right_start = F.mvuRightLineStart.data(); f.depth_start = F.mvDepthLineStart.data();
    f.u_right_end = F.mvuRightLineEnd.data(); f.depth_end = F.mvDepthLineEnd.data();
  }
  check(plvs_hip_frame_rgbd_dev(orb.handle(), lines ? lines->handle() : nullptr, d_image, width, height, step, d_depth, depthPitch,
                                &calib, &f, stream));
  const size_t n = (size_t)f.n_kp, nl = (size_t)f.n_lines;
  F.monoLeft = f.mono_index;
  F.mMedianDepth = f.median_depth;
  F.mvKeys.resize(n); F.mvKeysUn.resize(n); F.mDescriptors.resize(32 * n); F.mvuRight.resize(n); F.mvDepth.resize(n);
  F.cellItems.resize((size_t)f.n_items);
  F.mvKeyLines.resize(nl); F.mvKeyLinesUn.resize(nl); F.mLineDescriptors.resize(32 * nl);
  F.mvuRightLineStart.resize(nl); F.mvDepthLineStart.resize(nl); F.mvuRightLineEnd.resize(nl); F.mvDepthLineEnd.resize(nl);
}

// ---- stereo (src/Frame.cc:374): Frame::ComputeStereoLineMatches with LineMatcher::SearchStereoMatchesByKnn inside it, one
// launch.  The pair is rectified: mvKeyLinesUn == mvKeyLines on both sides.  The matcher's arguments default to the
// LineMatcher(0.7) the reference builds and LineMatcher::TH_LOW_STEREO.  Returns the lines left with both depths.
inline int ComputeStereoLineMatches(const std::vector<KeyLine>& mvKeyLinesUn, const std::vector<uint8_t>& mLineDescriptors,
                                    const std::vector<KeyLine>& mvKeyLinesRightUn, const std::vector<uint8_t>& mLineDescriptorsRight,
                                    const std::vector<float>& mvLineLevelSigma2, const float* K4, float mbf,
                                    std::vector<float>& mvuRightLineStart, std::vector<float>& mvDepthLineStart,
                                    std::vector<float>& mvuRightLineEnd, std::vector<float>& mvDepthLineEnd,
                                    float skLineStereoMaxDist = 20.0f, float skMinLineLength3D = 0.01f, float nnRatio = 0.7f,
                                    bool checkOrientation = true, int thDescriptorDist = 50, void* stream = nullptr) {   // :2008-2248
  const size_t n = mvKeyLinesUn.size(), nr = mvKeyLinesRightUn.size();
  if (mLineDescriptors.size() != 32 * n || mLineDescriptorsRight.size() != 32 * nr)
    throw std::invalid_argument("ComputeStereoLineMatches: 32 descriptor bytes per line");
  mvuRightLineStart.assign(n, -1.0f);
  mvDepthLineStart.assign(n, -1.0f);
  mvuRightLineEnd.assign(n, -1.0f);
  mvDepthLineEnd.assign(n, -1.0f);
  int stereo = 0;
  check(plvs_hip_frame_compute_stereo_line_matches(mvKeyLinesUn.data(), mLineDescriptors.data(), (int)n, mvKeyLinesRightUn.data(),
                                                   mLineDescriptorsRight.data(), (int)nr, mvLineLevelSigma2.data(),
                                                   (int)mvLineLevelSigma2.size(), K4, mbf, skLineStereoMaxDist, skMinLineLength3D, nnRatio,
                                                   checkOrientation ? 1 : 0, thDescriptorDist, mvuRightLineStart.data(),
                                                   mvDepthLineStart.data(), mvuRightLineEnd.data(), mvDepthLineEnd.data(), &stereo, stream));
  return stereo;
}

// The stereo constructor (src/Frame.cc:214-398) in one call on a RECTIFIED pair.  d_left / d_right (8-bit grey, `step` bytes a
// row, one size) are DEVICE pointers; the line extractors are both given or both nullptr; `stereo` comes from
// plvs_hip_stereo_create(left.handle(), right.handle(), ...) and is kept between frames.  calib.line_level_sigma2 points at the
// caller's mvLineLevelSigma2.  No bounds filter and no compaction of the lines (mvKeyLinesUn = mvKeyLines).  The members are
// what a Frame holds after the constructor.
struct StereoFrameMembers {
  int monoLeft = -1, monoRight = -1;
  std::vector<KeyPoint> mvKeys, mvKeysUn, mvKeysRight;
  std::vector<uint8_t> mDescriptors, mDescriptorsRight;
  std::vector<float> mvuRight, mvDepth;
  std::vector<KeyLine> mvKeyLines, mvKeyLinesUn, mvKeyLinesRight, mvKeyLinesRightUn;
  std::vector<uint8_t> mLineDescriptors, mLineDescriptorsRight;
  std::vector<float> mvuRightLineStart, mvDepthLineStart, mvuRightLineEnd, mvDepthLineEnd;
  std::vector<int32_t> cellStart, cellItems;   // mGrid as a CSR (AssignFeaturesToGrid above)
  int stereoPoints = 0, stereoLines = 0;       // key points / lines with depth
};
inline void StereoFrame(ORBextractor& left, ORBextractor& right, LineExtractor* linesLeft, LineExtractor* linesRight, plvs_stereo* stereo,
                        const uint8_t* d_left, const uint8_t* d_right, int width, int height, int step, const plvs_stereo_calib& calib,
                        StereoFrameMembers& F, int kpCapacity = 8192, int lineCapacity = 4096, void* stream = nullptr) {
  const bool withLines = linesLeft != nullptr;
  const size_t nc = (size_t)kpCapacity, lc = withLines ? (size_t)lineCapacity : 0;
  F.mvKeys.resize(nc); F.mvKeysUn.resize(nc); F.mDescriptors.resize(32 * nc); F.mvuRight.resize(nc); F.mvDepth.resize(nc);
  F.mvKeysRight.resize(nc); F.mDescriptorsRight.resize(32 * nc);
  F.cellStart.assign(64 * 48 + 1, 0); F.cellItems.resize(nc);
  F.mvKeyLines.resize(lc); F.mvKeyLinesUn.resize(lc); F.mLineDescriptors.resize(32 * lc);
  F.mvKeyLinesRight.resize(lc); F.mvKeyLinesRightUn.resize(lc); F.mLineDescriptorsRight.resize(32 * lc);
  F.mvuRightLineStart.resize(lc); F.mvDepthLineStart.resize(lc); F.mvuRightLineEnd.resize(lc); F.mvDepthLineEnd.resize(lc);
  plvs_stereo_frame f;
  std::memset(&f, 0, sizeof f);
  f.kp_cap = f.kp_right_cap = kpCapacity;
  f.line_cap = f.line_right_cap = (int)lc;
  f.kps = F.mvKeys.data(); f.kps_un = F.mvKeysUn.data(); f.desc = F.mDescriptors.data(); f.u_right = F.mvuRight.data();
  f.depth = F.mvDepth.data(); f.cell_start = F.cellStart.data(); f.cell_items = F.cellItems.data();
  f.kps_right = F.mvKeysRight.data(); f.desc_right = F.mDescriptorsRight.data();
  if (withLines) {
    f.keylines = F.mvKeyLines.data(); f.keylines_un = F.mvKeyLinesUn.data(); f.line_desc = F.mLineDescriptors.data();
    f.keylines_right = F.mvKeyLinesRight.data(); f.keylines_right_un = F.mvKeyLinesRightUn.data();
    f.line_desc_right = F.mLineDescriptorsRight.data();
    f.u_right_start = F.mvuRightLineStart.data(); f.depth_start = F.mvDepthLineStart.data();
    f.u_right_end = F.mvuRightLineEnd.data(); f.depth_end = F.mvDepthLineEnd.data();
  }
  check(plvs_hip_frame_stereo_dev(left.handle(), right.handle(), withLines ? linesLeft->handle() : nullptr,
                                  linesRight ? linesRight->handle() : nullptr, stereo, d_left, d_right, width, height, step, &calib, &f,
                                  stream));
  const size_t n = (size_t)f.n_kp, nr = (size_t)f.n_kp_right, nl = (size_t)f.n_lines, nlr = (size_t)f.n_lines_right;
  F.monoLeft = f.mono_index;
  F.monoRight = f.mono_index_right;
  F.stereoPoints = f.n_stereo_points;
  F.stereoLines = f.n_stereo_lines;
  F.mvKeys.resize(n); F.mvKeysUn.resize(n); F.mDescriptors.resize(32 * n); F.mvuRight.resize(n); F.mvDepth.resize(n);
  F.mvKeysRight.resize(nr); F.mDescriptorsRight.resize(32 * nr);
  F.cellItems.resize((size_t)f.n_items);
  F.mvKeyLines.resize(nl); F.mvKeyLinesUn.resize(nl); F.mLineDescriptors.resize(32 * nl);
  F.mvKeyLinesRight.resize(nlr); F.mvKeyLinesRightUn.resize(nl > 0 ? nlr : 0); F.mLineDescriptorsRight.resize(32 * nlr);
  F.mvuRightLineStart.resize(nl); F.mvDepthLineStart.resize(nl); F.mvuRightLineEnd.resize(nl); F.mvDepthLineEnd.resize(nl);
}

// ---- the local map (src/Tracking.cc:4430-4579): Frame::isInFrustum over the local map points and lines in one launch, and the
// two searches of TrackLocalMap behind it in one call.  The vectors are what the reference leaves on the map elements
// (mbTrackInView, mTrackProj*, mTrackDepth, mnTrackScaleLevel, mTrackViewCos); single-camera pinhole frames only.
struct LocalMapFields {
  std::vector<uint8_t> pointInView, lineInView;
  std::vector<float> trackProjX, trackProjY, trackProjXR, trackDepth, trackViewCos;
  std::vector<int32_t> trackScaleLevel, lineScaleLevel;
  std::vector<float> lineProj, lineProjXR, lineViewCos;   // 6 / 2 / 1 per line
  int nToMatchPoints = 0, nToMatchLines = 0;
  int32_t stats[4] = {0, 0, 0, 0};                         // see plvs_hip_frame_is_in_frustum
  std::vector<int32_t> assignedPoints, assignedLines;      // SearchLocalMap only
  int nMatchesPoints = 0, nMatchesLines = 0;
};
namespace detail {
inline void bind(LocalMapFields& o, plvs_track_points* P, plvs_track_lines* L) {
  if (P) {
    const size_t m = (size_t)P->m;
    o.pointInView.assign(m, 0); o.trackProjX.assign(m, -1.0f); o.trackProjY.assign(m, -1.0f); o.trackProjXR.assign(m, 0.0f);
    o.trackDepth.assign(m, 0.0f); o.trackViewCos.assign(m, 0.0f); o.trackScaleLevel.assign(m, 0);
    P->in_view = o.pointInView.data(); P->proj_x = o.trackProjX.data(); P->proj_y = o.trackProjY.data(); P->proj_xr = o.trackProjXR.data();
    P->track_depth = o.trackDepth.data(); P->level = o.trackScaleLevel.data(); P->view_cos = o.trackViewCos.data();
  }
  if (L) {
    const size_t m = (size_t)L->m;
    o.lineInView.assign(m, 0); o.lineProj.assign(6 * m, 0.0f); o.lineProjXR.assign(2 * m, -1.0f); o.lineViewCos.assign(m, 0.0f);
    o.lineScaleLevel.assign(m, 0);
    L->in_view = o.lineInView.data(); L->proj = o.lineProj.data(); L->proj_xr = o.lineProjXR.data(); L->level = o.lineScaleLevel.data();
    L->view_cos = o.lineViewCos.data();
  }
}
}  // namespace detail
// points / lines: the input members filled by the caller (m, skip, pos / start / end, normal, the distances, desc, has_obs);
// the output members are pointed at `out`.  Either may be nullptr.
inline void IsInFrustum(const plvs_track_camera& cam, plvs_track_points* points, plvs_track_lines* lines, LocalMapFields& out,
                        void* stream = nullptr) {
  detail::bind(out, points, lines);
  check(plvs_hip_frame_is_in_frustum(&cam, points, lines, &out.nToMatchPoints, &out.nToMatchLines, out.stats, stream));
}
// Tracking::SearchLocalPoints + SearchLocalLines: LF / lines nullptr without the line tracker.
inline void SearchLocalMap(const plvs_track_camera& cam, const plvs_frame_view& F, const plvs_line_frame_view* LF, plvs_track_points& points,
                           plvs_track_lines* lines, float th, bool bFarPoints, float thFarPoints, float nnRatio, bool bLargerSearch,
                           const uint8_t* occupiedPoints, const uint8_t* occupiedLines, LocalMapFields& out, void* stream = nullptr) {
  detail::bind(out, &points, lines);
  out.assignedPoints.assign((size_t)(F.n > 0 ? F.n : 0), -1);
  out.assignedLines.assign((size_t)(LF && LF->n > 0 ? LF->n : 0), -1);
  check(plvs_hip_frame_search_local_map(&cam, &F, LF, &points, lines, th, bFarPoints ? 1 : 0, thFarPoints, nnRatio, bLargerSearch ? 1 : 0,
                                        occupiedPoints, occupiedLines, out.assignedPoints.data(), &out.nMatchesPoints, out.assignedLines.data(),
                                        &out.nMatchesLines, &out.nToMatchPoints, &out.nToMatchLines, out.stats, stream));
}

// ---- the last frame (src/Tracking.cc:3615-3664): the search of TrackWithMotionModel in one call — the projection of the last
// frame's map points and lines on the device (Tcw * x3Dw as Sophus' quaternion action, Pinhole::project,
// LineProjection::ProjectLineWithCheck), ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) and
// LineMatcher::SearchByProjection(CurrentFrame, LastFrame, bLargerSearch, bMono) behind it, and the retry rules.  Single-camera
// pinhole frames only.
struct MotionModelMatches {
  std::vector<int32_t> assignedPoints, assignedLines;   // per current key point / key line: the last-frame index, or -1
  int nPointMatches = 0, nLineMatches = 0;
  bool bForward = false, bBackward = false, bLargerLineSearch = false;
  float thUsed = 0.0f;
  std::vector<uint8_t> projValidPoints, projValidLines;  // what the two separate entries expect from their caller
  std::vector<float> u, v, invz, lineProj;               // lineProj: uS, vS, uE, vE, invSz, invEz per line
  int32_t stats[4] = {0, 0, 0, 0};                       // see plvs_hip_frame_search_last_frame
};
// points / lines: the input members filled by the caller; their optional output members are ignored — the call works on copies
// whose output members point into `out`, and the caller's structures are left as they are.  LF / lines nullptr without the line
// tracker.  minPointMatches = 20, minLineMatches = 10 are Tracking's; 0, 0 make it one search of each kind.
inline void TrackWithMotionModelSearch(const plvs_motion_poses& poses, const plvs_frame_view& F, const float* curAngles,
                                       const plvs_line_frame_view* LF, const plvs_motion_points& pointsIn, const plvs_motion_lines* linesIn,
                                       float th, bool checkOrientation, MotionModelMatches& out, const uint8_t* occupiedPoints = nullptr,
                                       const uint8_t* occupiedLines = nullptr, int minPointMatches = 20, int minLineMatches = 10,
                                       float nnRatioPoints = 0.9f, float nnRatioLines = 0.9f, void* stream = nullptr) {
  plvs_motion_points points = pointsIn;
  plvs_motion_lines linesCopy;
  plvs_motion_lines* lines = nullptr;
  if (linesIn) { linesCopy = *linesIn; lines = &linesCopy; }
  const size_t n = (size_t)(points.n > 0 ? points.n : 0), nl = (size_t)(lines && lines->n > 0 ? lines->n : 0);
  out.projValidPoints.assign(n, 0); out.u.assign(n, -1.0f); out.v.assign(n, -1.0f); out.invz.assign(n, 0.0f);
  points.proj_valid = out.projValidPoints.data(); points.u = out.u.data(); points.v = out.v.data(); points.invz = out.invz.data();
  out.projValidLines.assign(nl, 0); out.lineProj.assign(6 * nl, 0.0f);
  if (lines) { lines->proj_valid = out.projValidLines.data(); lines->proj6 = out.lineProj.data(); }
  out.assignedPoints.assign((size_t)(F.n > 0 ? F.n : 0), -1);
  out.assignedLines.assign((size_t)(LF && LF->n > 0 ? LF->n : 0), -1);
  plvs_motion_policy policy;
  policy.th = th; policy.nn_ratio_points = nnRatioPoints; policy.nn_ratio_lines = nnRatioLines;
  policy.check_orientation = checkOrientation ? 1 : 0; policy.min_point_matches = minPointMatches; policy.min_line_matches = minLineMatches;
  plvs_motion_result res;
  check(plvs_hip_frame_search_last_frame(&poses, &F, curAngles, LF, &points, lines, &policy, occupiedPoints, occupiedLines,
                                         out.assignedPoints.data(), out.assignedLines.data(), &res, out.stats, stream));
  out.nPointMatches = res.nmatches_points; out.nLineMatches = res.nmatches_lines;
  out.bForward = res.forward != 0; out.bBackward = res.backward != 0; out.bLargerLineSearch = res.larger_line_search_used != 0;
  out.thUsed = res.th_used;
}

// ------------------------------------------------------------------------------------ dense stereo
// sgm::StereoSGM (Thirdparty/libsgm/include/libsgm.h:57-110) for 8-bit images and an 8-bit disparity, the way
// PointCloudKeyFrame::ProcessStereoLibsgm constructs it; execute() is EXECUTE_INOUT_HOST2HOST.
class StereoSGM {
 public:
  struct Parameters {
    int P1, P2;
    float uniqueness;
    Parameters(int P1 = 10, int P2 = 120, float uniqueness = 0.95f) : P1(P1), P2(P2), uniqueness(uniqueness) {}
  };
  StereoSGM(int width, int height, int disparity_size, int input_depth_bits = 8, int output_depth_bits = 8,
            const Parameters& param = Parameters()) {
    if (input_depth_bits != 8 || output_depth_bits != 8) throw std::logic_error("depth bits must be 8 on the accelerated path");
    if (disparity_size != 64 && disparity_size != 128) throw std::logic_error("disparity size must be 64 or 128");
    check(plvs_hip_sgm_create(width, height, disparity_size, param.P1, param.P2, param.uniqueness, &h_));
  }
  ~StereoSGM() { plvs_hip_sgm_destroy(h_); }
  StereoSGM(const StereoSGM&) = delete;
  StereoSGM& operator=(const StereoSGM&) = delete;
  void execute(const void* left_pixels, const void* right_pixels, void* dst) {
    check(plvs_hip_sgm_execute(h_, static_cast<const uint8_t*>(left_pixels), static_cast<const uint8_t*>(right_pixels),
                               static_cast<uint8_t*>(dst)));
  }

 private:
  plvs_sgm* h_ = nullptr;
};

// libelas::ElasGPU (Thirdparty/libelas-gpu/GPU/elas_gpu.h:29-47) without the inheritance: the two methods of
// libelas::Elas it overrides.  In a PLVS tree the class is the reference's own —
//     class ElasGPU : public Elas { ... computeDisparity(...) override; adaptiveMean(float* D) override; };
// — with these two bodies (INTEGRATION.md shows it); here the reference's types are spelled out so that the header
// stands alone.  support_pt / triangle have the layout of Elas::support_pt / Elas::triangle (elas.h:178-190).
class ElasGPU {
 public:
  struct support_pt { int32_t u, v, d; };
  struct triangle { int32_t c1, c2, c3; float t1a, t1b, t1c, t2a, t2b, t2c; };
  struct Parameters {   // the fields of Elas::Parameters the two methods read; defaults: ROBOTICS (elas.h:97-121)
    bool subsampling;
    int32_t grid_size, match_texture;
    float beta, gamma, sigma, sradius;
    int32_t disp_min, disp_max, candidate_stepsize, support_texture, lr_threshold;   // supportCandidates (lr_threshold: the check too)
    float support_threshold;
    float speckle_sim_threshold;                                                      // the post-processing methods
    int32_t speckle_size, ipol_gap_width;
    bool add_corners;
    Parameters()
        : subsampling(false), grid_size(20), match_texture(1), beta(0.02f), gamma(3), sigma(1), sradius(2), disp_min(0),
          disp_max(255), candidate_stepsize(5), support_texture(10), lr_threshold(2), support_threshold(0.85f),
          speckle_sim_threshold(1), speckle_size(200), ipol_gap_width(3), add_corners(false) {}
  };
  explicit ElasGPU(const Parameters& param = Parameters()) : param(param) {
    plvs_elas_params p{param.subsampling ? 1 : 0, param.grid_size, param.match_texture, param.beta, param.gamma, param.sigma,
                       param.sradius, param.disp_min, param.disp_max, param.candidate_stepsize, param.support_texture,
                       param.lr_threshold, param.support_threshold, param.speckle_sim_threshold, param.speckle_size,
                       param.ipol_gap_width, param.add_corners ? 1 : 0};
    check(plvs_hip_elas_create(&p, &h_));
  }
  ~ElasGPU() { plvs_hip_elas_destroy(h_); }
  ElasGPU(const ElasGPU&) = delete;
  ElasGPU& operator=(const ElasGPU&) = delete;
  // Elas::process sets width / height before it calls the two methods (elas.cpp:39-40); here the caller does.
  int32_t width = 0, height = 0;
  Parameters param;

  // Elas::computeDisparity's arguments.  The descriptor images are uploaded with the left image's call and reused by
  // the right image's (Elas::process calls the two back to back on the same pair, elas.cpp:113-114).
  void computeDisparity(const std::vector<support_pt>& p_support, const std::vector<triangle>& tri, const int32_t* disparity_grid,
                        const int32_t* grid_dims, const uint8_t* I1_desc, const uint8_t* I2_desc, bool right_image, float* D) {
    static_assert(sizeof(support_pt) == 12 && sizeof(triangle) == 36, "record layouts of the C ABI");
    const bool staged = (right_image || staged_by_support_) && I1_desc == staged_1_ && I2_desc == staged_2_ && staged_w_ == width &&
                        staged_h_ == height;
    check(plvs_hip_elas_compute_disparity(h_, reinterpret_cast<const int32_t*>(p_support.data()), (int)p_support.size(), tri.data(),
                                          (int)tri.size(), disparity_grid, grid_dims, staged ? nullptr : I1_desc,
                                          staged ? nullptr : I2_desc, width, height, right_image ? 1 : 0, D));
    staged_by_support_ = staged_by_support_ && !right_image;   // (the pair supportCandidates staged serves its two calls)
    staged_1_ = right_image ? nullptr : I1_desc;       // (only a left-image call vouches for the staged pair)
    staged_2_ = right_image ? nullptr : I2_desc;
    staged_w_ = width;
    staged_h_ = height;
  }
  void adaptiveMean(float* D) { check(plvs_hip_elas_adaptive_mean(h_, D, width, height)); }
  // the other virtual post-processing methods of Elas (elas.cpp:971-1347), in place
  void leftRightConsistencyCheck(float* D1, float* D2) { check(plvs_hip_elas_left_right_check(h_, D1, D2, width, height)); }
  void removeSmallSegments(float* D) { check(plvs_hip_elas_remove_small_segments(h_, D, width, height)); }
  void gapInterpolation(float* D) { check(plvs_hip_elas_gap_interpolation(h_, D, width, height)); }
  // Elas::computeDelaunayTriangulation (elas.cpp:492-556): the reference's triangles in its order, planes 0.  Host code.
  static std::vector<triangle> computeDelaunayTriangulation(const std::vector<support_pt>& p_support, int32_t right_image) {
    std::vector<triangle> tri(2 * p_support.size() + 2);
    int n = 0;
    check(plvs_hip_elas_triangulate(reinterpret_cast<const int32_t*>(p_support.data()), (int)p_support.size(), right_image,
                                    tri.data(), (int)tri.size(), &n));
    tri.resize(n);
    return tri;
  }
  // Elas::process (elas.cpp:36-157) with its signature, in one call: a replacement of ElasInterface::process is one line.
  // postprocess_only_left / filter_adaptive_mean as Elas::Parameters holds them (PLVS: both true).
  bool postprocess_only_left = true, filter_adaptive_mean = true;
  void process(uint8_t* I1, uint8_t* I2, float* D1, float* D2, const int32_t* dims) {
    width = dims[0];
    height = dims[1];
    check(plvs_hip_elas_process(h_, I1, I2, dims, postprocess_only_left ? 1 : 0, filter_adaptive_mean ? 1 : 0, D1, D2));
    staged_1_ = staged_2_ = nullptr;
    staged_w_ = width;
    staged_h_ = height;
    staged_by_support_ = false;
  }
  // libelas::Descriptor of both images on the device; supportCandidates / computeDisparity then take nullptr descriptors
  void setImages(const uint8_t* I1, const uint8_t* I2, int32_t stride) {
    check(plvs_hip_elas_set_images(h_, I1, I2, width, height, stride));
    staged_1_ = staged_2_ = nullptr;
    staged_w_ = width;
    staged_h_ = height;
    staged_by_support_ = true;
  }
  // The candidate loop of Elas::computeSupportMatches (elas.cpp:434-456): D_can as that function allocates it
  // (D_can_width x D_can_height int16); the reference's filters follow on the host.  Stages the descriptor pair.
  void supportCandidates(const uint8_t* I1_desc, const uint8_t* I2_desc, int16_t* D_can) {
    check(plvs_hip_elas_support_candidates(h_, I1_desc, I2_desc, width, height, D_can));
    staged_1_ = I1_desc;
    staged_2_ = I2_desc;
    staged_w_ = width;
    staged_h_ = height;
    staged_by_support_ = true;
  }

 private:
  plvs_elas* h_ = nullptr;
  const uint8_t *staged_1_ = nullptr, *staged_2_ = nullptr;
  int32_t staged_w_ = 0, staged_h_ = 0;
  bool staged_by_support_ = false;
};

// ------------------------------------------------------------------------------------ depth -> cloud
class PointCloudGenerator {   // PointCloudMapping::InitCamGridPoints + GeneratePointCloudInCameraFrameBGRA
 public:
  // matCamGridPoints: N x 2 floats after InitCamGridPoints, or empty for an undistorted camera (computed here)
  PointCloudGenerator(int width, int height, int downsampleStep, double fx, double fy, double cx, double cy,
                      double minDepth, double maxDepth, std::vector<float> matCamGridPoints = {})
      : w_(width), h_img_(height), min_(minDepth), max_(maxDepth) {
    ngrid_ = plvs_hip_cloudgen_num_grid_points(width, height, downsampleStep);
    if (matCamGridPoints.empty()) {
      matCamGridPoints.resize((size_t)2 * ngrid_);
      check(plvs_hip_cloudgen_grid_points(width, height, downsampleStep, fx, fy, cx, cy, matCamGridPoints.data()));
    }
    check(plvs_hip_cloudgen_create(width, height, downsampleStep, matCamGridPoints.data(), &h_));
  }
  ~PointCloudGenerator() { plvs_hip_cloudgen_destroy(h_); }
  PointCloudGenerator(const PointCloudGenerator&) = delete;
  PointCloudGenerator& operator=(const PointCloudGenerator&) = delete;

  std::vector<PointSurfelSegment> GeneratePointCloudInCameraFrameBGRA(uint32_t kfid, const Image8U& color,
                                                                      const Image32F& depth,
                                                                      std::vector<int32_t>* pixelToPointIndex = nullptr) {
    std::vector<PointSurfelSegment> cloud((size_t)ngrid_);
    if (pixelToPointIndex) pixelToPointIndex->resize((size_t)w_ * h_img_);
    int n = 0;
    check(plvs_hip_cloudgen_generate(h_, depth.data, (int)(depth.step / sizeof(float)), color.data, (int)color.step, min_,
                                     max_, kfid, cloud.data(), ngrid_, pixelToPointIndex ? pixelToPointIndex->data() : nullptr,
                                     &n));
    cloud.resize((size_t)n);
    return cloud;
  }

 private:
  plvs_cloudgen* h_ = nullptr;
  int w_, h_img_, ngrid_ = 0;
  double min_, max_;
};

// ------------------------------------------------------------------------------------ chisel map
struct Mesh {   // chisel::Mesh after RecomputeMesh
  std::vector<float> vertices, normals, colors;   // n x 3
  std::vector<uint32_t> kfids;
};

class PointCloudMapChisel {
 public:
  using ChunkID = std::tuple<int, int, int>;
  // bCloudDeformationOnSparseMapChange: the map keeps the reference's chunk order from its first cloud on, so that
  // OnMapChange can deform it as Chisel::Deform does (plvs_hip_tsdf_chisel_enable_deform)
  explicit PointCloudMapChisel(float resolution, bool useCarving = false, float carvingDist = 0.05f,
                               float nearPlaneDist = 0.05f, float farPlaneDist = 5.0f, bool bResetOnSparseMapChange = true,
                               bool bCloudDeformationOnSparseMapChange = false, bool queueInsertions = true)
      : useCarving_(useCarving), carvingDist_(carvingDist), near_(nearPlaneDist), far_(farPlaneDist),
        resetOnChange_(bResetOnSparseMapChange), deformOnChange_(bCloudDeformationOnSparseMapChange),
        // queueInsertions: InsertCloud uploads the key frame's cloud, UpdateMap (or whatever reads or changes the map
        // first) integrates the ones waiting — at most five between two UpdateMap calls of PointCloudMapping
        // (src/PointCloudMapping.cc:540-552) — in one batch: the reference only reads the map in UpdateMap, and the batch
        // gives the same map bit for bit in the (default) ordered mode (plvs_hip_tsdf_chisel_queue).  Off with the
        // deformation bookkeeping, which follows the map call by call.
        queue_(queueInsertions && !bCloudDeformationOnSparseMapChange) {
    plvs_tsdf_chisel_params p;
    check(plvs_hip_tsdf_chisel_default_params(resolution, &p));
    check(plvs_hip_tsdf_chisel_create(&p, &h_));
    if (deformOnChange_) check(plvs_hip_tsdf_chisel_enable_deform(h_));
  }
  ~PointCloudMapChisel() { plvs_hip_tsdf_chisel_destroy(h_); }
  PointCloudMapChisel(const PointCloudMapChisel&) = delete;
  PointCloudMapChisel& operator=(const PointCloudMapChisel&) = delete;

  // InsertCloud(cloud_camera, Twc, max_range): SetPointCloud + IntegrateLastPointCloud (PointCloudMapChisel.cc:76-98)
  void InsertCloud(const std::vector<PointSurfelSegment>& cloud_camera, const SE3f& Twc, double /*max_range*/ = 0) {
    const size_t n = cloud_camera.size();
    xyz_.resize(3 * n);
    rgb_.resize(3 * n);
    kfid_.resize(n);
    for (size_t i = 0; i < n; ++i) {   // PclPointCloudToChisel: position, the r, g, b members, kfid
      const PointSurfelSegment& p = cloud_camera[i];
      xyz_[3 * i] = p.x; xyz_[3 * i + 1] = p.y; xyz_[3 * i + 2] = p.z;
      rgb_[3 * i] = p.r; rgb_[3 * i + 1] = p.g; rgb_[3 * i + 2] = p.b;
      kfid_[i] = p.kfid;
    }
    if (queue_) {
      check(plvs_hip_tsdf_chisel_queue(h_, xyz_.data(), rgb_.data(), kfid_.data(), (int)n, Twc.m));
      return;
    }
    check(plvs_hip_tsdf_chisel_integrate(h_, xyz_.data(), rgb_.data(), kfid_.data(), (int)n, Twc.m));
    MarkUpdated();
  }
  // Integrates the queued key frames (one batch) and notes the meshes they invalidate.
  void Flush() {
    int waiting = 0;
    check(plvs_hip_tsdf_chisel_queued(h_, &waiting));
    if (waiting > 0) {
      check(plvs_hip_tsdf_chisel_flush(h_));
      MarkUpdated();
    }
  }
  // InsertCloudWithDepth: carving of the depth image's frustum first when useCarving (Chisel.cpp:394-438)
  void InsertCloudWithDepth(const std::vector<PointSurfelSegment>& cloud_camera, const SE3f& Twc, const Image32F& depthImage,
                            float fx, float fy, float cx, float cy, double max_range = 0) {
    if (useCarving_) {
      Flush();   // (carving reads and changes the map: what is waiting goes in first)
      if (depthImage.step != (size_t)depthImage.cols * sizeof(float))
        throw std::invalid_argument("InsertCloudWithDepth: the depth image must be continuous");
      int carved = 0;
      check(plvs_hip_tsdf_chisel_carve(h_, depthImage.data, depthImage.cols, depthImage.rows, fx, fy, cx, cy, near_, far_,
                                       Twc.m, carvingDist_, &carved));
      if (carved > 0) {   // meshesToUpdate[chunkID] = true for every carved chunk, the chunk alone (Chisel.cpp:432)
        std::vector<int32_t> ids((size_t)3 * carved);
        int n = 0;
        check(plvs_hip_tsdf_chisel_updated_chunk_ids(h_, ids.data(), carved, &n));
        for (int i = 0; i < n && i < carved; ++i) meshesToUpdate_.insert(ChunkID(ids[3 * i], ids[3 * i + 1], ids[3 * i + 2]));
      }
    }
    InsertCloud(cloud_camera, Twc, max_range);
  }
  // SetDepthCameraModel (src/PointCloudMapChisel.cc:63-67): the camera InsertDepthScanColor projects through
  void SetDepthCameraModel(float fx, float fy, float cx, float cy, int width, int height) {
    depthCam_.fx = fx; depthCam_.fy = fy; depthCam_.cx = cx; depthCam_.cy = cy;
    depthCam_.width = width; depthCam_.height = height;
    depthCam_.near_plane = near_; depthCam_.far_plane = far_;
  }
  // InsertDepthScanColor (src/PointCloudMapChisel.cc:134-189): the depth image and the BGR / BGRA image registered to
  // it through the projective integrator (Chisel::IntegrateDepthScanColorWithOneCameraModelBGR, Chisel.h:198-258);
  // carving follows useCarving.  colorChannels: cv::Mat::channels() of the colour image (3 or 4).
  void InsertDepthScanColor(const Image32F& depthImage, const Image8U& colorImage, const SE3f& Twc, uint64_t /*timestamp*/ = 0,
                            int colorChannels = 3) {
    if (depthImage.data != nullptr && depthImage.rows > 0 && depthImage.cols > 0 && !colorImage.empty()) {
      if (depthCam_.width != depthImage.cols || depthCam_.height != depthImage.rows || colorImage.cols != depthImage.cols ||
          colorImage.rows != depthImage.rows)
        throw std::invalid_argument("InsertDepthScanColor: SetDepthCameraModel first, with the size of the (registered) images");
      Flush();   // (the scan reads and changes the map: what is waiting goes in first)
      check(plvs_hip_tsdf_chisel_integrate_scan(h_, depthImage.data, (int)depthImage.step, colorImage.data, (int)colorImage.step,
                                                colorChannels, &depthCam_, Twc.m, useCarving_ ? 1 : 0, carvingDist_));
      MarkUpdated();   // the 27 neighbours of every updated chunk (Chisel.h:233-245)
    } else {
      std::fprintf(stderr, "PointCloudMapChisel::InsertDepthScanColor() - ERROR: depth and/or color images are emtpy \n");
    }
  }
  // InsertData (src/PointCloudMapChisel.cc:192-225): the dispatch on the input kind; an unknown kind ends the process
  // there (quick_exit), and here.
  struct Input {
    enum Type { kPointCloud, kColorAndDepthImages, kPointCloudAndDepthImage } type = kPointCloud;
    const std::vector<PointSurfelSegment>* pCloudCamera = nullptr;
    Image32F imgDepth;
    Image8U imgColor;
    int colorChannels = 3;
    SE3f Twc{};
    uint64_t timestamp = 0;
    double maxRange = 0;
  };
  void InsertData(const Input& d) {
    static const std::vector<PointSurfelSegment> none;
    switch (d.type) {
      case Input::kPointCloud:
        InsertCloud(d.pCloudCamera ? *d.pCloudCamera : none, d.Twc, d.maxRange);
        break;
      case Input::kColorAndDepthImages:
        InsertDepthScanColor(d.imgDepth, d.imgColor, d.Twc, d.timestamp, d.colorChannels);
        break;
      case Input::kPointCloudAndDepthImage:
        InsertCloudWithDepth(d.pCloudCamera ? *d.pCloudCamera : none, d.Twc, d.imgDepth, depthCam_.fx, depthCam_.fy, depthCam_.cx,
                             depthCam_.cy, d.maxRange);
        break;
      default:
        std::fprintf(stderr, "PointCloudMapChisel<PointT>::InsertData() - ERROR - unknown data mode\n");
        std::quick_exit(-1);
    }
  }
  // UpdateMap: UpdateMesh (meshes of the 27-neighbourhood of every chunk updated since the last call,
  // Chisel.cpp:553-568) + GetPointCloud (ChiselServer.cpp:971-1068).  Returns the cloud size.
  int UpdateMap() {
    Flush();
    std::vector<int32_t> ids;
    for (const ChunkID& c : meshesToUpdate_) { ids.push_back(std::get<0>(c)); ids.push_back(std::get<1>(c)); ids.push_back(std::get<2>(c)); }
    const int nch = (int)meshesToUpdate_.size();
    if (nch > 0) {
      std::vector<int32_t> first((size_t)nch + 1);
      std::vector<float> V, N, C;
      std::vector<uint32_t> K;
      int nv = 0;
      int rc = plvs_hip_tsdf_chisel_mesh_chunks(h_, ids.data(), nch, nullptr, nullptr, nullptr, nullptr, 0, first.data(), &nv);
      if (rc == PLVS_ERR_CAPACITY) {
        V.resize((size_t)3 * nv); N.resize((size_t)3 * nv); C.resize((size_t)3 * nv); K.resize((size_t)nv);
        rc = plvs_hip_tsdf_chisel_mesh_chunks(h_, ids.data(), nch, V.data(), N.data(), C.data(), K.data(), nv, first.data(), &nv);
      }
      check(rc);
      int c = 0;
      for (const ChunkID& id : meshesToUpdate_) {
        const int a = first[(size_t)c], b = first[(size_t)c + 1];
        ++c;
        if (a == b) {
          // RecomputeMesh stores non-empty meshes only (ChunkManager.cpp:165-167) — but it re-uses the mesh object
          // already in allMeshes and GenerateMesh clears it first (:581): an existing mesh becomes empty in place
          auto it = allMeshes_.find(id);
          if (it != allMeshes_.end()) { it->second.vertices.clear(); it->second.normals.clear(); it->second.colors.clear(); it->second.kfids.clear(); }
          continue;
        }
        Mesh& m = allMeshes_[id];
        m.vertices.assign(V.begin() + 3 * a, V.begin() + 3 * b);
        m.normals.assign(N.begin() + 3 * a, N.begin() + 3 * b);
        m.colors.assign(C.begin() + 3 * a, C.begin() + 3 * b);
        m.kfids.assign(K.begin() + a, K.begin() + b);
      }
      meshesToUpdate_.clear();
    }
    pointCloud_.clear();
    for (const auto& kv : allMeshes_) {   // the reference walks an unordered_map: its order is unspecified, this one is by id
      const Mesh& m = kv.second;
      for (size_t i = 0; i < m.kfids.size(); ++i) {
        PointSurfelSegment p;
        std::memset(&p, 0, sizeof p);
        p.x = m.vertices[3 * i]; p.y = m.vertices[3 * i + 1]; p.z = m.vertices[3 * i + 2];
        p.r = (uint8_t)(m.colors[3 * i] * 255);          // point.r = meshCol[0]*255, ChiselServer.cpp:1023-1025
        p.g = (uint8_t)(m.colors[3 * i + 1] * 255);
        p.b = (uint8_t)(m.colors[3 * i + 2] * 255);
        p.normal_x = m.normals[3 * i]; p.normal_y = m.normals[3 * i + 1]; p.normal_z = m.normals[3 * i + 2];
        p.kfid = m.kfids[i];
        pointCloud_.push_back(p);
      }
    }
    return (int)pointCloud_.size();
  }
  // LoadMap once PointCloudMap::LoadMap has read the saved cloud (src/PointCloudMapChisel.cc:527-546):
  // ChiselServer::IntegrateWorldPointCloud(cloud, identity) — every point along its normal
  // (Chisel::IntegrateWorldPointCloudWithNormals) — then UpdateMap.
  int LoadMap(const std::vector<PointSurfelSegment>& cloud) {
    const size_t n = cloud.size();
    xyz_.resize(3 * n); rgb_.resize(3 * n); kfid_.resize(n);
    std::vector<float> nrm(3 * n);
    for (size_t i = 0; i < n; ++i) {
      const PointSurfelSegment& p = cloud[i];
      xyz_[3 * i] = p.x; xyz_[3 * i + 1] = p.y; xyz_[3 * i + 2] = p.z;
      rgb_[3 * i] = p.r; rgb_[3 * i + 1] = p.g; rgb_[3 * i + 2] = p.b;
      nrm[3 * i] = p.normal_x; nrm[3 * i + 1] = p.normal_y; nrm[3 * i + 2] = p.normal_z;
      kfid_[i] = p.kfid;
    }
    const float identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    Flush();
    check(plvs_hip_tsdf_chisel_integrate_world_normals(h_, xyz_.data(), rgb_.data(), kfid_.data(), nrm.data(), (int)n, identity));
    MarkUpdated();
    return UpdateMap();
  }
  void Clear() {
    check(plvs_hip_tsdf_chisel_clear(h_));
    meshesToUpdate_.clear();
    allMeshes_.clear();
    pointCloud_.clear();
  }
  // OnMapChange (src/PointCloudMapChisel.cc:262-274, :389-496).  mapKfidToRt: kfid -> Twc_new * Tcw_at_integration
  // (12 floats: R row-major, then t) for every valid key frame, which the caller derives from its key frames as
  // :420-478 does.  Reset, or UpdateMap + Chisel::Deform (volume and stored meshes) + UpdateMap.
  struct Rt12 { float v[12]; };
  int OnMapChange(const std::map<uint32_t, Rt12>& mapKfidToRt = {}) {
    if (resetOnChange_) { check(plvs_hip_tsdf_chisel_clear(h_)); meshesToUpdate_.clear(); allMeshes_.clear(); }
    if (deformOnChange_) {
      UpdateMap();
      std::vector<uint32_t> kf;
      std::vector<float> rt;
      for (const auto& e : mapKfidToRt) { kf.push_back(e.first); rt.insert(rt.end(), e.second.v, e.second.v + 12); }
      plvs_tsdf_deform_stats st;
      check(plvs_hip_tsdf_chisel_deform(h_, kf.data(), rt.data(), (int)kf.size(), &st));
      for (auto& kv : allMeshes_) {   // ChunkManager.cpp:1020-1051
        Mesh& m = kv.second;
        if (!m.kfids.empty())
          check(plvs_hip_tsdf_chisel_deform_mesh(m.vertices.data(), m.normals.data(), m.kfids.data(), (int)m.kfids.size(), kf.data(),
                                                 rt.data(), (int)kf.size()));
      }
    }
    return UpdateMap();
  }
  const std::vector<PointSurfelSegment>& GetPointCloud() const { return pointCloud_; }
  const std::map<ChunkID, Mesh>& GetAllMeshes() const { return allMeshes_; }
  plvs_tsdf_chisel* handle() { return h_; }

 private:
  void MarkUpdated() {
    int n = 0;
    check(plvs_hip_tsdf_chisel_updated_chunk_ids(h_, nullptr, 0, &n));
    std::vector<int32_t> ids((size_t)3 * (n > 0 ? n : 1));
    if (n > 0) check(plvs_hip_tsdf_chisel_updated_chunk_ids(h_, ids.data(), n, &n));
    for (int i = 0; i < n; ++i)
      for (int dx = -1; dx <= 1; ++dx)
        for (int dy = -1; dy <= 1; ++dy)
          for (int dz = -1; dz <= 1; ++dz)
            meshesToUpdate_.insert(ChunkID(ids[3 * i] + dx, ids[3 * i + 1] + dy, ids[3 * i + 2] + dz));
  }
  plvs_tsdf_chisel* h_ = nullptr;
  bool useCarving_;
  float carvingDist_, near_, far_;
  bool resetOnChange_ = true, deformOnChange_ = false, queue_ = true;
  plvs_scan_camera depthCam_{};
  std::vector<float> xyz_;
  std::vector<uint8_t> rgb_;
  std::vector<uint32_t> kfid_;
  std::set<ChunkID> meshesToUpdate_;
  std::map<ChunkID, Mesh> allMeshes_;
  std::vector<PointSurfelSegment> pointCloud_;
};

// ------------------------------------------------------------------------------------ voxblox map
struct VoxbloxMesh {   // voxblox::Mesh after updateMeshForBlock (three consecutive vertices = one triangle)
  std::vector<float> vertices, normals;   // n x 3
  std::vector<uint8_t> colors;            // n x 4: Color r, g, b, a
};

class PointCloudMapVoxblox {
 public:
  using BlockID = std::tuple<int, int, int>;
  // integrationMethod: PointCloudMapping.voxbloxIntegrationMethod (src/PointCloudMapVoxblox.cc:44, :74) — "simple",
  // "merged" and "fast" are all on the accelerated path, each the one-thread schedule of the reference's integrator bit
  // for bit ("fast": with its two approximate hash sets word for word, kept from scan to scan; plvs_hip.h has the
  // details — on the device it is the slowest of the three: INTEGRATION.md §4).  The default is the reference's own
  // (skIntegrationMethod = "fast", :44); "simple" is the opt-in for speed.
  // queueInsertions ("simple" only): InsertCloud uploads, UpdateMap — the one reader of the layer — integrates what waits as
  // one batch (plvs_hip_tsdf_voxblox_queue / _flush): the same layer bit for bit, at a quarter of the per-key-frame cost.
  explicit PointCloudMapVoxblox(float voxelSize, bool useCarving = false, const std::string& integrationMethod = "fast",
                                bool queueInsertions = true)
      : merged_(integrationMethod == "merged"), fast_(integrationMethod == "fast"),
        queue_(queueInsertions && integrationMethod == "simple") {
    if (integrationMethod != "simple" && integrationMethod != "merged" && integrationMethod != "fast")
      throw std::runtime_error("plvs_hip: unknown voxblox integration method '" + integrationMethod + "'");
    plvs_tsdf_voxblox_params p;
    check(plvs_hip_tsdf_voxblox_default_params(voxelSize, useCarving ? 1 : 0, &p));
    check(plvs_hip_tsdf_voxblox_create(&p, &h_));
  }
  ~PointCloudMapVoxblox() { plvs_hip_tsdf_voxblox_destroy(h_); }
  PointCloudMapVoxblox(const PointCloudMapVoxblox&) = delete;
  PointCloudMapVoxblox& operator=(const PointCloudMapVoxblox&) = delete;

  // InsertCloud: pcl cloud -> voxblox Pointcloud / Colors (r, g, b, a members) -> integratePointCloud
  // (PointCloudMapVoxblox.cc:81-99)
  void InsertCloud(const std::vector<PointSurfelSegment>& cloud_camera, const SE3f& Twc, double /*max_range*/ = 0) {
    const size_t n = cloud_camera.size();
    xyz_.resize(3 * n);
    rgba_.resize(4 * n);
    for (size_t i = 0; i < n; ++i) {
      const PointSurfelSegment& p = cloud_camera[i];
      xyz_[3 * i] = p.x; xyz_[3 * i + 1] = p.y; xyz_[3 * i + 2] = p.z;
      rgba_[4 * i] = p.r; rgba_[4 * i + 1] = p.g; rgba_[4 * i + 2] = p.b; rgba_[4 * i + 3] = p.a;
    }
    if (merged_) check(plvs_hip_tsdf_voxblox_integrate_merged(h_, xyz_.data(), rgba_.data(), (int)n, Twc.m));
    else if (fast_) check(plvs_hip_tsdf_voxblox_integrate_fast(h_, xyz_.data(), rgba_.data(), (int)n, Twc.m));
    else if (queue_) {
      check(plvs_hip_tsdf_voxblox_queue(h_, xyz_.data(), rgba_.data(), (int)n, Twc.m));
      pending_ = true;
      return;
    } else check(plvs_hip_tsdf_voxblox_integrate(h_, xyz_.data(), rgba_.data(), (int)n, Twc.m));
    MarkUpdated();
  }
  // Integrates what InsertCloud has queued (UpdateMap and every other reader of the layer call it).
  void Flush() {
    if (!pending_) return;
    check(plvs_hip_tsdf_voxblox_flush(h_));
    pending_ = false;
    MarkUpdated();
  }
  // The reference's LoadMap leaves the blocks of the loaded cloud outside the layer until the next InsertCloud
  // (integrateWorlPointCloud never publishes them: plvs_hip_tsdf_voxblox_set_deferred_world_blocks) — its UpdateMap
  // meshes none of them.  Off by default (the loaded map shows at once); on = what a PLVS build does today.
  void SetReferenceLoadMapVisibility(bool on) { Flush(); check(plvs_hip_tsdf_voxblox_set_deferred_world_blocks(h_, on ? 1 : 0)); }
  // LoadMap of a saved cloud once PointCloudMap::LoadMap has read it (src/PointCloudMapVoxblox.cc:233-258):
  // TsdfServer::insertWorldPointCloud(cloud, identity) — every point along its normal — then UpdateMap.
  int LoadMap(const std::vector<PointSurfelSegment>& cloud) {
    Flush();
    const size_t n = cloud.size();
    xyz_.resize(3 * n);
    rgba_.resize(4 * n);
    std::vector<float> nrm(3 * n);
    for (size_t i = 0; i < n; ++i) {
      const PointSurfelSegment& p = cloud[i];
      xyz_[3 * i] = p.x; xyz_[3 * i + 1] = p.y; xyz_[3 * i + 2] = p.z;
      rgba_[4 * i] = p.r; rgba_[4 * i + 1] = p.g; rgba_[4 * i + 2] = p.b; rgba_[4 * i + 3] = p.a;
      nrm[3 * i] = p.normal_x; nrm[3 * i + 1] = p.normal_y; nrm[3 * i + 2] = p.normal_z;
    }
    const float identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    check(plvs_hip_tsdf_voxblox_integrate_world_normals(h_, xyz_.data(), rgba_.data(), nrm.data(), (int)n, identity));
    MarkUpdated();
    return UpdateMap();
  }
  // UpdateMap: TsdfServer::updateMesh (generateMesh(only_mesh_updated_blocks, clear_updated_flag), tsdf_server.cc:775-787)
  // + getMeshAsPointcloud (voxblox_ros/mesh_vis.h:272-318, ColorMode::kColor)  (src/PointCloudMapVoxblox.cc:160-179).
  // Returns the cloud size.
  int UpdateMap() {
    Flush();
    const int nb = (int)updated_.size();
    if (nb > 0) {
      std::vector<int32_t> ids;
      for (const BlockID& b : updated_) { ids.push_back(std::get<0>(b)); ids.push_back(std::get<1>(b)); ids.push_back(std::get<2>(b)); }
      std::vector<int32_t> first((size_t)nb + 1);
      std::vector<float> V, N;
      std::vector<uint8_t> C;
      int nv = 0;
      int rc = plvs_hip_tsdf_voxblox_mesh_blocks(h_, ids.data(), nb, nullptr, nullptr, nullptr, 0, first.data(), &nv);
      if (rc == PLVS_ERR_CAPACITY) {
        V.resize((size_t)3 * nv); N.resize((size_t)3 * nv); C.resize((size_t)4 * nv);
        rc = plvs_hip_tsdf_voxblox_mesh_blocks(h_, ids.data(), nb, V.data(), N.data(), C.data(), nv, first.data(), &nv);
      }
      check(rc);
      int c = 0;
      for (const BlockID& id : updated_) {   // allocateMeshPtrByIndex + mesh->clear(): an updated block always owns a mesh
        const int a = first[(size_t)c], b = first[(size_t)c + 1];
        ++c;
        VoxbloxMesh& m = meshLayer_[id];
        m.vertices.assign(V.begin() + 3 * a, V.begin() + 3 * b);
        m.normals.assign(N.begin() + 3 * a, N.begin() + 3 * b);
        m.colors.assign(C.begin() + 4 * a, C.begin() + 4 * b);
      }
      updated_.clear();
    }
    pointCloud_.clear();
    for (const auto& kv : meshLayer_) {   // the reference walks an unordered_map: its order is unspecified, this one is by id
      const VoxbloxMesh& m = kv.second;
      for (size_t i = 0; i < m.vertices.size() / 3; ++i) {
        PointSurfelSegment p;
        std::memset(&p, 0, sizeof p);
        p.x = m.vertices[3 * i]; p.y = m.vertices[3 * i + 1]; p.z = m.vertices[3 * i + 2];
        p.r = CloudColour(m.colors[4 * i]); p.g = CloudColour(m.colors[4 * i + 1]); p.b = CloudColour(m.colors[4 * i + 2]);
        p.normal_x = m.normals[3 * i]; p.normal_y = m.normals[3 * i + 1]; p.normal_z = m.normals[3 * i + 2];
        pointCloud_.push_back(p);
      }
    }
    return (int)pointCloud_.size();
  }
  void Clear() {
    check(plvs_hip_tsdf_voxblox_clear(h_));   // (drops what was queued)
    pending_ = false;
    updated_.clear();
    meshLayer_.clear();
    pointCloud_.clear();
  }
  int NumBlocks() { Flush(); int n = 0; check(plvs_hip_tsdf_voxblox_num_blocks(h_, &n)); return n; }
  // The device side of TsdfServer::saveMap / loadMap (tsdf_server.cc:859-872): every block's voxel planes out of /
  // into HBM; the `.proto` serialisation of a StoredBlock stays with the reference's protobuf code.  A loaded block
  // replaces / creates its block and is marked updated (BlockMergingStrategy::kReplace, core/layer_inl.h:195-197, :215).
  struct StoredBlock {
    BlockID id;
    std::vector<float> distance, weight;   // 4096 each, index x + 16 * (y + 16 * z)
    std::vector<uint32_t> rgba;
  };
  std::vector<StoredBlock> SaveLayer() {
    const int n = NumBlocks();
    std::vector<int32_t> ids((size_t)3 * (n > 0 ? n : 1));
    int m = 0;
    check(plvs_hip_tsdf_voxblox_block_ids(h_, ids.data(), n, &m));
    std::vector<StoredBlock> out((size_t)n);
    for (int i = 0; i < n; ++i) {
      StoredBlock& b = out[(size_t)i];
      b.id = BlockID(ids[3 * i], ids[3 * i + 1], ids[3 * i + 2]);
      b.distance.resize(4096); b.weight.resize(4096); b.rgba.resize(4096);
      check(plvs_hip_tsdf_voxblox_download_block(h_, ids[3 * i], ids[3 * i + 1], ids[3 * i + 2], b.distance.data(), b.weight.data(),
                                                 b.rgba.data()));
    }
    return out;
  }
  bool LoadLayer(const std::vector<StoredBlock>& blocks) {
    Flush();
    for (const StoredBlock& b : blocks) {
      check(plvs_hip_tsdf_voxblox_upload_block(h_, std::get<0>(b.id), std::get<1>(b.id), std::get<2>(b.id), b.distance.data(),
                                               b.weight.data(), b.rgba.data()));
      updated_.insert(b.id);
    }
    return true;
  }
  const std::vector<PointSurfelSegment>& GetPointCloud() const { return pointCloud_; }
  const std::map<BlockID, VoxbloxMesh>& GetMeshLayer() const { return meshLayer_; }
  plvs_tsdf_voxblox* handle() { return h_; }

 private:
  // every block the integrator touched has updated() set (tsdf_integrator.cc:151) until the next updateMesh
  void MarkUpdated() {
    int nu = 0;
    check(plvs_hip_tsdf_voxblox_updated_block_ids(h_, nullptr, 0, &nu));
    std::vector<int32_t> ids((size_t)3 * (nu > 0 ? nu : 1));
    if (nu > 0) check(plvs_hip_tsdf_voxblox_updated_block_ids(h_, ids.data(), nu, &nu));
    for (int i = 0; i < nu; ++i) updated_.insert(BlockID(ids[3 * i], ids[3 * i + 1], ids[3 * i + 2]));
  }
  // colorVoxbloxToMsg then colorMsgToVoxblox (voxblox_ros/conversions.h:44-60): through a float in [0, 1] and back
  static uint8_t CloudColour(uint8_t c) {
    const float msg = (float)(c / 255.0);
    return (uint8_t)(msg * 255.0);
  }
  plvs_tsdf_voxblox* h_ = nullptr;
  bool merged_ = false;
  bool fast_ = false;
  bool queue_ = false, pending_ = false;
  std::vector<float> xyz_;
  std::vector<uint8_t> rgba_;
  std::set<BlockID> updated_;
  std::map<BlockID, VoxbloxMesh> meshLayer_;
  std::vector<PointSurfelSegment> pointCloud_;
};

}  // namespace PLVS2hip
