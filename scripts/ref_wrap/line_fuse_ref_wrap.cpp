// The reference's own LineMatcher::Fuse(pKF, vpMapLines, th, bRight) (src/LineMatcher.cc:2043-2315), both
// KeyFrame::GetLineFeaturesInArea overloads it reaches (src/KeyFrame.cc:1291-1402), LineProjection::ProjectLineWithCheck
// (include/LineProjection.h:144-264), Geom2DUtils::GetLine2dRepresentationNoTheta / GetLine2dRepresentation
// (include/Geom2DUtils.h:135-159), MapLine::PredictScale(const float&, KeyFramePtr&) (src/MapLine.cc:721-736),
// MapLine::GetMinDistanceInvariance / GetMaxDistanceInvariance (:707-719), GeometricCamera::projectLinear(const Eigen::Vector3f&)
// (include/CameraModels/GeometricCamera.h:197-203), the constants kChiSquareLinePointProj, LineMatcher::TH_LOW, Frame::kDeltaTheta /
// kDeltaD, the grid macros of include/Frame.h:70-73 and the #defines of src/LineMatcher.cc:38-40 and src/MapLine.cc:33, behind a C
// interface.  This file holds declarations, recording accessors and calls: the DEFINITIONS are cut verbatim out of the reference
// tree into line_fuse_cut_*.inc at build time (scripts/make_line_fuse_golden.py) and compiled here, against oracle/ref/eigen_full,
// with -O2 -ffp-contract=off -fno-fast-math.  The classes below carry exactly the members those definitions touch.
//
// What Fuse does per pair is RECORDED by the accessors it calls, not inferred.  The cut functions that are accessors themselves
// (projectLinear, the two distance getters, PredictScale) are compiled under another name (a #define around their cut) and
// called by a recording member of the reference's name: GetWorldEndPoints (the pair was not skipped), projectLinear (count and
// values: the middle, the start, the end), GetMaxDistanceInvariance (the middle was inside), GetNormal (ProjectLineWithCheck
// returned true), PredictScale (the viewing angle passed; its level), GetDescriptor (the window was not empty),
// DescriptorDistance (a candidate passed the level band and the gates; count and minimum), GetMapLine / AddObservation /
// AddMapLine (bestDist <= TH_LOW, with bestIdx).  GetMapLine returns null, so the run mutates nothing that a later pair reads.
//
// RESTATED, not compiled — each marked where it stands:
//   * FrameTransformsForLineProjection (include/LineProjection.h:34-75): the four members, filled from the pose handed in;
//   * LineMatcher::DescriptorDistance (src/LineMatcher.cc:2658-2680), as a recording accessor;
//   * Frame::PosLineInGrid and the grid's filling (src/Frame.cc:1477-1495, :757-790), whose mLineGrid the key frame copies —
//     through the cut GetLine2dRepresentation;
//   * which test a pair stopped at between GetMaxDistanceInvariance and GetNormal (ref_line_fuse: `stop`), from the comparisons of
//     include/LineProjection.h:193-251.
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <limits>
#include <memory>
#include <mutex>
#include <vector>

#include <Eigen/Core>

using namespace std;

#include "line_fuse_cut_macros.inc"

#define MSG_ASSERT(cond, msg) do { if (!(cond)) { std::cerr << msg << std::endl; std::abort(); } } while (0)
#define VERBOSE 0

namespace cv {   // the OpenCV types the cut text names
struct Mat {
  const uint8_t* p = nullptr;
  Mat row(size_t i) const { Mat m; m.p = p + 32 * i; return m; }
};
namespace line_descriptor_c {
struct KeyLine {
  float startPointX = 0, startPointY = 0, endPointX = 0, endPointY = 0;
  int octave = 0;
};
}  // namespace line_descriptor_c
}  // namespace cv

namespace PLVS2 {

struct PairRecord {
  int32_t flags = 0, n_proj = 0, n_dist = 0, min_dist_seen = 256, best_idx = -1, level = -1;
  float proj[6] = {0, 0, 0, 0, 0, 0};
};
enum { kGotEndPoints = 1, kGotMaxDistance = 2, kGotNormal = 4, kPredicted = 8, kGotDescriptor = 16, kGotMapLine = 32, kAddObservation = 64,
       kAddMapLine = 128, kReplace = 256 };
static PairRecord* g_rec = nullptr;   // the pair Fuse is at: set by isBad

struct Line2DRepresentation {   // the four members of include/Geom2DUtils.h:31-42, zero as its constructor leaves them
  float theta = 0, nx = 0, ny = 0, d = 0;
};
class Geom2DUtils {
 public:
#include "line_fuse_cut_geom.inc"
};

class GeometricCamera {
 public:
  enum { CAM_PINHOLE = 0, CAM_FISHEYE = 1 };
  virtual ~GeometricCamera() {}
  virtual Eigen::Vector2f project(const Eigen::Vector3f& v3D) const { return projectLinearCut(v3D); }   // (pinhole: never called)
  Eigen::Vector2f projectLinearCut(const Eigen::Vector3f& v3D) const;
  Eigen::Vector2f projectLinear(const Eigen::Vector3f& v3D) const {
    const Eigen::Vector2f uv = projectLinearCut(v3D);
    if (g_rec->n_proj < 3) { g_rec->proj[2 * g_rec->n_proj] = uv(0); g_rec->proj[2 * g_rec->n_proj + 1] = uv(1); }
    ++g_rec->n_proj;
    return uv;
  }
  unsigned int GetType() const { return mnType; }
  std::vector<float> mvParameters, mvLinearParameters;
  unsigned int mnType = CAM_PINHOLE;
};

class Frame {
 public:
  static const float kDeltaTheta;
  static const float kDeltaD;
};

class KeyFrame;
class MapLine;
typedef KeyFrame* KeyFramePtr;
typedef MapLine* MapLinePtr;

class KeyFrame {
 public:
  Eigen::Vector3f GetCameraCenter() { return mOw; }
  Eigen::Vector3f GetRightCameraCenter() { return mOw; }
  vector<size_t> GetLineFeaturesInArea(const Line2DRepresentation& lineRepresentation, const float& dtheta, const float& dd, const bool bRight = false) const;
  void GetLineFeaturesInArea(const float thetaMin, const float thetaMax, const float dMin, const float dMax, vector<size_t>& vIndices,
                             const bool bRight = false) const;
  MapLinePtr GetMapLine(const size_t& idx) { g_rec->flags |= kGotMapLine; g_rec->best_idx = (int32_t)idx; return nullptr; }
  void AddMapLine(MapLinePtr, const size_t&) { g_rec->flags |= kAddMapLine; }
  Eigen::Matrix3f mRcw;
  Eigen::Vector3f mtcw, mOw;
  GeometricCamera *mpCamera = nullptr, *mpCamera2 = nullptr;
  float mbf = 0;
  int Nlines = 0, NlinesLeft = -1;
  int mnMinX = 0, mnMinY = 0, mnMaxX = 0, mnMaxY = 0, mnMaxDiag = 0;   // int in the reference's KeyFrame (include/KeyFrame.h:366)
  float mfLineGridElementThetaInv = 0, mfLineGridElementDInv = 0;
  float mfLineLogScaleFactor = 0;
  int mnLineScaleLevels = 0;
  vector<float> mvLineScaleFactors, mvLineInvLevelSigma2, mvuRightLineStart, mvuRightLineEnd;
  vector<cv::line_descriptor_c::KeyLine> mvKeyLinesUn, mvKeyLinesRightUn;
  cv::Mat mLineDescriptors;
  vector<vector<vector<size_t>>> mLineGrid, mLineGridRight;
};

class MapLine {
 public:
  bool isBad() { g_rec = rec; return skip == 2; }
  bool IsInKeyFrame(KeyFramePtr) { return skip == 3; }
  void GetWorldEndPoints(Eigen::Vector3f& s, Eigen::Vector3f& e) { rec->flags |= kGotEndPoints; s = mWorldPosStart; e = mWorldPosEnd; }
  Eigen::Vector3f GetNormal() { rec->flags |= kGotNormal; return mNormalVector; }
  float GetMinDistanceInvarianceCut();
  float GetMaxDistanceInvarianceCut();
  float GetMinDistanceInvariance() { return GetMinDistanceInvarianceCut(); }
  float GetMaxDistanceInvariance() { rec->flags |= kGotMaxDistance; return GetMaxDistanceInvarianceCut(); }
  int PredictScaleCut(const float& currentDist, KeyFramePtr& pKF);
  int PredictScale(const float& currentDist, KeyFramePtr& pKF) {
    rec->flags |= kPredicted;
    rec->level = PredictScaleCut(currentDist, pKF);
    return rec->level;
  }
  cv::Mat GetDescriptor() { rec->flags |= kGotDescriptor; return mDescriptor; }
  int Observations() { return 1; }
  void Replace(MapLinePtr) { rec->flags |= kReplace; }
  void AddObservation(KeyFramePtr, size_t idx) { rec->flags |= kAddObservation; rec->best_idx = (int32_t)idx; }
  Eigen::Vector3f mWorldPosStart, mWorldPosEnd, mNormalVector;
  float mfMaxDistance = 0;
  cv::Mat mDescriptor;
  std::mutex mMutexPos;
  int skip = 0;
  PairRecord* rec = nullptr;
};

struct FrameTransformsForLineProjection {   // RESTATED include/LineProjection.h:34-75
  explicit FrameTransformsForLineProjection(KeyFrame& F) : mRcw(F.mRcw), mRrw(F.mRcw), mtcw(F.mtcw), mtrw(F.mtcw) {}
  Eigen::Matrix3f mRcw, mRrw;
  Eigen::Vector3f mtcw, mtrw;
};

class LineProjection {   // the members of include/LineProjection.h:78-103, zero as its constructor leaves them
 public:
  template <typename FrameType>
  bool ProjectLineWithCheck(const MapLinePtr& pML, const FrameType& F, const FrameTransformsForLineProjection& frameTfs, bool bRight = false);
  float uS = 0, vS = 0, uE = 0, vE = 0, uM = 0, vM = 0, invSz = 0, invEz = 0;
  float distMiddlePoint = 0;
  Eigen::Vector3f p3DMw;
};

class LineMatcher {
 public:
  static const int TH_LOW;
  int Fuse(KeyFramePtr& pKF, const vector<MapLinePtr>& vpMapLines, const float th = 3.0, const bool bRight = false);
  // RESTATED src/LineMatcher.cc:2658-2680 (the bit trick counts the differing bits), recording
  static int DescriptorDistance(const cv::Mat& a, const cv::Mat& b) {
    int dist = 0;
    for (int i = 0; i < 32; ++i) dist += __builtin_popcount((unsigned)(a.p[i] ^ b.p[i]));
    ++g_rec->n_dist;
    if (dist < g_rec->min_dist_seen) g_rec->min_dist_seen = dist;
    return dist;
  }
};

#define projectLinear projectLinearCut
#define GetMinDistanceInvariance GetMinDistanceInvarianceCut
#define GetMaxDistanceInvariance GetMaxDistanceInvarianceCut
#define PredictScale PredictScaleCut
#include "line_fuse_cut_accessors.inc"
#undef projectLinear
#undef GetMinDistanceInvariance
#undef GetMaxDistanceInvariance
#undef PredictScale

template <typename FrameType>
#include "line_fuse_cut_lineproj.inc"

#include "line_fuse_cut_defs.inc"

}  // namespace PLVS2

using namespace PLVS2;

namespace {
struct KfHolder {
  KeyFrame kf;
  GeometricCamera cam;
};
}  // namespace

extern "C" {

int ref_use_endpoints_averaging() { return USE_ENDPOINTS_AVERAGING; }
int ref_use_distsegment2segment() { return USE_DISTSEGMENT2SEGMENT_FOR_MATCHING; }
int ref_use_stereo_projection_check() { return USE_STEREO_PROJECTION_CHECK; }
int ref_th_low() { return LineMatcher::TH_LOW; }
float ref_chi_square() { return kChiSquareLinePointProj; }

// segs: n x 4 = startPointX, startPointY, endPointX, endPointY of mvKeyLinesUn; u_right_start / end: NULL = the vectors are empty;
// bounds4: mnMinX, mnMaxX, mnMinY, mnMaxY (integral); max_diag: the Frame's float mnMaxDiag.  in_grid (n): whether PosLineInGrid placed
// the key line.
void* ref_line_kf_create(int n, const float* segs, const int32_t* octave, const float* u_right_start, const float* u_right_end, const uint8_t* desc,
                         const float* bounds4, float max_diag, const float* K4, float mbf, const float* Rcw, const float* tcw, const float* Ow,
                         int n_levels, const float* scale_factors, const float* inv_sigma2, float log_scale_factor, uint8_t* in_grid) {
  KfHolder* h = new KfHolder;
  KeyFrame& kf = h->kf;
  h->cam.mvLinearParameters.assign(K4, K4 + 4);
  h->cam.mvParameters.assign(K4, K4 + 4);
  kf.mpCamera = &h->cam;
  kf.mbf = mbf;
  for (int c = 0; c < 3; ++c)
    for (int r = 0; r < 3; ++r) kf.mRcw(r, c) = Rcw[3 * c + r];   // Eigen's own layout: column-major
  kf.mtcw = Eigen::Vector3f(tcw[0], tcw[1], tcw[2]);
  kf.mOw = Eigen::Vector3f(Ow[0], Ow[1], Ow[2]);
  kf.Nlines = n;
  kf.mnMinX = (int)bounds4[0]; kf.mnMaxX = (int)bounds4[1]; kf.mnMinY = (int)bounds4[2]; kf.mnMaxY = (int)bounds4[3];
  // src/Frame.cc:264-265 with the Frame's float mnMaxDiag; src/KeyFrame.cc:121, :144: the key frame copies the two inverses and
  // truncates the diagonal to int
  const float frame_diag = max_diag;
  kf.mfLineGridElementThetaInv = static_cast<float>(LINE_THETA_GRID_ROWS) / static_cast<float>(LINE_THETA_SPAN);
  kf.mfLineGridElementDInv = static_cast<float>(LINE_D_GRID_COLS) / (2.0f * frame_diag);
  kf.mnMaxDiag = frame_diag;
  kf.mfLineLogScaleFactor = log_scale_factor; kf.mnLineScaleLevels = n_levels;
  kf.mvLineScaleFactors.assign(scale_factors, scale_factors + n_levels);
  kf.mvLineInvLevelSigma2.assign(inv_sigma2, inv_sigma2 + n_levels);
  if (u_right_start) {
    kf.mvuRightLineStart.assign(u_right_start, u_right_start + n);
    kf.mvuRightLineEnd.assign(u_right_end, u_right_end + n);
  }
  kf.mvKeyLinesUn.resize(n);
  kf.mLineDescriptors.p = desc;
  kf.mLineGrid.assign(LINE_D_GRID_COLS, vector<vector<size_t>>(LINE_THETA_GRID_ROWS));
  for (int i = 0; i < n; ++i) {
    cv::line_descriptor_c::KeyLine& kl = kf.mvKeyLinesUn[i];
    kl.startPointX = segs[4 * i]; kl.startPointY = segs[4 * i + 1]; kl.endPointX = segs[4 * i + 2]; kl.endPointY = segs[4 * i + 3];
    kl.octave = octave[i];
    // RESTATED src/Frame.cc:1477-1495 (PosLineInGrid, with Frame::mnMaxDiag a float) and the filling loop of :757-790
    Line2DRepresentation lineRepresentation;
    Geom2DUtils::GetLine2dRepresentation(kl.startPointX, kl.startPointY, kl.endPointX, kl.endPointY, lineRepresentation);
    const int posYrow = round((lineRepresentation.theta - LINE_THETA_MIN) * kf.mfLineGridElementThetaInv);
    const int posXcol = round((lineRepresentation.d + frame_diag) * kf.mfLineGridElementDInv);
    in_grid[i] = !(posYrow < 0 || posYrow >= LINE_THETA_GRID_ROWS || posXcol < 0 || posXcol >= LINE_D_GRID_COLS);
    if (in_grid[i]) kf.mLineGrid[posXcol][posYrow].push_back(i);
  }
  return h;
}
void ref_line_kf_destroy(void* h) { delete static_cast<KfHolder*>(h); }

// One call of the reference's Fuse.  skip[i]: 0, or 1 = null pointer, 2 = isBad(), 3 = IsInKeyFrame(pKF).  rec: m x {flags, n_proj,
// n_dist, min_dist_seen, best_idx, level}, proj: m x 6 (uM, vM, uS, vS, uE, vE as far as projectLinear was called), stop: m — for the
// pairs that called GetMaxDistanceInvariance but not GetNormal, RESTATED from include/LineProjection.h:193-251: 1 = too near, 2 = too
// far, 3 = an end point behind, 4 = an end point outside.
int ref_line_fuse(void* h, int m, const float* start, const float* end, const float* normal, const float* max_dist, const uint8_t* desc,
                  const uint8_t* skip, float th, int32_t* rec, float* proj, int32_t* stop) {
  KeyFramePtr pKF = &static_cast<KfHolder*>(h)->kf;
  vector<MapLine> store(m);
  vector<PairRecord> records(m);
  vector<MapLinePtr> vp(m, nullptr);
  for (int i = 0; i < m; ++i) {
    MapLine& p = store[i];
    p.mWorldPosStart = Eigen::Vector3f(start[3 * i], start[3 * i + 1], start[3 * i + 2]);
    p.mWorldPosEnd = Eigen::Vector3f(end[3 * i], end[3 * i + 1], end[3 * i + 2]);
    p.mNormalVector = Eigen::Vector3f(normal[3 * i], normal[3 * i + 1], normal[3 * i + 2]);
    p.mfMaxDistance = max_dist[i];
    p.mDescriptor.p = desc + 32 * (size_t)i;
    p.skip = skip ? skip[i] : 0;
    p.rec = &records[i];
    if (p.skip != 1) vp[i] = &p;
  }
  LineMatcher matcher;
  const int fused = matcher.Fuse(pKF, vp, th, false);
  for (int i = 0; i < m; ++i) {
    const PairRecord& r = records[i];
    int32_t* o = rec + 6 * (size_t)i;
    o[0] = r.flags; o[1] = r.n_proj; o[2] = r.n_dist; o[3] = r.min_dist_seen; o[4] = r.best_idx; o[5] = r.level;
    for (int c = 0; c < 6; ++c) proj[6 * (size_t)i + c] = r.proj[c];
    stop[i] = 0;
    if ((r.flags & kGotMaxDistance) && !(r.flags & kGotNormal)) {   // RESTATED include/LineProjection.h:189-251
      const Eigen::Vector3f p3DMw = 0.5 * (store[i].mWorldPosStart + store[i].mWorldPosEnd);
      const Eigen::Vector3f p3DMc = pKF->mRcw * p3DMw + pKF->mtcw;
      const float distMiddlePoint = p3DMc.norm();
      if (distMiddlePoint < 0.8f * max_dist[i]) stop[i] = 1;
      else if (distMiddlePoint > 1.2f * max_dist[i]) stop[i] = 2;
      else stop[i] = r.n_proj == 1 ? 3 : 4;
    }
  }
  return fused;
}

// the same call without the records read back: for timing
int ref_line_fuse_plain(void* h, int m, const float* start, const float* end, const float* normal, const float* max_dist, const uint8_t* desc,
                        const uint8_t* skip, float th) {
  vector<int32_t> rec(6 * (size_t)m), stop(m);
  vector<float> proj(6 * (size_t)m);
  return ref_line_fuse(h, m, start, end, normal, max_dist, desc, skip, th, rec.data(), proj.data(), stop.data());
}

int ref_line_predict_scale(float dist, float max_dist, float log_scale_factor, int levels) {
  KeyFrame kf;
  kf.mfLineLogScaleFactor = log_scale_factor; kf.mnLineScaleLevels = levels;
  KeyFramePtr p = &kf;
  MapLine ml;
  PairRecord r;
  ml.rec = &r;
  ml.mfMaxDistance = max_dist;
  return ml.PredictScale(dist, p);
}

// theta of the cut GetLine2dRepresentation alone
float ref_line_theta(float xs, float ys, float xe, float ye) {
  Line2DRepresentation r;
  Geom2DUtils::GetLine2dRepresentation(xs, ys, xe, ye, r);
  return r.theta;
}

}  // extern "C"
