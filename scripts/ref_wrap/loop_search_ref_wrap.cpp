// The reference's own loop-closing SearchByProjection overloads behind a C interface, compiled twice
// (scripts/make_loop_search_golden.py).  -DLOOP_SEARCH_WRAP_POINTS:
//   ORBmatcher::SearchByProjection(KeyFramePtr&, Sophus::Sim3f&, const vector<MapPointPtr>&, vector<MapPointPtr>&, int, float)
//                                                                                                      (src/ORBmatcher.cc:509-615)
//   ORBmatcher::SearchByProjection(KeyFramePtr&, Sophus::Sim3<float>&, const std::vector<MapPointPtr>&, const std::vector<KeyFramePtr>&,
//                                  std::vector<MapPointPtr>&, std::vector<KeyFramePtr>&, int, float)                   (:617-730)
// with KeyFrame::GetFeaturesInArea, KeyFrame::IsInImage, MapPoint::PredictScale(const float&, KeyFramePtr&), Pinhole::project(const
// Eigen::Vector3f&) and the three statements of Sophus' point action.  -DLOOP_SEARCH_WRAP_LINES:
//   LineMatcher::SearchByProjection(KeyFramePtr&, const Sophus::Sim3f&, const vector<MapLinePtr>&, vector<MapLinePtr>&, int, float)
//                                                                                                   (src/LineMatcher.cc:1767-1909)
//   LineMatcher::SearchByProjection(KeyFramePtr&, const Sophus::Sim3f&, const std::vector<MapLinePtr>&, const std::vector<KeyFramePtr>&,
//                                   std::vector<MapLinePtr>&, std::vector<KeyFramePtr>&, int, float)                (:1913-2037)
// with both KeyFrame::GetLineFeaturesInArea overloads, LineProjection::ProjectLineWithCheck,
// Geom2DUtils::GetLine2dRepresentation(NoTheta), MapLine::PredictScale, the two distance getters, GeometricCamera::projectLinear,
// the constants and the #defines.
// This file holds declarations, recording accessors and calls, as scripts/ref_wrap/loop_fuse_ref_wrap.cpp does for the Sim3 Fuse:
// the DEFINITIONS are cut verbatim out of the reference tree into loop_search_cut_*.inc at build time and compiled here, against
// oracle/ref/eigen_full, with -O2 -ffp-contract=off -fno-fast-math.  What a call does per pair is RECORDED by the accessors it
// calls; the match itself is read back from vpMatched / vpMatchedKF after the call.
//
// Two cut definitions are compiled under another name so that a recording member of the reference's name can stand in front of
// them: KeyFrame::IsInImage (records the u, v either overload tests — the second overload's are locals nothing else sees) and
// MapPoint::PredictScale (records the level).  The rename is a #define around the one #include; the text is untouched.
//
// OUTSIDE THE PIN: the decomposition of Scw — Sophus::Sim3f / SE3f below are stand-ins that hand the scenario's decomposed pose
// through, as in loop_fuse_ref_wrap.cpp.  Scw.translation() / Scw.scale() IS compiled: a per-component f32 division.
//
// RESTATED, not compiled — each marked where it stands.
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <limits>
#include <memory>
#include <mutex>
#include <unordered_set>
#include <vector>

#include <Eigen/Core>

using namespace std;

#if defined(LOOP_SEARCH_WRAP_POINTS)

namespace cv {   // the three OpenCV types the cut text names
struct Point2f { float x = 0, y = 0; };
struct KeyPoint { Point2f pt; int octave = 0; };
struct Mat {
  const uint8_t* p = nullptr;
  Mat row(size_t i) const { Mat m; m.p = p + 32 * i; return m; }
};
}  // namespace cv

namespace {
struct Quat {   // the unit quaternion as Sophus::SO3f hands it to the three statements
  Eigen::Vector3f v;
  float s;
  const Eigen::Vector3f& vec() const { return v; }
  float w() const { return s; }
};
template <class PointDerived>
using PointProduct = Eigen::Vector3f;
template <class PointDerived>
PointProduct<PointDerived> so3_times(const Quat& q, const PointDerived& p) {   // Sophus::SO3f::operator*(point): the body is the cut
#include "loop_search_cut_so3.inc"
}
struct RecordedPose {   // the scenario's decomposition of Scw (outside the pin, see the head)
  Eigen::Matrix3f R;
  Eigen::Vector3f s_t, ow_points;
  float scale = 1;
  Quat q;
};
const RecordedPose* g_pose = nullptr;
}  // namespace

namespace Sophus {
struct SE3f {
  struct Inverse {
    Eigen::Vector3f t;
    Eigen::Vector3f translation() const { return t; }
  };
  Quat q;
  Eigen::Vector3f t;
  SE3f() {}
  SE3f(const Eigen::Matrix3f&, const Eigen::Vector3f& t_) : q(g_pose->q), t(t_) {}                 // STAND-IN: the recorded quaternion
  Eigen::Vector3f operator*(const Eigen::Vector3f& p) const { return so3_times(q, p) + t; }       // RESTATED se3.hpp:323
  Inverse inverse() const { return Inverse{g_pose->ow_points}; }                                  // STAND-IN: the recorded centre
};
template <class Scalar>
struct Sim3 {   // STAND-IN: the recorded fields
  Eigen::Matrix3f rotationMatrix() const { return g_pose->R; }
  Eigen::Vector3f translation() const { return g_pose->s_t; }
  float scale() const { return g_pose->scale; }
};
typedef Sim3<float> Sim3f;
}  // namespace Sophus

namespace PLVS2 {

class GeometricCamera {
 public:
  virtual ~GeometricCamera() {}
  virtual Eigen::Vector2f project(const Eigen::Vector3f& v3D) const = 0;
  std::vector<float> mvParameters;
};
class Pinhole : public GeometricCamera {
 public:
  Eigen::Vector2f project(const Eigen::Vector3f& v3D) const;
};

struct PairRecord {
  int32_t flags = 0, n_dist = 0, min_dist_seen = 256, level = -1;
  float u = 0, v = 0;
};
enum { kGotWorldPos = 1, kCameraProject = 2, kImageTested = 4, kGotMaxDistance = 8, kGotNormal = 16, kPredicted = 32, kGotDescriptor = 64 };
static PairRecord* g_rec = nullptr;   // the pair the call is at: set through isBad

class RecordingPinhole : public Pinhole {
 public:
  Eigen::Vector2f project(const Eigen::Vector3f& v3D) const {
    g_rec->flags |= kCameraProject;
    return Pinhole::project(v3D);
  }
};

class KeyFrame;
class MapPoint;
typedef KeyFrame* KeyFramePtr;
typedef MapPoint* MapPointPtr;

class KeyFrame {
 public:
  bool IsInImageCut(const float& x, const float& y) const;   // the cut definition (see the head)
  bool IsInImage(const float& x, const float& y) const {
    g_rec->flags |= kImageTested;
    g_rec->u = x; g_rec->v = y;
    return IsInImageCut(x, y);
  }
  vector<size_t> GetFeaturesInArea(const float& x, const float& y, const float& r, const bool bRight = false) const;
  GeometricCamera *mpCamera = nullptr, *mpCamera2 = nullptr;
  float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
  int N = 0, NLeft = -1;
  int mnMinX = 0, mnMinY = 0, mnMaxX = 0, mnMaxY = 0;          // int in the reference's KeyFrame (include/KeyFrame.h)
  int mnGridCols = 64, mnGridRows = 48;
  float mfGridElementWidthInv = 0, mfGridElementHeightInv = 0;
  float mfLogScaleFactor = 0;
  int mnScaleLevels = 0;
  vector<float> mvScaleFactors, mvInvLevelSigma2, mvuRight;
  vector<cv::KeyPoint> mvKeysUn, mvKeys, mvKeysRight;
  cv::Mat mDescriptors;
  vector<vector<vector<size_t>>> mGrid, mGridRight;
};

class MapPoint {
 public:
  bool isBad() { g_rec = rec; return skip == 2; }
  Eigen::Vector3f GetWorldPos() { rec->flags |= kGotWorldPos; return mWorldPos; }
  Eigen::Vector3f GetNormal() { rec->flags |= kGotNormal; return mNormalVector; }
  float GetMinDistanceInvariance() { return 0.8f * mfMinDistance; }                                   // RESTATED src/MapPoint.cc:572
  float GetMaxDistanceInvariance() { rec->flags |= kGotMaxDistance; return 1.2f * mfMaxDistance; }    // RESTATED src/MapPoint.cc:578
  int PredictScaleCut(const float& currentDist, KeyFramePtr& pKF);   // the cut definition (see the head)
  int PredictScale(const float& currentDist, KeyFramePtr& pKF) {
    rec->flags |= kPredicted;
    return rec->level = PredictScaleCut(currentDist, pKF);
  }
  cv::Mat GetDescriptor() { rec->flags |= kGotDescriptor; return mDescriptor; }
  Eigen::Vector3f mWorldPos, mNormalVector;
  float mfMinDistance = 0, mfMaxDistance = 0;
  cv::Mat mDescriptor;
  std::mutex mMutexPos;
  int skip = 0;
  PairRecord* rec = nullptr;
};

class ORBmatcher {
 public:
  static const int TH_LOW = 50;   // src/ORBmatcher.cc:58
  int SearchByProjection(KeyFramePtr& pKF, Sophus::Sim3f& Scw, const vector<MapPointPtr>& vpPoints, vector<MapPointPtr>& vpMatched, int th,
                         float ratioHamming);
  int SearchByProjection(KeyFramePtr& pKF, Sophus::Sim3<float>& Scw, const std::vector<MapPointPtr>& vpPoints,
                         const std::vector<KeyFramePtr>& vpPointsKFs, std::vector<MapPointPtr>& vpMatched, std::vector<KeyFramePtr>& vpMatchedKF,
                         int th, float ratioHamming);
  // RESTATED src/ORBmatcher.cc:2198-2217 (the bit trick counts the differing bits), recording
  static int DescriptorDistance(const cv::Mat& a, const cv::Mat& b) {
    int dist = 0;
    for (int i = 0; i < 32; ++i) dist += __builtin_popcount((unsigned)(a.p[i] ^ b.p[i]));
    ++g_rec->n_dist;
    if (dist < g_rec->min_dist_seen) g_rec->min_dist_seen = dist;
    return dist;
  }
};

#include "loop_search_cut_helpers.inc"
#define IsInImage IsInImageCut
#include "loop_search_cut_isinimage.inc"
#undef IsInImage
#define PredictScale PredictScaleCut
#include "loop_search_cut_predict.inc"
#undef PredictScale
#include "loop_search_cut_point_defs.inc"

}  // namespace PLVS2

using namespace PLVS2;

namespace {
struct KfHolder {
  KeyFrame kf;
  RecordingPinhole cam;
  RecordedPose pose;
};
}  // namespace

extern "C" {

int ref_th_low() { return ORBmatcher::TH_LOW; }

// bounds4: mnMinX, mnMaxX, mnMinY, mnMaxY (integral).  pose: Rcw (9, column-major), s_t = Scw.translation() (3), scale, q_cw (4),
// Ow_points (3)
void* ref_kf_create(int n, const float* x, const float* y, const int32_t* octave, const float* u_right, const uint8_t* desc, const float* bounds4,
                    float grid_w_inv, float grid_h_inv, const float* K4, float mbf, const float* Rcw, const float* s_t, float scale, const float* q,
                    const float* Ow, int n_levels, const float* scale_factors, const float* inv_sigma2, float log_scale_factor) {
  KfHolder* h = new KfHolder;
  KeyFrame& kf = h->kf;
  h->cam.mvParameters.assign(K4, K4 + 4);
  kf.mpCamera = &h->cam;
  kf.fx = K4[0]; kf.fy = K4[1]; kf.cx = K4[2]; kf.cy = K4[3]; kf.mbf = mbf;
  for (int c = 0; c < 3; ++c)
    for (int r = 0; r < 3; ++r) h->pose.R(r, c) = Rcw[3 * c + r];
  h->pose.s_t = Eigen::Vector3f(s_t[0], s_t[1], s_t[2]);
  h->pose.scale = scale;
  h->pose.q = Quat{Eigen::Vector3f(q[0], q[1], q[2]), q[3]};
  h->pose.ow_points = Eigen::Vector3f(Ow[0], Ow[1], Ow[2]);
  kf.N = n;
  kf.mnMinX = (int)bounds4[0]; kf.mnMaxX = (int)bounds4[1]; kf.mnMinY = (int)bounds4[2]; kf.mnMaxY = (int)bounds4[3];
  kf.mfGridElementWidthInv = grid_w_inv; kf.mfGridElementHeightInv = grid_h_inv;
  kf.mfLogScaleFactor = log_scale_factor; kf.mnScaleLevels = n_levels;
  kf.mvScaleFactors.assign(scale_factors, scale_factors + n_levels);
  kf.mvInvLevelSigma2.assign(inv_sigma2, inv_sigma2 + n_levels);
  kf.mvuRight.assign(u_right, u_right + n);
  kf.mvKeysUn.resize(n);
  kf.mDescriptors.p = desc;
  kf.mGrid.assign(kf.mnGridCols, vector<vector<size_t>>(kf.mnGridRows));
  for (int i = 0; i < n; ++i) {
    kf.mvKeysUn[i].pt.x = x[i]; kf.mvKeysUn[i].pt.y = y[i]; kf.mvKeysUn[i].octave = octave[i];
    // RESTATED src/Frame.cc:1305-1316 (PosInGrid) and :717-752 (AssignFeaturesToGrid)
    const int posX = round((x[i] - bounds4[0]) * grid_w_inv), posY = round((y[i] - bounds4[2]) * grid_h_inv);
    if (posX < 0 || posX >= kf.mnGridCols || posY < 0 || posY >= kf.mnGridRows) continue;
    kf.mGrid[posX][posY].push_back(i);
  }
  return h;
}
void ref_kf_destroy(void* h) { delete static_cast<KfHolder*>(h); }

// One call of the reference's SearchByProjection.  overload: 0 = :509-615, 1 = :617-730 (with vpPointsKFs / vpMatchedKF).  skip[i]:
// 0, or 2 = isBad(), 3 = in spAlreadyFound (the point sits in vpMatched on entry, at a slot past the key points' n: the set is built
// from vpMatched and nothing else).  occupied (n bytes or null): vpMatched[j] holds some other map point on entry.
// rec: m x {flags, n_dist, min_dist_seen, level, match}, match = the j with vpMatched[j] == vpPoints[i] after the call (and, overload
// 1, vpMatchedKF[j] == vpPointsKFs[i]: asserted), else -1.  uv: m x 2.  band: m (1 = too near, 2 = too far: RESTATED from :560 for
// the pairs that stopped there).  tcw (3): what the compiled Scw.translation() / Scw.scale() gave.
int ref_search(void* hv, int overload, int m, const float* pos, const float* normal, const float* min_dist, const float* max_dist,
               const uint8_t* desc, const uint8_t* skip, const uint8_t* occupied, int th, float ratio, int32_t* rec, float* uv, int32_t* band,
               float* tcw) {
  KfHolder* h = static_cast<KfHolder*>(hv);
  KeyFramePtr pKF = &h->kf;
  const int n = pKF->N;
  vector<MapPoint> store(m);
  vector<KeyFrame> owners(m);            // vpPointsKFs[i]: a key frame of its own per point, only its address is used
  vector<PairRecord> records(m);
  MapPoint other;                        // what an occupied slot holds on entry
  vector<MapPointPtr> vp(m, nullptr), vpMatched(n, static_cast<MapPointPtr>(nullptr));
  vector<KeyFramePtr> vpKFs(m, nullptr), vpMatchedKF(n, static_cast<KeyFramePtr>(nullptr));
  for (int j = 0; j < n; ++j)
    if (occupied && occupied[j]) vpMatched[j] = &other;
  for (int i = 0; i < m; ++i) {
    MapPoint& p = store[i];
    p.mWorldPos = Eigen::Vector3f(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]);
    p.mNormalVector = Eigen::Vector3f(normal[3 * i], normal[3 * i + 1], normal[3 * i + 2]);
    p.mfMinDistance = min_dist[i]; p.mfMaxDistance = max_dist[i];
    p.mDescriptor.p = desc + 32 * (size_t)i;
    p.skip = skip ? skip[i] : 0;
    p.rec = &records[i];
    vp[i] = &p;
    vpKFs[i] = &owners[i];
  }
  // spAlreadyFound is built from vpMatched itself: a point that is "already found" has to sit in it.  The slots are appended behind
  // the key points' n — no window reaches them (GetFeaturesInArea returns indices below n).
  for (int i = 0; i < m; ++i)
    if (store[i].skip == 3) { vpMatched.push_back(&store[i]); vpMatchedKF.push_back(nullptr); }
  g_pose = &h->pose;
  ORBmatcher matcher;
  Sophus::Sim3f Scw;
  const int found = overload == 0 ? matcher.SearchByProjection(pKF, Scw, vp, vpMatched, th, ratio)
                                  : matcher.SearchByProjection(pKF, Scw, vp, vpKFs, vpMatched, vpMatchedKF, th, ratio);
  const Eigen::Vector3f t = Scw.translation() / Scw.scale();   // the expression of :518, compiled here once more
  for (int c = 0; c < 3; ++c) tcw[c] = t(c);
  vector<int32_t> match(m, -1);
  for (int j = 0; j < n; ++j) {
    MapPointPtr p = vpMatched[j];
    if (!p || p == &other) {
      if (overload == 1 && vpMatchedKF[j]) abort();   // vpMatchedKF is written with vpMatched, never alone
      continue;
    }
    const int i = (int)(p - store.data());
    if (match[i] != -1) abort();                      // a point is matched once
    match[i] = j;
    if (overload == 1 && vpMatchedKF[j] != vpKFs[i]) abort();
    if (overload == 0 && vpMatchedKF[j]) abort();
  }
  for (int i = 0; i < m; ++i) {
    const PairRecord& r = records[i];
    rec[5 * i] = r.flags; rec[5 * i + 1] = r.n_dist; rec[5 * i + 2] = r.min_dist_seen; rec[5 * i + 3] = r.level; rec[5 * i + 4] = match[i];
    uv[2 * i] = r.u; uv[2 * i + 1] = r.v;
    band[i] = 0;
    if ((r.flags & kGotMaxDistance) && !(r.flags & kGotNormal)) {   // RESTATED :557-560
      const Eigen::Vector3f PO = store[i].mWorldPos - h->pose.ow_points;
      const float dist = PO.norm();
      band[i] = dist < 0.8f * min_dist[i] ? 1 : (dist > 1.2f * max_dist[i] ? 2 : 0);
    }
  }
  return found;
}

// the same call without the records read back: for timing
int ref_search_plain(void* h, int overload, int m, const float* pos, const float* normal, const float* min_dist, const float* max_dist,
                     const uint8_t* desc, const uint8_t* skip, int th, float ratio) {
  vector<int32_t> rec(5 * (size_t)m), band(m);
  vector<float> uv(2 * (size_t)m);
  float tcw[3];
  return ref_search(h, overload, m, pos, normal, min_dist, max_dist, desc, skip, nullptr, th, ratio, rec.data(), uv.data(), band.data(), tcw);
}

}  // extern "C"

#elif defined(LOOP_SEARCH_WRAP_LINES)

#include "loop_search_cut_macros.inc"

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

namespace Sophus {
struct Sim3f {   // STAND-IN: the recorded fields (see the head)
  Eigen::Matrix3f R;
  Eigen::Vector3f s_t;
  float s = 1;
  Eigen::Matrix3f rotationMatrix() const { return R; }
  Eigen::Vector3f translation() const { return s_t; }
  float scale() const { return s; }
};
}  // namespace Sophus

namespace PLVS2 {

struct PairRecord {
  int32_t flags = 0, n_proj = 0, n_dist = 0, min_dist_seen = 256, level = -1;
  float proj[6] = {0, 0, 0, 0, 0, 0};
};
enum { kGotEndPoints = 1, kGotMaxDistance = 2, kGotNormal = 4, kPredicted = 8, kGotDescriptor = 16 };
static PairRecord* g_rec = nullptr;   // the pair the call is at: set by isBad

struct Line2DRepresentation {   // the four members of include/Geom2DUtils.h:31-42, zero as its constructor leaves them
  float theta = 0, nx = 0, ny = 0, d = 0;
};
class Geom2DUtils {
 public:
#include "loop_search_cut_geom.inc"
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
  vector<size_t> GetLineFeaturesInArea(const Line2DRepresentation& lineRepresentation, const float& dtheta, const float& dd, const bool bRight = false) const;
  void GetLineFeaturesInArea(const float thetaMin, const float thetaMax, const float dMin, const float dMax, vector<size_t>& vIndices,
                             const bool bRight = false) const;
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
  Eigen::Vector3f mWorldPosStart, mWorldPosEnd, mNormalVector;
  float mfMaxDistance = 0;
  cv::Mat mDescriptor;
  std::mutex mMutexPos;
  int skip = 0;
  PairRecord* rec = nullptr;
};

struct FrameTransformsForLineProjection {   // RESTATED include/LineProjection.h:60-74: the (Rcw, tcw) constructor
  FrameTransformsForLineProjection(const Eigen::Matrix3f& Rcw, const Eigen::Vector3f& tcw) : mRcw(Rcw), mRrw(Rcw), mtcw(tcw), mtrw(tcw) {}
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
  int SearchByProjection(KeyFramePtr& pKF, const Sophus::Sim3f& Scw, const vector<MapLinePtr>& vpLines, vector<MapLinePtr>& vpMatched, int th,
                         float ratioHamming);
  int SearchByProjection(KeyFramePtr& pKF, const Sophus::Sim3f& Scw, const std::vector<MapLinePtr>& vpLines,
                         const std::vector<KeyFramePtr>& vpLinesKFs, std::vector<MapLinePtr>& vpMatched, std::vector<KeyFramePtr>& vpMatchedKF,
                         int th, float ratioHamming);
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
#include "loop_search_cut_accessors.inc"
#undef projectLinear
#undef GetMinDistanceInvariance
#undef GetMaxDistanceInvariance
#undef PredictScale

template <typename FrameType>
#include "loop_search_cut_lineproj.inc"

#include "loop_search_cut_line_defs.inc"

// :1770-1773 alone, the cut statements in a body of their own
static void line_pose(const Sophus::Sim3f& Scw, float* tcw_out, float* ow_out) {
#include "loop_search_cut_line_pose.inc"
  for (int c = 0; c < 3; ++c) { tcw_out[c] = tcw(c); ow_out[c] = Ow(c); }
}

}  // namespace PLVS2

using namespace PLVS2;

namespace {
struct KfHolder {
  KeyFrame kf;
  GeometricCamera cam;
  Sophus::Sim3f Scw;
};
}  // namespace

extern "C" {

int ref_th_low() { return LineMatcher::TH_LOW; }

// segs: n x 4 = startPointX, startPointY, endPointX, endPointY of mvKeyLinesUn; u_right_start / end: NULL = the vectors are empty;
// bounds4: mnMinX, mnMaxX, mnMinY, mnMaxY (integral); max_diag: the Frame's float mnMaxDiag.  Rcw (9, column-major), s_t =
// Scw.translation(), scale.
void* ref_line_kf_create(int n, const float* segs, const int32_t* octave, const float* u_right_start, const float* u_right_end, const uint8_t* desc,
                         const float* bounds4, float max_diag, const float* K4, float mbf, const float* Rcw, const float* s_t, float scale,
                         int n_levels, const float* scale_factors, const float* inv_sigma2, float log_scale_factor) {
  KfHolder* h = new KfHolder;
  KeyFrame& kf = h->kf;
  h->cam.mvLinearParameters.assign(K4, K4 + 4);
  h->cam.mvParameters.assign(K4, K4 + 4);
  kf.mpCamera = &h->cam;
  kf.mbf = mbf;
  for (int c = 0; c < 3; ++c)
    for (int r = 0; r < 3; ++r) h->Scw.R(r, c) = Rcw[3 * c + r];   // Eigen's own layout: column-major
  h->Scw.s_t = Eigen::Vector3f(s_t[0], s_t[1], s_t[2]);
  h->Scw.s = scale;
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
    if (!(posYrow < 0 || posYrow >= LINE_THETA_GRID_ROWS || posXcol < 0 || posXcol >= LINE_D_GRID_COLS)) kf.mLineGrid[posXcol][posYrow].push_back(i);
  }
  return h;
}
void ref_line_kf_destroy(void* h) { delete static_cast<KfHolder*>(h); }

// tcw, Ow (3 each): what the compiled :1770-1773 make of the key frame's Scw
void ref_line_pose(void* h, float* tcw, float* Ow) { line_pose(static_cast<KfHolder*>(h)->Scw, tcw, Ow); }

// One call of the reference's SearchByProjection.  overload: 0 = :1767-1909, 1 = :1913-2037 (with vpLinesKFs / vpMatchedKF).
// skip, occupied: as ref_search of the point side.  rec: m x {flags, n_proj, n_dist, min_dist_seen, level, match}, proj: m x 6,
// stop: m — for the pairs that called GetMaxDistanceInvariance but not GetNormal, RESTATED from include/LineProjection.h:193-251:
// 1 = too near, 2 = too far, 3 = an end point behind, 4 = an end point outside.
int ref_line_search(void* hv, int overload, int m, const float* start, const float* end, const float* normal, const float* max_dist,
                    const uint8_t* desc, const uint8_t* skip, const uint8_t* occupied, int th, float ratio, int32_t* rec, float* proj,
                    int32_t* stop) {
  KfHolder* h = static_cast<KfHolder*>(hv);
  KeyFramePtr pKF = &h->kf;
  const int n = pKF->Nlines;
  vector<MapLine> store(m);
  vector<KeyFrame> owners(m);            // vpLinesKFs[i]: a key frame of its own per line, only its address is used
  vector<PairRecord> records(m);
  MapLine other;                         // what an occupied slot holds on entry
  vector<MapLinePtr> vp(m, nullptr), vpMatched(n, static_cast<MapLinePtr>(nullptr));
  vector<KeyFramePtr> vpKFs(m, nullptr), vpMatchedKF(n, static_cast<KeyFramePtr>(nullptr));
  for (int j = 0; j < n; ++j)
    if (occupied && occupied[j]) vpMatched[j] = &other;
  for (int i = 0; i < m; ++i) {
    MapLine& p = store[i];
    p.mWorldPosStart = Eigen::Vector3f(start[3 * i], start[3 * i + 1], start[3 * i + 2]);
    p.mWorldPosEnd = Eigen::Vector3f(end[3 * i], end[3 * i + 1], end[3 * i + 2]);
    p.mNormalVector = Eigen::Vector3f(normal[3 * i], normal[3 * i + 1], normal[3 * i + 2]);
    p.mfMaxDistance = max_dist[i];
    p.mDescriptor.p = desc + 32 * (size_t)i;
    p.skip = skip ? skip[i] : 0;
    p.rec = &records[i];
    vp[i] = &p;
    vpKFs[i] = &owners[i];
  }
  for (int i = 0; i < m; ++i)   // spAlreadyFound is built from vpMatched: slots appended behind the key lines' n, which no window reaches
    if (store[i].skip == 3) { vpMatched.push_back(&store[i]); vpMatchedKF.push_back(nullptr); }
  LineMatcher matcher;
  const int found = overload == 0 ? matcher.SearchByProjection(pKF, h->Scw, vp, vpMatched, th, ratio)
                                  : matcher.SearchByProjection(pKF, h->Scw, vp, vpKFs, vpMatched, vpMatchedKF, th, ratio);
  float tcw[3], ow[3];
  line_pose(h->Scw, tcw, ow);
  const Eigen::Vector3f t(tcw[0], tcw[1], tcw[2]);
  vector<int32_t> match(m, -1);
  for (int j = 0; j < n; ++j) {
    MapLinePtr p = vpMatched[j];
    if (!p || p == &other) {
      if (vpMatchedKF[j]) abort();   // vpMatchedKF is written with vpMatched, never alone
      continue;
    }
    const int i = (int)(p - store.data());
    if (match[i] != -1) abort();     // a line is matched once
    match[i] = j;
    if (overload == 1 ? vpMatchedKF[j] != vpKFs[i] : vpMatchedKF[j] != nullptr) abort();
  }
  for (int i = 0; i < m; ++i) {
    const PairRecord& r = records[i];
    int32_t* o = rec + 6 * (size_t)i;
    o[0] = r.flags; o[1] = r.n_proj; o[2] = r.n_dist; o[3] = r.min_dist_seen; o[4] = r.level; o[5] = match[i];
    for (int c = 0; c < 6; ++c) proj[6 * (size_t)i + c] = r.proj[c];
    stop[i] = 0;
    if ((r.flags & kGotMaxDistance) && !(r.flags & kGotNormal)) {   // RESTATED include/LineProjection.h:189-251
      const Eigen::Vector3f p3DMw = 0.5 * (store[i].mWorldPosStart + store[i].mWorldPosEnd);
      const Eigen::Vector3f p3DMc = h->Scw.R * p3DMw + t;
      const float distMiddlePoint = p3DMc.norm();
      if (distMiddlePoint < 0.8f * max_dist[i]) stop[i] = 1;
      else if (distMiddlePoint > 1.2f * max_dist[i]) stop[i] = 2;
      else stop[i] = r.n_proj == 1 ? 3 : 4;
    }
  }
  return found;
}

// the same call without the records read back: for timing
int ref_line_search_plain(void* h, int overload, int m, const float* start, const float* end, const float* normal, const float* max_dist,
                          const uint8_t* desc, const uint8_t* skip, int th, float ratio) {
  vector<int32_t> rec(6 * (size_t)m), stop(m);
  vector<float> proj(6 * (size_t)m);
  return ref_line_search(h, overload, m, start, end, normal, max_dist, desc, skip, nullptr, th, ratio, rec.data(), proj.data(), stop.data());
}

}  // extern "C"

#else
#error "compile with -DLOOP_SEARCH_WRAP_POINTS or -DLOOP_SEARCH_WRAP_LINES"
#endif
