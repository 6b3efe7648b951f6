// The reference's own ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight) (src/ORBmatcher.cc:1244-1434), KeyFrame::GetFeaturesInArea
// (src/KeyFrame.cc:1179-1229), KeyFrame::IsInImage (:1404-1407), MapPoint::PredictScale(const float&, KeyFramePtr&)
// (src/MapPoint.cc:581-596), Pinhole::project(const Eigen::Vector3f&) and the three statements of Sophus' point action
// (Thirdparty/Sophus/sophus/so3.hpp:364-366), behind a C interface.  This file holds declarations, recording accessors and calls:
// the DEFINITIONS are cut verbatim out of the reference tree into orb_fuse_cut_*.inc at build time
// (scripts/make_orb_fuse_golden.py) and compiled here, against oracle/ref/eigen_full, with -O2 -ffp-contract=off -fno-fast-math.
// The classes below carry exactly the members those definitions touch.
//
// What Fuse does per pair is RECORDED by the accessors it calls, not inferred: GetWorldPos (the pair was not skipped),
// project (the depth test passed), GetMaxDistanceInvariance (IsInImage passed), GetNormal (the band passed), GetDescriptor (the
// window was not empty), DescriptorDistance (a candidate passed the level band and its gate; count and minimum), GetMapPoint /
// AddObservation / AddMapPoint (bestDist <= TH_LOW, with bestIdx).  GetMapPoint returns null, so the run mutates nothing that a
// later pair reads: what is recorded is the search.
//
// RESTATED, not compiled — each marked where it stands:
//   * the cross product's coefficient formula is the stand-in's Matrix<T, 3, 1>::cross (oracle/ref/eigen_full/Eigen/Core);
//   * the `+ translation()` of Thirdparty/Sophus/sophus/se3.hpp:323;
//   * MapPoint::GetMinDistanceInvariance / GetMaxDistanceInvariance (src/MapPoint.cc:569-579), as recording accessors;
//   * ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:2198-2217), as a recording accessor;
//   * Frame::AssignFeaturesToGrid / PosInGrid (src/Frame.cc:717-752, :1305-1316), whose mGrid the key frame copies
//     (src/KeyFrame.cc, constructor);
//   * which side of the band rejected a pair (ref_fuse: too near / too far), from the two comparisons of src/ORBmatcher.cc:1323.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include <Eigen/Core>

using namespace std;

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
#include "orb_fuse_cut_so3.inc"
}
}  // namespace

namespace Sophus {
struct SE3f {
  Quat q;
  Eigen::Vector3f t;
  Eigen::Vector3f operator*(const Eigen::Vector3f& p) const { return so3_times(q, p) + t; }   // RESTATED se3.hpp:323
};
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
  int32_t flags = 0, n_dist = 0, min_dist_seen = 256, best_idx = -1;
  float u = 0, v = 0;
};
enum { kGotWorldPos = 1, kProjected = 2, kGotMaxDistance = 4, kGotNormal = 8, kGotDescriptor = 16, kGotMapPoint = 32, kAddObservation = 64,
       kAddMapPoint = 128, kReplace = 256 };
static PairRecord* g_rec = nullptr;   // the pair Fuse is at: set by GetWorldPos' owner (the loop below sets it through isBad)

class RecordingPinhole : public Pinhole {
 public:
  Eigen::Vector2f project(const Eigen::Vector3f& v3D) const {
    const Eigen::Vector2f uv = Pinhole::project(v3D);
    g_rec->flags |= kProjected;
    g_rec->u = uv(0); g_rec->v = uv(1);
    return uv;
  }
};

class KeyFrame;
class MapPoint;
typedef KeyFrame* KeyFramePtr;
typedef MapPoint* MapPointPtr;

class KeyFrame {
 public:
  Sophus::SE3f GetPose() { return mTcw; }
  Sophus::SE3f GetRightPose() { return mTcw; }
  Eigen::Vector3f GetCameraCenter() { return mOw; }
  Eigen::Vector3f GetRightCameraCenter() { return mOw; }
  bool IsInImage(const float& x, const float& y) const;
  vector<size_t> GetFeaturesInArea(const float& x, const float& y, const float& r, const bool bRight = false) const;
  MapPointPtr GetMapPoint(const size_t& idx) { g_rec->flags |= kGotMapPoint; g_rec->best_idx = (int32_t)idx; return nullptr; }
  void AddMapPoint(MapPointPtr, const size_t& idx) { g_rec->flags |= kAddMapPoint; }
  Sophus::SE3f mTcw;
  Eigen::Vector3f mOw;
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
  bool IsInKeyFrame(KeyFramePtr) { return skip == 3; }
  Eigen::Vector3f GetWorldPos() { rec->flags |= kGotWorldPos; return mWorldPos; }
  Eigen::Vector3f GetNormal() { rec->flags |= kGotNormal; return mNormalVector; }
  float GetMinDistanceInvariance() { return 0.8f * mfMinDistance; }                                   // RESTATED src/MapPoint.cc:572
  float GetMaxDistanceInvariance() { rec->flags |= kGotMaxDistance; return 1.2f * mfMaxDistance; }    // RESTATED src/MapPoint.cc:578
  int PredictScale(const float& currentDist, KeyFramePtr& pKF);
  cv::Mat GetDescriptor() { rec->flags |= kGotDescriptor; return mDescriptor; }
  int Observations() { return 1; }
  void Replace(MapPointPtr) { rec->flags |= kReplace; }
  void AddObservation(KeyFramePtr, size_t idx) { rec->flags |= kAddObservation; rec->best_idx = (int32_t)idx; }
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
  int Fuse(KeyFramePtr& pKF, const vector<MapPointPtr>& vpMapPoints, const float th = 3.0, const bool bRight = false);
  // RESTATED src/ORBmatcher.cc:2198-2217 (the bit trick counts the differing bits), recording
  static int DescriptorDistance(const cv::Mat& a, const cv::Mat& b) {
    int dist = 0;
    for (int i = 0; i < 32; ++i) dist += __builtin_popcount((unsigned)(a.p[i] ^ b.p[i]));
    ++g_rec->n_dist;
    if (dist < g_rec->min_dist_seen) g_rec->min_dist_seen = dist;
    return dist;
  }
};

#include "orb_fuse_cut_defs.inc"

}  // namespace PLVS2

using namespace PLVS2;

namespace {
struct KfHolder {
  KeyFrame kf;
  RecordingPinhole cam;
};
}  // namespace

extern "C" {

// bounds4: mnMinX, mnMaxX, mnMinY, mnMaxY (integral values: the key frame holds them as int)
void* ref_kf_create(int n, const float* x, const float* y, const int32_t* octave, const float* u_right, const uint8_t* desc, const float* bounds4,
                    float grid_w_inv, float grid_h_inv, const float* K4, float mbf, const float* q, const float* t, const float* Ow, int n_levels,
                    const float* scale_factors, const float* inv_sigma2, float log_scale_factor) {
  KfHolder* h = new KfHolder;
  KeyFrame& kf = h->kf;
  h->cam.mvParameters.assign(K4, K4 + 4);
  kf.mpCamera = &h->cam;
  kf.fx = K4[0]; kf.fy = K4[1]; kf.cx = K4[2]; kf.cy = K4[3]; kf.mbf = mbf;
  kf.mTcw.q = Quat{Eigen::Vector3f(q[0], q[1], q[2]), q[3]};
  kf.mTcw.t = Eigen::Vector3f(t[0], t[1], t[2]);
  kf.mOw = Eigen::Vector3f(Ow[0], Ow[1], Ow[2]);
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

// One call of the reference's Fuse.  skip[i]: 0, or 1 = null pointer, 2 = isBad(), 3 = IsInKeyFrame(pKF).  rec: m x {flags, n_dist,
// min_dist_seen, best_idx}, uv: m x 2, band: m (1 = too near, 2 = too far: RESTATED from :1323 for the pairs that stopped there).
int ref_fuse(void* h, int m, const float* pos, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* desc,
             const uint8_t* skip, float th, int32_t* rec, float* uv, int32_t* band) {
  KeyFramePtr pKF = &static_cast<KfHolder*>(h)->kf;
  vector<MapPoint> store(m);
  vector<PairRecord> records(m);
  vector<MapPointPtr> vp(m, nullptr);
  for (int i = 0; i < m; ++i) {
    MapPoint& p = store[i];
    p.mWorldPos = Eigen::Vector3f(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]);
    p.mNormalVector = Eigen::Vector3f(normal[3 * i], normal[3 * i + 1], normal[3 * i + 2]);
    p.mfMinDistance = min_dist[i]; p.mfMaxDistance = max_dist[i];
    p.mDescriptor.p = desc + 32 * (size_t)i;
    p.skip = skip ? skip[i] : 0;
    p.rec = &records[i];
    if (p.skip != 1) vp[i] = &p;
  }
  ORBmatcher matcher;
  const int fused = matcher.Fuse(pKF, vp, th, false);
  for (int i = 0; i < m; ++i) {
    const PairRecord& r = records[i];
    rec[4 * i] = r.flags; rec[4 * i + 1] = r.n_dist; rec[4 * i + 2] = r.min_dist_seen; rec[4 * i + 3] = r.best_idx;
    uv[2 * i] = r.u; uv[2 * i + 1] = r.v;
    band[i] = 0;
    if ((r.flags & kGotMaxDistance) && !(r.flags & kGotNormal)) {   // RESTATED :1319-1323
      const Eigen::Vector3f PO = store[i].mWorldPos - pKF->mOw;
      const float dist3D = PO.norm();
      band[i] = dist3D < 0.8f * min_dist[i] ? 1 : (dist3D > 1.2f * max_dist[i] ? 2 : 0);
    }
  }
  return fused;
}

// the same call without the records read back: for timing
int ref_fuse_plain(void* h, int m, const float* pos, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* desc,
                   const uint8_t* skip, float th) {
  vector<int32_t> rec(4 * (size_t)m), band(m);
  vector<float> uv(2 * (size_t)m);
  return ref_fuse(h, m, pos, normal, min_dist, max_dist, desc, skip, th, rec.data(), uv.data(), band.data());
}

int ref_predict_scale(float dist, float max_dist, float log_scale_factor, int levels) {
  KeyFrame kf;
  kf.mfLogScaleFactor = log_scale_factor; kf.mnScaleLevels = levels;
  KeyFramePtr p = &kf;
  MapPoint mp;
  mp.mfMaxDistance = max_dist;
  return mp.PredictScale(dist, p);
}

}  // extern "C"
