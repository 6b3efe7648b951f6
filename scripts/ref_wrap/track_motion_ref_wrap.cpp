// The reference's own LineProjection::ProjectLineWithCheck, Pinhole::project(const Eigen::Vector3f&),
// GeometricCamera::projectLinear(const Eigen::Vector3f&), MapLine::Get{Min,Max}DistanceInvariance and the three statements of
// Sophus' point action (Thirdparty/Sophus/sophus/so3.hpp:364-366), behind a C interface.  This file holds declarations and calls
// only: the DEFINITIONS are cut verbatim out of the reference tree into track_motion_cut_*.inc at build time
// (scripts/make_track_motion_golden.py) and compiled here, against oracle/ref/eigen_full, with -O2 -ffp-contract=off
// -fno-fast-math.  The classes below carry exactly the members those definitions touch.
//
// RESTATED, not compiled (real Sophus and Eigen's own cross / Quaternion cannot be compiled here: no Eigen is installed, and
// the stand-in's Quaternion is a bare struct) — each marked where it stands:
//   * the coefficient formula of the 3-vector cross product (Eigen/src/Geometry/OrthoMethods.h, cross3_impl: a1 b2 - a2 b1,
//     a2 b0 - a0 b2, a0 b1 - a1 b0) is the stand-in's Matrix<T, 3, 1>::cross (oracle/ref/eigen_full/Eigen/Core);
//   * the `+ translation()` of Thirdparty/Sophus/sophus/se3.hpp:323;
//   * the expression around the cut in src/ORBmatcher.cc: `1.0/x3Dc(2)` (:1810), `if(invzc<0)` (:1812) and the four
//     comparisons of :1817-1820; and bForward / bBackward of :1794-1795.
#include <cmath>
#include <cstdint>
#include <memory>
#include <mutex>
#include <vector>

#include <Eigen/Core>

using namespace std;

namespace PLVS2 {

class GeometricCamera {
 public:
  enum { CAM_PINHOLE = 0, CAM_FISHEYE = 1 };
  virtual ~GeometricCamera() {}
  virtual Eigen::Vector2f project(const Eigen::Vector3f& v3D) const = 0;
  Eigen::Vector2f projectLinear(const Eigen::Vector3f& v3D) const;
  unsigned int GetType() const { return mnType; }
  std::vector<float> mvParameters, mvLinearParameters;
  unsigned int mnType = CAM_PINHOLE;
};

class Pinhole : public GeometricCamera {
 public:
  Eigen::Vector2f project(const Eigen::Vector3f& v3D) const;
};

class MapLine {
 public:
  void GetWorldEndPoints(Eigen::Vector3f& s, Eigen::Vector3f& e) { s = mWorldPosStart; e = mWorldPosEnd; }
  float GetMinDistanceInvariance();
  float GetMaxDistanceInvariance();
  Eigen::Vector3f mWorldPosStart, mWorldPosEnd;
  float mfMinDistance = 0, mfMaxDistance = 0;
  std::mutex mMutexPos;
};
typedef MapLine* MapLinePtr;

class Frame {
 public:
  GeometricCamera* mpCamera = nullptr;
  GeometricCamera* mpCamera2 = nullptr;
  float mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0;
};

struct FrameTransformsForLineProjection {
  Eigen::Matrix3f mRcw, mRrw;
  Eigen::Vector3f mtcw, mtrw;
};

class LineProjection {
 public:
  template <typename FrameType>
  bool ProjectLineWithCheck(const MapLinePtr& pML, const FrameType& F, const FrameTransformsForLineProjection& frameTfs, bool bRight = false);
  // -1 / 0 before a store is THIS PROJECT'S convention for what a line rejected early reports (include/plvs_hip.h,
  // plvs_motion_lines), not the reference's: its constructor zeroes these members (include/LineProjection.h:83-87).  The
  // reference never reads a rejected line's fields, so the difference decides nothing.
  float uS = -1, vS = -1, uE = -1, vE = -1, uM = -1, vM = -1, invSz = 0, invEz = 0;
  float distMiddlePoint = 0;
  Eigen::Vector3f p3DMw;
};

template <typename FrameType>
#include "track_motion_cut_lineproj.inc"

#include "track_motion_cut_defs.inc"

}  // namespace PLVS2

namespace {

// the unit quaternion as Sophus::SO3f hands it to the three statements: vec() and w()
struct Quat {
  Eigen::Vector3f v;
  float s;
  const Eigen::Vector3f& vec() const { return v; }
  float w() const { return s; }
};
template <class PointDerived>
using PointProduct = Eigen::Vector3f;

// Sophus::SO3f::operator*(point), so3.hpp:358-367: the body is the cut
template <class PointDerived>
PointProduct<PointDerived> so3_times(const Quat& q, const PointDerived& p) {
#include "track_motion_cut_so3.inc"
}
// Sophus::SE3f::operator*(point) — RESTATED from se3.hpp:323: `return so3() * p + translation();`
Eigen::Vector3f se3_times(const Quat& q, const Eigen::Vector3f& t, const Eigen::Vector3f& p) { return so3_times(q, p) + t; }

Quat quat_of(const float* q) { return Quat{Eigen::Vector3f(q[0], q[1], q[2]), q[3]}; }

}  // namespace

extern "C" {

// The projection of ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono), src/ORBmatcher.cc:1797-1820.  Outputs
// in the layout of plvs_motion_points (include/plvs_hip.h); pc = x3Dc, 3 per point.
void ref_project_points(const float* q_cw, const float* tcw, const float* K4, const float* bounds4, int n, const uint8_t* valid,
                        const float* pos, float* pc, uint8_t* proj_valid, float* u, float* v, float* invz) {
  PLVS2::Pinhole cam;
  cam.mvParameters.assign(K4, K4 + 4);
  const Quat q = quat_of(q_cw);
  const Eigen::Vector3f t(tcw[0], tcw[1], tcw[2]);
  const float mnMinX = bounds4[0], mnMaxX = bounds4[1], mnMinY = bounds4[2], mnMaxY = bounds4[3];
  for (int i = 0; i < n; ++i) {
    proj_valid[i] = 0; u[i] = -1; v[i] = -1; invz[i] = 0;
    pc[3 * i] = pc[3 * i + 1] = pc[3 * i + 2] = 0;
    if (!valid[i]) continue;
    const Eigen::Vector3f x3Dw(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]);
    const Eigen::Vector3f x3Dc = se3_times(q, t, x3Dw);
    for (int j = 0; j < 3; ++j) pc[3 * i + j] = x3Dc(j);
    const float invzc = 1.0 / x3Dc(2);   // RESTATED :1810
    invz[i] = invzc;
    if (invzc < 0) continue;             // RESTATED :1812
    const Eigen::Vector2f uv = cam.project(x3Dc);
    u[i] = uv(0); v[i] = uv(1);
    if (uv(0) < mnMinX || uv(0) > mnMaxX) continue;   // RESTATED :1817-1820
    if (uv(1) < mnMinY || uv(1) > mnMaxY) continue;
    proj_valid[i] = 1;
  }
}

// bForward / bBackward — RESTATED from src/ORBmatcher.cc:1788-1795 (twc = Tcw.inverse().translation() is the frame's mOw)
void ref_direction(const float* q_lw, const float* tlw, const float* Ow, float mb, int mono, int* forward, int* backward) {
  const bool bMono = mono != 0;
  const Eigen::Vector3f tlc = se3_times(quat_of(q_lw), Eigen::Vector3f(tlw[0], tlw[1], tlw[2]), Eigen::Vector3f(Ow[0], Ow[1], Ow[2]));
  *forward = tlc(2) > mb && !bMono;
  *backward = -tlc(2) > mb && !bMono;
}

// LineProjection::ProjectLineWithCheck over the last frame's lines (src/LineMatcher.cc:872-902).  A fresh LineProjection per
// line, so that a rejected line reports this project's -1 / 0 and not the line before it: the reference re-uses one object
// (src/LineMatcher.cc:862) and never reads it after a `false`.
void ref_project_lines(const float* Rcw, const float* tcw, const float* K4_linear, const float* bounds4, int n, const uint8_t* valid,
                       const float* start, const float* end, const float* max_dist, uint8_t* proj_valid, float* proj6, float* dist) {
  PLVS2::Pinhole cam;
  cam.mvParameters.assign(K4_linear, K4_linear + 4);
  cam.mvLinearParameters.assign(K4_linear, K4_linear + 4);
  PLVS2::Frame F;
  F.mpCamera = &cam;
  F.mnMinX = bounds4[0]; F.mnMaxX = bounds4[1]; F.mnMinY = bounds4[2]; F.mnMaxY = bounds4[3];
  PLVS2::FrameTransformsForLineProjection tf;
  for (int i = 0; i < 9; ++i) tf.mRcw(i) = Rcw[i];   // the layout Eigen::Matrix3f has in memory
  for (int i = 0; i < 3; ++i) tf.mtcw(i) = tcw[i];
  for (int i = 0; i < n; ++i) {
    PLVS2::LineProjection proj;
    proj_valid[i] = 0;
    dist[i] = 0;
    if (valid[i]) {
      PLVS2::MapLine ml;
      ml.mWorldPosStart = Eigen::Vector3f(start[3 * i], start[3 * i + 1], start[3 * i + 2]);
      ml.mWorldPosEnd = Eigen::Vector3f(end[3 * i], end[3 * i + 1], end[3 * i + 2]);
      ml.mfMaxDistance = max_dist[i];
      PLVS2::MapLinePtr p = &ml;
      proj_valid[i] = proj.ProjectLineWithCheck(p, F, tf) ? 1 : 0;
      dist[i] = proj.distMiddlePoint;
    }
    float* o = proj6 + 6 * i;
    o[0] = proj.uS; o[1] = proj.vS; o[2] = proj.uE; o[3] = proj.vE; o[4] = proj.invSz; o[5] = proj.invEz;
  }
}

}  // extern "C"
