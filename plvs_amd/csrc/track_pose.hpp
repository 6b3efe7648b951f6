// The pose arithmetic of the motion-model link (frame_motion.hip), in plain C++ that the host and the projection kernel share:
// one text, two compilers.
//
// Tcw * x3Dw of ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (src/ORBmatcher.cc:1806) is Sophus' action
// of a unit quaternion on a point (Thirdparty/Sophus/sophus/so3.hpp:363-366) followed by the translation (se3.hpp:323):
//     uv = q.vec().cross(p);  uv += uv;  return p + q.w() * uv + q.vec().cross(uv);          ... + translation()
// Both cross products are temporaries (MatrixBase::cross returns a plain vector), so the sum is evaluated per coefficient, left
// to right: (p[i] + w * uv[i]) + c[i], then + t[i].  The 3-vector cross product is Eigen's coefficient formula
// (Eigen/src/Geometry/OrthoMethods.h): a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0.  This is NOT the float sequence of R p + t.
// The units that include this are built without contraction and without fast-math.
//
// bForward / bBackward (:1788-1795, src/LineMatcher.cc:851-860): twc = Tcw.inverse().translation() is the frame's mOw by the same
// expression (Frame::UpdatePoseMatrices), tlc = Tlw * twc is the same action with the last frame's pose.
#pragma once

#if defined(__HIPCC__)
#define PLVS_POSE_FN __host__ __device__ inline
#else
#define PLVS_POSE_FN inline
#endif

namespace plvs {
namespace trackpose {

struct V3 { float x, y, z; };

PLVS_POSE_FN V3 cross(const V3& a, const V3& b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// q: x, y, z, w (the order of Eigen::Quaternionf::coeffs())
PLVS_POSE_FN V3 so3_act(const float* q, const V3& p) {
  const V3 v{q[0], q[1], q[2]};
  V3 uv = cross(v, p);
  uv.x += uv.x; uv.y += uv.y; uv.z += uv.z;
  const V3 c = cross(v, uv);
  return V3{(p.x + q[3] * uv.x) + c.x, (p.y + q[3] * uv.y) + c.y, (p.z + q[3] * uv.z) + c.z};
}

PLVS_POSE_FN V3 se3_act(const float* q, const float* t, const V3& p) {
  const V3 r = so3_act(q, p);
  return V3{r.x + t[0], r.y + t[1], r.z + t[2]};
}

// bForward = tlc(2) > mb && !bMono, bBackward = -tlc(2) > mb && !bMono
inline void direction(const float* q_lw, const float* tlw, const float* Ow, float mb, int mono, int* forward, int* backward) {
  const V3 tlc = se3_act(q_lw, tlw, V3{Ow[0], Ow[1], Ow[2]});
  *forward = (tlc.z > mb && !mono) ? 1 : 0;
  *backward = (-tlc.z > mb && !mono) ? 1 : 0;
}

}  // namespace trackpose
}  // namespace plvs
