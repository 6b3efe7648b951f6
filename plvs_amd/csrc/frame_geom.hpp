// Eigen::Vector3d as the frame's stereo code uses it (frame_rgbd.hip, frame_stereo.hip), in the evaluation order the
// reference's run shows: cross by the plain formula, sums of three as c0 + (c1 + c2) (Eigen's unrolled reduction),
// norm = sqrt, v / s a true division per component.  Built with -ffp-contract=off: nothing fuses.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace plvs {

struct V3 {
  double x, y, z;
};
__device__ __forceinline__ V3 v3(float a, float b, float c) { return V3{(double)a, (double)b, (double)c}; }
__device__ __forceinline__ V3 cross(const V3& a, const V3& b) {
  return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ double sqnorm(const V3& a) { return a.x * a.x + (a.y * a.y + a.z * a.z); }
__device__ __forceinline__ double norm(const V3& a) { return sqrt(sqnorm(a)); }
__device__ __forceinline__ double dot(const V3& a, const V3& b) { return a.x * b.x + (a.y * b.y + a.z * b.z); }
__device__ __forceinline__ V3 divided(const V3& a, double s) { return V3{a.x / s, a.y / s, a.z / s}; }
__device__ __forceinline__ V3 normalized(const V3& a) {   // v / sqrt(squaredNorm) when positive
  const double z2 = sqnorm(a);
  if (!(z2 > 0.0)) return a;
  return divided(a, sqrt(z2));
}

// Frame::kCosViewZAngleMax (src/Frame.cc:103), computed on the host as the reference writes it
inline float cos_view_z_angle_max() { return (float)cos(30. * M_PI / 180.f); }

}  // namespace plvs
