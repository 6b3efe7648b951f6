// What the kernels over resident key frames read of a call: the query (FusePoints) and, per listed key frame, the call's pose
// inside the handle's constants with pointers into the handle's allocation (KfRes).  One text for orb_fuse.hip (the Fuse searches)
// and orb_loop_search.hip (the loop-closing SearchByProjection).  Internal to the library.
#pragma once
#include "common.hpp"
#include "fuse_pair.hpp"
#include "keyframe_handle.hpp"
#include "orb_window.hpp"

namespace plvs {
namespace orbfuse {

using plvs::fusepair::KfConst;
using plvs::orbwin::FrameGrid;

constexpr int kPosBits = 23;   // a lane's key: distance (9 bits) above the enumeration position

struct FusePoints {
  const float *pos, *normal, *min_dist, *max_dist;
  const uint4* desc;
  const uint8_t* skip;   // n_kfs x m, or null
  int m, n_pairs;
};

// where the walk finds one key frame's arrays: resolved from the staged block's offsets (KfDev) or the handle's pointers (KfRes)
struct KfArrays {
  const FrameGrid::Member* members;
  const int* start;
  const float* u_right;
  const uint4* desc;
  const float *sf, *sig;
  int n;
};

// one key frame of a resident call's table: the call's pose inside the handle's constants, and pointers into the handle's allocation
struct KfRes {
  KfConst k;
  KfArrays a;
};
static_assert(sizeof(KfRes) == 160, "the per-call table entry: stats[3] of the resident entries is documented and tested from it");

inline KfArrays arrays_at(const char* block, const plvs_keyframe::Points& s) {
  return KfArrays{reinterpret_cast<const FrameGrid::Member*>(block + s.o_mem), reinterpret_cast<const int*>(block + s.o_start),
                  reinterpret_cast<const float*>(block + s.o_ur), reinterpret_cast<const uint4*>(block + s.o_desc),
                  reinterpret_cast<const float*>(block + s.o_sf), reinterpret_cast<const float*>(block + s.o_sig), s.n};
}

// the handle's constants with the Sim3 call's pose (plvs_keyframe_sim3_pose: the point overloads' Ow)
inline KfConst sim3_const(const plvs_keyframe& kf, const plvs_keyframe_sim3_pose& pose) {
  KfConst c = kf.pt.c;
  for (int i = 0; i < 4; ++i) c.q[i] = pose.q_cw[i];
  for (int i = 0; i < 3; ++i) { c.t[i] = pose.tcw[i]; c.Ow[i] = pose.Ow_points[i]; }
  return c;
}

}  // namespace orbfuse
}  // namespace plvs
