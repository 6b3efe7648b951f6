// What the line kernels over resident key frames read of a call: the query (FuseLines) and, per listed key frame, the call's pose
// inside the handle's constants with pointers into the handle's allocation (KfRes).  One text for line_fuse.hip (the Fuse searches)
// and line_loop_search.hip (the loop-closing SearchByProjection).  Internal to the library.
#pragma once
#include "common.hpp"
#include "keyframe_handle.hpp"
#include "line_fuse_pair.hpp"

namespace plvs {
namespace linefusetab {

using plvs::linefuse::KfConst;
using plvs::linefuse::Member;

constexpr int kPosBits = 23;   // a lane's key: distance (9 bits) above the enumeration position

struct FuseLines {
  const float *start, *end, *normal, *max_dist;
  const uint4* desc;
  const uint8_t* skip;   // n_kfs x m, or null
  int m, n_pairs;
};

// where the walk finds one key frame's arrays: resolved from the staged block's offsets (KfDev) or the handle's pointers (KfRes)
struct KfArrays {
  const Member* members;
  const int* start;
  const uint4* desc;
  const float *sf, *sig;
  int n_members;
};

// one key frame of a resident call's table: the call's pose inside the handle's constants, and pointers into the handle's allocation
struct KfRes {
  KfConst k;
  KfArrays a;
};
static_assert(sizeof(KfRes) == 168, "the per-call table entry: stats[3] of the resident entries is documented and tested from it");

inline KfArrays arrays_at(const char* block, const plvs_keyframe::Lines& s) {
  return KfArrays{reinterpret_cast<const Member*>(block + s.o_mem), reinterpret_cast<const int*>(block + s.o_start),
                  reinterpret_cast<const uint4*>(block + s.o_desc), reinterpret_cast<const float*>(block + s.o_sf),
                  reinterpret_cast<const float*>(block + s.o_sig), s.n_members};
}

// the handle's constants with the Sim3 call's pose (plvs_keyframe_sim3_pose: the line overloads' Ow)
inline KfConst sim3_const(const plvs_keyframe& kf, const plvs_keyframe_sim3_pose& pose) {
  KfConst c = kf.ln.c;
  for (int i = 0; i < 9; ++i) c.R[i] = pose.Rcw[i];
  for (int i = 0; i < 3; ++i) { c.t[i] = pose.tcw[i]; c.Ow[i] = pose.Ow_lines[i]; }
  return c;
}

}  // namespace linefusetab
}  // namespace plvs
