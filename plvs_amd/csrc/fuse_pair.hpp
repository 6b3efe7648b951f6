// One (key frame, map point) pair of ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight = false) (reference src/ORBmatcher.cc:1244-1434)
// up to the choice of bestIdx, in plain C++ that the host and the kernel of orb_fuse.hip share: one text, two compilers.  Nothing
// here names HIP or the library's own headers but track_pose.hpp and track_level.hpp (tests/host/fuse_pair_host.cpp builds it under
// g++ and clang alone).  The units that include this are built without contraction and without fast-math.
//
// The f32 sequence, line by line:
//   :1295  p3Dc = Tcw * p3Dw          Sophus' quaternion action + translation (track_pose.hpp), NOT R p + t
//   :1298  p3Dc(2) < 0.0f             -0.0f and +0.0f pass; they die at :1309
//   :1304  invz = 1 / p3Dc(2)         an f32 division (the int literal is converted)
//   :1306  Pinhole::project           fx * x / z + cx: a true division, not a product with invz
//   :1309  KeyFrame::IsInImage        x >= min && x < max (src/KeyFrame.cc:1404-1407): NaN and +-inf fail, unlike isInFrustum's test
//   :1315  ur = uv(0) - bf * invz
//   :1319  PO = p3Dw - Ow, dist3D = PO.norm() = sqrt(c0 + (c1 + c2))
//   :1323  0.8f * mfMinDistance, 1.2f * mfMaxDistance (src/MapPoint.cc:569-579)
//   :1331  PO.dot(Pn) < 0.5 * dist3D  the dot in f32 as c0 + (c1 + c2), the comparison in f64
//   :1337  PredictScale(dist3D, pKF)  ratio = mfMaxDistance / dist (f32), then track_level.hpp.  dist3D == 0 (ratio = inf, the
//                                     level undefined in the reference) is reported as rejected by the viewing angle
//   :1340  radius = th * mvScaleFactors[level]
//   :1342  KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:1179-1229): Frame's cell arithmetic, no level filter inside
//   :1365-1392  per candidate: the level band, then the chi-square gate — stereo if mvuRight[idx] >= 0 (not > 0) — with the
//               product in f32 and the comparison in f64 against the double literal
//   :1400  dist < bestDist from 256 in the window's enumeration order: the first minimum wins
//
// The Sim3 overload of loop closing and map merging, ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (:1437-1553), is the
// gate policy kGateSim3 of the same text: :1467-1499 is :1294-1337 without ur (the pose is the caller's decomposition of Scw,
// plvs_hip.h: plvs_keyframe_sim3_pose), and a candidate passes the level band alone (:1520) — no chi-square gate.  bestDist starts at
// INT_MAX there (:1513) and is compared <= TH_LOW (:1535): 256 serves, no Hamming distance lies above it.
//
// The loop-closing ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) (:509-615) and its overload with
// vpPointsKFs / vpMatchedKF (:617-730) are the same text again (loop_search_pair.hpp): the gate kGateSim3, the projection policy —
// the first overload calls Pinhole::project (:548, kProjectCamera), the second multiplies by invz (:657-662, kProjectInvz: x * invz is
// rounded before fx multiplies it, so u and v can differ in the last bit) — the exclusion `if(vpMatched[idx]) continue` in front of
// the level band (:587, :701: `claimed`), and bestDist <= TH_LOW * ratioHamming as an integer cut (:606, :720: `cut`).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "track_level.hpp"
#include "track_pose.hpp"

#if defined(__HIPCC__)
#define PLVS_FUSE_FN __host__ __device__ inline
#else
#define PLVS_FUSE_FN inline
#endif

namespace plvs {
namespace fusepair {

using trackpose::V3;

// the `continue` a pair left by (plvs_hip.h: PLVS_FUSE_*)
enum Reached : int {
  kSkipped = 0, kBehind = 1, kOutside = 2, kTooNear = 3, kTooFar = 4, kViewAngle = 5, kEmptyWindow = 6, kNoCandidate = 7,
  kAboveThLow = 8, kCandidate = 9
};
constexpr int kGridCols = 64, kGridRows = 48;   // FRAME_GRID_COLS / ROWS: KeyFrame copies mnGridCols / mnGridRows from them
constexpr int kThLow = 50;                      // ORBmatcher::TH_LOW
enum Gate : int { kGateSE3 = 0, kGateSim3 = 1 };   // which overload's candidate gate (see the head)
enum Projection : int { kProjectCamera = 0, kProjectInvz = 1 };   // plvs_hip.h: PLVS_LOOP_PROJECT_* (see the head)

// what the pair loop reads of pKF besides its grid
struct KfConst {
  float q[4], t[3], Ow[3];                 // GetPose(): quaternion x, y, z, w and translation; GetCameraCenter()
  float fx, fy, cx, cy, mbf;
  float min_x, max_x, min_y, max_y;        // IsInImage
  float grid_min_x, grid_min_y, grid_w_inv, grid_h_inv;
  float log_scale_factor;
  int n_levels;
};

struct Front {
  int reached;        // kBehind .. kViewAngle, or kEmptyWindow: every test passed, the window is next
  int ambiguous;      // predict_level's mark: the host's logarithm decides the level
  int level;
  float u, v, ur, ratio;
};

PLVS_FUSE_FN float dot3(const V3& a, const V3& b) { return a.x * b.x + (a.y * b.y + a.z * b.z); }

// :1294-1337 for one pair
template <Projection kProjection = kProjectCamera>
PLVS_FUSE_FN Front front(const KfConst& K, const float* pos, const float* normal, float min_dist, float max_dist) {
  Front f{kBehind, 0, 0, 0.0f, 0.0f, 0.0f, 0.0f};
  const V3 pw{pos[0], pos[1], pos[2]};
  const V3 pc = trackpose::se3_act(K.q, K.t, pw);
  if (pc.z < 0.0f) return f;
  const float invz = 1.0f / pc.z;
  if (kProjection == kProjectInvz) {
    const float x = pc.x * invz, y = pc.y * invz;
    f.u = K.fx * x + K.cx;
    f.v = K.fy * y + K.cy;
  } else {
    f.u = K.fx * pc.x / pc.z + K.cx;
    f.v = K.fy * pc.y / pc.z + K.cy;
  }
  f.reached = kOutside;
  if (!(f.u >= K.min_x && f.u < K.max_x && f.v >= K.min_y && f.v < K.max_y)) return f;
  f.ur = f.u - K.mbf * invz;
  const float max_distance = 1.2f * max_dist, min_distance = 0.8f * min_dist;
  const V3 PO{pw.x - K.Ow[0], pw.y - K.Ow[1], pw.z - K.Ow[2]};
  const float dist = sqrtf(dot3(PO, PO));
  f.reached = kTooNear;
  if (dist < min_distance) return f;
  f.reached = kTooFar;
  if (dist > max_distance) return f;
  f.reached = kViewAngle;
  if ((double)dot3(PO, V3{normal[0], normal[1], normal[2]}) < 0.5 * (double)dist) return f;
  if (dist == 0.0f) return f;
  f.ratio = max_dist / dist;
  const LevelChoice lc = predict_level(f.ratio, K.log_scale_factor, K.n_levels);
  f.level = lc.level;
  f.ambiguous = lc.ambiguous;
  f.reached = kEmptyWindow;
  return f;
}

// the cell range of GetFeaturesInArea; false: one of its early returns
struct Cells { int c0, c1, r0, r1; };
PLVS_FUSE_FN bool window_cells(const KfConst& K, float x, float y, float r, Cells* w) {
  const int c0 = (int)floorf((x - K.grid_min_x - r) * K.grid_w_inv);
  w->c0 = c0 < 0 ? 0 : c0;
  if (w->c0 >= kGridCols) return false;
  const int c1 = (int)ceilf((x - K.grid_min_x + r) * K.grid_w_inv);
  w->c1 = c1 > kGridCols - 1 ? kGridCols - 1 : c1;
  if (w->c1 < 0) return false;
  const int r0 = (int)floorf((y - K.grid_min_y - r) * K.grid_h_inv);
  w->r0 = r0 < 0 ? 0 : r0;
  if (w->r0 >= kGridRows) return false;
  const int r1 = (int)ceilf((y - K.grid_min_y + r) * K.grid_h_inv);
  w->r1 = r1 > kGridRows - 1 ? kGridRows - 1 : r1;
  if (w->r1 < 0) return false;
  return true;
}

// :1222 — the member is in vIndices
PLVS_FUSE_FN bool in_area(float kx, float ky, float x, float y, float r) {
  const float distx = kx - x, disty = ky - y;
  return fabsf(distx) < r && fabsf(disty) < r;
}

// :1365-1392 (kGateSim3: :1520 alone) — true: the candidate's Hamming distance is taken
template <Gate kGate = kGateSE3>
PLVS_FUSE_FN bool candidate_gate(float u, float v, float ur, int level, float kx, float ky, int octave, float kr, const float* inv_level_sigma2) {
  if (octave < level - 1 || octave > level) return false;
  if (kGate == kGateSim3) return true;
  const float ex = u - kx, ey = v - ky;
  if (kr >= 0) {
    const float er = ur - kr;
    const float e2 = ex * ex + ey * ey + er * er;
    if ((double)(e2 * inv_level_sigma2[octave]) > 7.8) return false;
  } else {
    const float e2 = ex * ex + ey * ey;
    if ((double)(e2 * inv_level_sigma2[octave]) > 5.99) return false;
  }
  return true;
}

PLVS_FUSE_FN int hamming256(const uint32_t* a, const uint32_t* b) {
  int d = 0;
  for (int i = 0; i < 8; ++i) {
    uint32_t v = a[i] ^ b[i];   // ORBmatcher::DescriptorDistance's bit trick counts the same bits
    v = v - ((v >> 1) & 0x55555555u);
    v = (v & 0x33333333u) + ((v >> 2) & 0x33333333u);
    d += (int)((((v + (v >> 4)) & 0x0F0F0F0Fu) * 0x01010101u) >> 24);
  }
  return d;
}

// The grid as the window walk reads it: CSR cell starts (column-major cells, ix * kGridRows + iy) over members in the reference's
// enumeration order.  Member: anything with x, y, octave, idx.
template <typename Member>
struct KfGrid {
  const int* start;
  const Member* members;
  const float* u_right;
  const uint8_t* desc;               // N x 32, 4-byte aligned
  const float* scale_factors;
  const float* inv_level_sigma2;
};

struct Result { int best_idx, best_dist, reached; };

// :1340-1408 for a pair whose tests passed, serially, with the level given (the host's).  claimed (may be null): the members a
// greedy overload's earlier pairs took (vpMatched[idx] != null), left out behind the gate; cut: the largest distance that is taken
template <Gate kGate = kGateSE3, typename Member>
inline Result search_window(const KfConst& K, const KfGrid<Member>& G, const Front& f, int level, float th, const uint8_t* point_desc,
                            const uint8_t* claimed = nullptr, int cut = kThLow) {
  Result res{-1, -1, kEmptyWindow};
  const float radius = th * G.scale_factors[level];
  Cells w;
  if (!window_cells(K, f.u, f.v, radius, &w)) return res;
  uint32_t qd[8];
  std::memcpy(qd, point_desc, 32);
  int best = 256, best_idx = -1;
  bool any = false, gated = false;
  for (int ix = w.c0; ix <= w.c1; ++ix) {
    const Member* m = G.members + G.start[ix * kGridRows + w.r0];
    const Member* const end = G.members + G.start[ix * kGridRows + w.r1 + 1];
    for (; m < end; ++m) {
      if (!in_area(m->x, m->y, f.u, f.v, radius)) continue;
      any = true;
      if (!candidate_gate<kGate>(f.u, f.v, f.ur, level, m->x, m->y, m->octave, G.u_right[m->idx], G.inv_level_sigma2)) continue;
      gated = true;
      if (claimed && claimed[m->idx]) continue;
      uint32_t td[8];
      std::memcpy(td, G.desc + 32 * (size_t)m->idx, 32);
      const int d = hamming256(qd, td);
      if (d < best) { best = d; best_idx = m->idx; }
    }
  }
  if (!any) return res;
  res.reached = !gated ? kNoCandidate : (best <= cut ? kCandidate : kAboveThLow);
  if (res.reached == kCandidate) { res.best_idx = best_idx; res.best_dist = best; }
  return res;
}

// the whole pair on the host: the level is the reference's own expression on the host's libm
template <Gate kGate = kGateSE3, typename Member>
inline Result pair_host(const KfConst& K, const KfGrid<Member>& G, const float* pos, const float* normal, float min_dist, float max_dist,
                        const uint8_t* point_desc, float th, int double_overload) {
  const Front f = front(K, pos, normal, min_dist, max_dist);
  if (f.reached != kEmptyWindow) return Result{-1, -1, f.reached};
  return search_window<kGate>(K, G, f, predict_level_host(f.ratio, K.log_scale_factor, K.n_levels, double_overload), th, point_desc);
}

}  // namespace fusepair
}  // namespace plvs
