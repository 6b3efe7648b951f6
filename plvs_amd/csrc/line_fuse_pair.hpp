// One (key frame, map line) pair of LineMatcher::Fuse(pKF, vpMapLines, th, bRight = false) (reference src/LineMatcher.cc:2043-2276)
// up to the choice of bestIdx, in plain C++ that the host and the kernel of line_fuse.hip share: one text, two compilers.  Nothing
// here names HIP or the library's own headers but track_level.hpp (tests/host/line_fuse_pair_host.cpp builds it under g++ and
// clang alone).  The units that include this are built without contraction and without fast-math.
//
// The f32 sequence, line by line:
//   LineProjection::ProjectLineWithCheck (include/LineProjection.h:144-264), pinhole, bRight == false
//     :155   p3DMw = 0.5 * (S + E)      the scalar is converted to f32: a sum and a halving per component
//     :158   p3DMc = R * p3DMw + t      mRcw column-major, the product first (a temporary), then the sum
//     :162   p3DMcZ < 0.0f              -0.0f and +0.0f pass
//     :166   Pinhole::projectLinear     fx * x / z + cx: a true division
//     :174   uM < mnMinX || uM > mnMaxX the key frame's int bounds, converted; a NaN passes all four comparisons
//     :189   distMiddlePoint            p3DMc.norm() = sqrt(c0 + (c1 + c2)): the CAMERA-frame norm
//     :191   the band                   0.8f * mfMaxDistance .. 1.2f * mfMaxDistance (src/MapLine.cc:707-719: both from mfMaxDistance)
//     :197-210  start and end point in the camera, both depths tested before either is projected
//     :214   invSz = 1.0f / z
//   LineMatcher::Fuse
//     :2103  PO = p3DMw - Ow            the WORLD middle point
//     :2113  PO.dot(Pn) < 0.5 * distMiddlePoint   the dot in f32 as c0 + (c1 + c2), the comparison in f64
//     :2116  MapLine::PredictScale(distMiddlePoint, pKF) (src/MapLine.cc:721-736): ratio = mfMaxDistance / dist (f32), then
//            track_level.hpp with mfLineLogScaleFactor / mnLineScaleLevels.  distMiddlePoint == 0 (ratio NaN or infinite, the
//            level undefined in the reference) is reported as kDegenerate
//     :2122  Geom2DUtils::GetLine2dRepresentation (include/Geom2DUtils.h:135-159).  End points that coincide in f32 (or whose
//            squared distance underflows to 0): the normal is 0 * inf, theta a NaN and the cell index an int cast of it —
//            undefined in the reference, kDegenerate here
//     :2124  scale = mvLineScaleFactors[level]; deltaTheta = kDeltaTheta * scale; deltaD = (th * kDeltaD) * scale
//     :2127  KeyFrame::GetLineFeaturesInArea (src/KeyFrame.cc:1291-1402): no level filter inside; the theta rows in f64
//            (thetaMin - LINE_THETA_MIN is a double expression), the d columns in f32 with the key frame's INT mnMaxDiag; the split
//            at +-pi/2 negates d and lists the wrapped sub-window FIRST; column ix outer, row iy inner, insertion order in a cell
//     :2148  the level band [level - 1, level]
//     :2198-2206  the two point-to-line distances, each squared, times mvLineInvLevelSigma2[klLevel], compared in F32 against
//            kChiSquareLinePointProj (a const float 3.84)
//     :2215-2250  the same on the right image when mvuRightLineStart is not empty and both entries are >= 0; the projected
//            line's right-image representation from uS - mbf * invSz (a product with the projection's own inverse depth)
//     :2259  dist < bestDist from 256: the first minimum in enumeration order
//
// The Sim3 overload of loop closing and map merging, LineMatcher::Fuse(pKF, Scw, vpLines, th, vpReplaceLine) (:2321-2561), is the
// gate policy kGateSim3 of the same text: the same ProjectLineWithCheck overload (:2397) on the caller's decomposition of Scw
// (plvs_hip.h: plvs_keyframe_sim3_pose; Ow = -Rcw.transpose() * tcw, :2327), and per candidate the two point-to-line distances times
// mvLineInvLevelSigma2[nPredictedLevel] (:2463-2464), NOT [klLevel]; the right-image check is compiled out (#if 0, :2471).
// bestDist starts at INT_MAX (:2426) and (bestDist <= TH_LOW) && (bestIdx >= 0) decides (:2530): 256 serves.
//
// The loop-closing LineMatcher::SearchByProjection(pKF, Scw, vpLines, vpMatched, th, ratioHamming) (:1767-1909) and its overload
// with vpLinesKFs / vpMatchedKF (:1913-2037) are the gate policy kGateBand of the same text: the Sim3 overload's front (:1770-1773,
// :1827-1844), a candidate gate of the level band alone (:1868) behind the exclusion `if(vpMatched[idx]) continue` (:1863:
// `claimed`), and (bestDist <= TH_LOW * ratioHamming) && (bestIdx >= 0) as an integer cut (:1894: `cut`; loop_search_pair.hpp).
//
// THETA NEEDS THE HOST'S atan2.  GetLine2dRepresentation calls atan2(ny, nx) on two floats with <math.h> in scope: the
// compiled reference calls atan2f (tests/golden/line_fuse_reference_facts.json records the undefined symbol).  No device
// arctangent equals it bit for bit, and theta decides the > pi refusal, the two split tests and the row indices of every
// sub-window.  So, as track_level.hpp does for the logarithm: the kernel takes theta_d = the f64 arctangent rounded to f32,
// evaluates every theta-dependent decision (theta_plan) for theta_d and its f32 neighbours within +-kThetaUlps, and marks the pair
// AMBIGUOUS when any of them differs from theta_d's; ambiguous pairs are evaluated once more by the host's code after the wait.
//
// kThetaUlps.  Let CR be the correctly rounded f32 arctangent of the two f32 inputs.
//   the host's atan2f: glibc states a largest known error of 1 ulp for atan2f (its manual, "Known Maximum Errors in Math
//     Functions"; since 2.41 the function is correctly rounded).  A result within 1 ulp of the exact value lies at most ONE f32
//     step from CR.  tests/test_line_fuse.py measures the deviation from CR (via atan2l) over a seeded sample and asserts <= 1.
//   theta_d: an f64 arctangent of a few f64 ulp, rounded to f32: CR, except where the exact value lies within ~2^-50 relative of a
//     rounding boundary, and then ONE step from it.
// So the host's theta lies within 2 steps of theta_d.  kThetaUlps = 4 is twice that: a safety factor of 2.
// Marked fraction: a pair has at most four row edges and two split tests, each marks a band of 2 * 4 + 1 steps of <= 1.2e-7 rad; a
// row is pi / 36 = 0.087 rad wide: 6 * 1.1e-6 / 0.087 ~ 7e-5 at most, of the order 1e-5 (the host test counts it; it asserts no
// figure).  A window that would need a third sub-window (a sub-window that itself crosses +-pi/2: only with deltaTheta near
// pi / 2) is marked ambiguous too: the host's code walks the reference's recursion as it is written.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "track_level.hpp"

#if defined(__HIPCC__)
#define PLVS_LFUSE_FN __host__ __device__ inline
#else
#define PLVS_LFUSE_FN inline
#endif

namespace plvs {
namespace linefuse {

// the `continue` a pair left by (plvs_hip.h: PLVS_LINE_FUSE_*)
enum Reached : int {
  kSkipped = 0, kMiddleBehind = 1, kMiddleOutside = 2, kTooNear = 3, kTooFar = 4, kEndBehind = 5, kEndOutside = 6, kViewAngle = 7,
  kDegenerate = 8, kEmptyWindow = 9, kNoCandidate = 10, kAboveThLow = 11, kCandidate = 12,
  kFullTheta = 13   // internal: fabs(thetaMin - thetaMax) > M_PI, where the reference leaves the process — the call is refused
};
constexpr int kRows = 36, kCols = 160;             // LINE_THETA_GRID_ROWS, LINE_D_GRID_COLS (include/Frame.h:72-73)
constexpr int kThLow = 60;                         // LineMatcher::TH_LOW (src/LineMatcher.cc:88)
constexpr int kThetaUlps = 4;
enum Gate : int { kGateSE3 = 0, kGateSim3 = 1, kGateBand = 2 };   // which overload's candidate gate (see the head)
constexpr float kChi2 = 3.84f;                     // kChiSquareLinePointProj, a const float (:98)
constexpr float kEps = 1.1920929e-07f;             // std::numeric_limits<float>::epsilon()
constexpr double kPi = 3.14159265358979323846, kPi2 = 1.57079632679489661923;   // M_PI, M_PI_2

struct V3 { float x, y, z; };

// what the pair loop reads of pKF besides its grid
struct KfConst {
  float R[9], t[3], Ow[3];                // mRcw in Eigen::Matrix3f's memory layout (column-major), mtcw, GetCameraCenter()
  float fx, fy, cx, cy, mbf;              // mvLinearParameters, mbf
  float min_x, max_x, min_y, max_y;       // mnMinX .. mnMaxY, int in the key frame
  float diag;                             // (float)KeyFrame::mnMaxDiag, an int: the Frame's float diagonal truncated
  float theta_inv, d_inv;                 // mfLineGridElementThetaInv / DInv, copied from the Frame (its FLOAT diagonal)
  float log_scale_factor;                 // mfLineLogScaleFactor
  int n_levels;                           // mnLineScaleLevels
};

struct Rep { float nx, ny, d; };

struct Front {
  int reached;        // a rejection, or kEmptyWindow: every test passed, the window is next
  int ambiguous;      // predict_level's mark: the host's logarithm decides the level
  int level;
  float ratio;
  float uS, vS, uE, vE, invSz, invEz;
  Rep rep;            // of the projected line; theta is the caller's (host: atan2f, kernel: theta_device)
};

PLVS_LFUSE_FN V3 to_camera(const KfConst& K, const V3& p) {
  const float* R = K.R;
  return V3{(R[0] * p.x + (R[3] * p.y + R[6] * p.z)) + K.t[0], (R[1] * p.x + (R[4] * p.y + R[7] * p.z)) + K.t[1],
            (R[2] * p.x + (R[5] * p.y + R[8] * p.z)) + K.t[2]};
}
PLVS_LFUSE_FN bool outside(const KfConst& K, float u, float v) {
  if (u < K.min_x || u > K.max_x) return true;
  if (v < K.min_y || v > K.max_y) return true;
  return false;
}
// GetLine2dRepresentationNoTheta; false: the squared norm is 0 (see the head)
PLVS_LFUSE_FN bool representation(float xs, float ys, float xe, float ye, Rep* r) {
  float nx = ye - ys, ny = xs - xe;
  if (nx < 0) { nx *= -1.0f; ny *= -1.0f; }
  const float n2 = nx * nx + ny * ny;
  const float inv = 1.0f / sqrtf(n2);
  nx *= inv;
  ny *= inv;
  r->nx = nx;
  r->ny = ny;
  r->d = nx * xe + ny * ye;
  return n2 != 0.0f;
}

// ProjectLineWithCheck and :2103-2122 for one pair
PLVS_LFUSE_FN Front front(const KfConst& K, const float* start, const float* end, const float* normal, float max_dist) {
  Front f;
  f.reached = kMiddleBehind; f.ambiguous = 0; f.level = 0; f.ratio = 0.0f;
  f.uS = f.vS = f.uE = f.vE = f.invSz = f.invEz = 0.0f;
  f.rep = Rep{0.0f, 0.0f, 0.0f};
  const V3 S{start[0], start[1], start[2]}, E{end[0], end[1], end[2]};
  const V3 Mw{(S.x + E.x) * 0.5f, (S.y + E.y) * 0.5f, (S.z + E.z) * 0.5f};
  const V3 Mc = to_camera(K, Mw);
  if (Mc.z < 0.0f) return f;
  const float uM = K.fx * Mc.x / Mc.z + K.cx, vM = K.fy * Mc.y / Mc.z + K.cy;
  f.reached = kMiddleOutside;
  if (outside(K, uM, vM)) return f;
  const float dist = sqrtf(Mc.x * Mc.x + (Mc.y * Mc.y + Mc.z * Mc.z));
  const float max_distance = 1.2f * max_dist, min_distance = 0.8f * max_dist;
  f.reached = kTooNear;
  if (dist < min_distance) return f;
  f.reached = kTooFar;
  if (dist > max_distance) return f;
  const V3 Sc = to_camera(K, S);
  f.reached = kEndBehind;
  if (Sc.z < 0.0f) return f;
  const V3 Ec = to_camera(K, E);
  if (Ec.z < 0.0f) return f;
  f.invSz = 1.0f / Sc.z;
  f.uS = K.fx * Sc.x / Sc.z + K.cx;
  f.vS = K.fy * Sc.y / Sc.z + K.cy;
  f.reached = kEndOutside;
  if (outside(K, f.uS, f.vS)) return f;
  f.invEz = 1.0f / Ec.z;
  f.uE = K.fx * Ec.x / Ec.z + K.cx;
  f.vE = K.fy * Ec.y / Ec.z + K.cy;
  if (outside(K, f.uE, f.vE)) return f;
  const V3 PO{Mw.x - K.Ow[0], Mw.y - K.Ow[1], Mw.z - K.Ow[2]};
  const float dot = PO.x * normal[0] + (PO.y * normal[1] + PO.z * normal[2]);
  f.reached = kViewAngle;
  if ((double)dot < 0.5 * (double)dist) return f;
  f.reached = kDegenerate;
  if (dist == 0.0f) return f;
  f.ratio = max_dist / dist;
  const LevelChoice lc = predict_level(f.ratio, K.log_scale_factor, K.n_levels);
  f.level = lc.level;
  f.ambiguous = lc.ambiguous;
  if (!representation(f.uS, f.vS, f.uE, f.vE, &f.rep)) return f;
  f.reached = kEmptyWindow;
  return f;
}

// the f32 value `steps` representable values away from x (finite x, small steps)
PLVS_LFUSE_FN float f32_step(float x, int steps) {
  int32_t b;
  memcpy(&b, &x, 4);
  int32_t ordered = b < 0 ? (int32_t)0x80000000 - b : b;   // monotone in x; -0.0f and +0.0f share 0
  ordered += steps;
  b = ordered < 0 ? (int32_t)0x80000000 - ordered : ordered;
  float y;
  memcpy(&y, &b, 4);
  return y;
}
// theta on the device: the f64 arctangent rounded to f32 (see the head)
PLVS_LFUSE_FN float theta_device(const Rep& r) { return (float)atan2((double)r.ny, (double)r.nx); }

// a cell index of GetLineFeaturesInArea before its clamp: (int)floor(v), with values the clamp would cut anyway kept inside int
PLVS_LFUSE_FN int cell_of(double v, int cells) {
  if (!(v > -1.0)) return -1;   // (and a NaN, which the reference's cast leaves undefined)
  if (v > (double)cells) return cells;
  return (int)floor(v);
}

// One leaf of GetLineFeaturesInArea(thetaMin, thetaMax, dMin, dMax, ...), :1359-1382
struct Leaf { float tmin, tmax, dmin, dmax; };
struct Cells { int r0, r1, c0, c1, ok; };
PLVS_LFUSE_FN void leaf_rows(const KfConst& K, float tmin, float tmax, int* r0, int* r1, int* ok) {
  const int a = cell_of(((double)tmin + kPi2) * (double)K.theta_inv, kRows);
  *r0 = a < 0 ? 0 : a;
  const int b = cell_of(((double)tmax + kPi2) * (double)K.theta_inv, kRows);
  *r1 = b > kRows - 1 ? kRows - 1 : b;
  *ok = (*r0 < kRows && *r1 >= 0) ? 1 : 0;
}
PLVS_LFUSE_FN Cells leaf_cells(const KfConst& K, const Leaf& w) {
  Cells c;
  leaf_rows(K, w.tmin, w.tmax, &c.r0, &c.r1, &c.ok);
  const int a = cell_of((double)((w.dmin + K.diag) * K.d_inv), kCols);
  c.c0 = a < 0 ? 0 : a;
  const int b = cell_of((double)((w.dmax + K.diag) * K.d_inv), kCols);
  c.c1 = b > kCols - 1 ? kCols - 1 : b;
  if (c.c0 >= kCols || c.c1 < 0) c.ok = 0;
  return c;
}

// Everything theta decides: the refusal, which branch splits, the sub-windows' theta ranges and their rows.
struct ThetaPlan {
  int full;        // fabs(thetaMin - thetaMax) > M_PI
  int branch;      // 0: no split, 1: thetaMin < -pi/2, 2: thetaMax > pi/2
  int nested;      // a sub-window would split again: the host's recursion takes the pair
  int n;           // leaves: 1 or 2, in the reference's order
  float tmin[2], tmax[2];
  int flip[2];     // the leaf's d range is [-dMax, -dMin]
  int r0[2], r1[2], ok[2];
};
PLVS_LFUSE_FN ThetaPlan theta_plan(const KfConst& K, float theta, float dtheta) {
  ThetaPlan p;
  const float tmin = theta - dtheta, tmax = theta + dtheta;
  p.full = ((double)fabsf(tmin - tmax) > kPi) ? 1 : 0;
  p.nested = 0;
  p.flip[0] = p.flip[1] = 0;
  p.tmin[1] = p.tmax[1] = 0.0f;
  p.r0[1] = p.r1[1] = p.ok[1] = 0;
  if ((double)tmin < -kPi2) {
    p.branch = 1; p.n = 2;
    p.tmin[0] = (float)((double)tmin + kPi); p.tmax[0] = (float)(kPi2 - (double)kEps); p.flip[0] = 1;
    p.tmin[1] = (float)(-kPi2 + (double)kEps); p.tmax[1] = tmax;
  } else if ((double)tmax > kPi2) {
    p.branch = 2; p.n = 2;
    p.tmin[0] = (float)(-kPi2 + (double)kEps); p.tmax[0] = (float)((double)tmax - kPi); p.flip[0] = 1;
    p.tmin[1] = tmin; p.tmax[1] = (float)(kPi2 - (double)kEps);
  } else {
    p.branch = 0; p.n = 1;
    p.tmin[0] = tmin; p.tmax[0] = tmax;
  }
  for (int s = 0; s < p.n; ++s) {
    if (p.n == 2 && ((double)p.tmin[s] < -kPi2 || (double)p.tmax[s] > kPi2)) p.nested = 1;
    leaf_rows(K, p.tmin[s], p.tmax[s], &p.r0[s], &p.r1[s], &p.ok[s]);
  }
  return p;
}
PLVS_LFUSE_FN bool same_decisions(const ThetaPlan& a, const ThetaPlan& b) {
  if (a.full != b.full || a.branch != b.branch || a.nested != b.nested) return false;
  for (int s = 0; s < a.n; ++s)
    if (a.r0[s] != b.r0[s] || a.r1[s] != b.r1[s] || a.ok[s] != b.ok[s]) return false;
  return true;
}
// 1: some f32 within kThetaUlps of theta decides differently than theta
PLVS_LFUSE_FN int theta_ambiguous(const KfConst& K, float theta, float dtheta, const ThetaPlan& p) {
  for (int j = -kThetaUlps; j <= kThetaUlps; ++j) {
    if (j == 0) continue;
    if (!same_decisions(p, theta_plan(K, f32_step(theta, j), dtheta))) return 1;
  }
  return 0;
}
PLVS_LFUSE_FN Leaf plan_leaf(const ThetaPlan& p, int s, float dmin, float dmax) {
  return p.flip[s] ? Leaf{p.tmin[s], p.tmax[s], -dmax, -dmin} : Leaf{p.tmin[s], p.tmax[s], dmin, dmax};
}

// a key line as the candidate loop reads it: one load, plus the descriptor
struct Member {
  float sx, sy, ex, ey;     // mvKeyLinesUn[idx].startPointX .. endPointY
  float urs, ure;           // mvuRightLineStart / End [idx]; -1, -1 when the key frame's vectors are empty
  int octave, idx;
};

// the right-image representation of the projected line (:2220-2226), formed once per pair
PLVS_LFUSE_FN Rep right_rep(const KfConst& K, const Front& f) {
  Rep r;
  (void)representation(f.uS - K.mbf * f.invSz, f.vS, f.uE - K.mbf * f.invEz, f.vE, &r);
  return r;
}
// :2148-2250 (kGateSim3: :2437-2467, rr is not read; kGateBand: :1868 alone) — true: the candidate's descriptor distance is taken
template <Gate kGate = kGateSE3>
PLVS_LFUSE_FN bool candidate_gate(const Rep& pr, const Rep& rr, int level, const Member& m, const float* inv_level_sigma2) {
  if (m.octave < level - 1 || m.octave > level) return false;
  if (kGate == kGateBand) return true;
  const float sig = inv_level_sigma2[kGate == kGateSim3 ? level : m.octave];
  const float ds = pr.nx * m.sx + pr.ny * m.sy - pr.d;
  const float de = pr.nx * m.ex + pr.ny * m.ey - pr.d;
  const float ds2 = ds * ds, de2 = de * de;
  if (ds2 * sig > kChi2 || de2 * sig > kChi2) return false;
  if (kGate == kGateSE3 && m.urs >= 0 && m.ure >= 0) {
    const float dsr = rr.nx * m.urs + rr.ny * m.sy - rr.d;
    const float der = rr.nx * m.ure + rr.ny * m.ey - rr.d;
    const float dsr2 = dsr * dsr, der2 = der * der;
    if (dsr2 * sig > kChi2 || der2 * sig > kChi2) return false;
  }
  return true;
}

PLVS_LFUSE_FN int hamming256(const uint32_t* a, const uint32_t* b) {
  int d = 0;
  for (int i = 0; i < 8; ++i) {
    uint32_t v = a[i] ^ b[i];
    v = v - ((v >> 1) & 0x55555555u);
    v = (v & 0x33333333u) + ((v >> 2) & 0x33333333u);
    d += (int)((((v + (v >> 4)) & 0x0F0F0F0Fu) * 0x01010101u) >> 24);
  }
  return d;
}

// ---------------------------------------------------------------------------------------------------------- host only
// what the host reads of a key line (plvs_keyline's fields, handed over by the caller of build_grid)
struct KeyLineIn { float sx, sy, ex, ey; int octave; };

// The key frame's (theta, d) grid — Frame::PosLineInGrid (src/Frame.cc:1477-1495) with the FRAME's float diagonal, copied
// into the key frame cell by cell (src/KeyFrame.cc:189-198) — as CSR cell starts (cells in (column, row) order, ix * kRows + iy)
// over members in insertion order.  double_overload: the arctangent is ::atan2(double, double) rounded to f32.
struct Grid {
  std::vector<int> start;         // kCols * kRows + 1
  std::vector<Member> members;    // the key lines PosLineInGrid placed
};
inline float theta_host(const Rep& r, int double_overload) {
  return double_overload ? (float)std::atan2((double)r.ny, (double)r.nx) : std::atan2(r.ny, r.nx);
}
template <typename GetLine>
inline void build_grid(int n, GetLine line, const float* u_right_start, const float* u_right_end, float max_diag, float theta_inv, float d_inv,
                       int double_overload, Grid* g) {
  std::vector<int> cell((size_t)n, -1);
  g->start.assign((size_t)kRows * kCols + 1, 0);
  for (int i = 0; i < n; ++i) {
    const KeyLineIn k = line(i);
    Rep r;
    (void)representation(k.sx, k.sy, k.ex, k.ey, &r);
    const float theta = theta_host(r, double_overload);
    const double row = std::round(((double)theta + kPi2) * (double)theta_inv);   // theta - LINE_THETA_MIN: a double expression
    const float col = std::round((r.d + max_diag) * d_inv);
    if (!(row >= 0.0 && row < (double)kRows && col >= 0.0f && col < (float)kCols)) continue;   // (a NaN stays out as well)
    cell[i] = (int)col * kRows + (int)row;
    ++g->start[(size_t)cell[i] + 1];
  }
  for (size_t c = 0; c + 1 < g->start.size(); ++c) g->start[c + 1] += g->start[c];
  g->members.resize((size_t)g->start.back());
  std::vector<int> fill((size_t)kRows * kCols, 0);
  for (int i = 0; i < n; ++i) {
    if (cell[i] < 0) continue;
    const KeyLineIn k = line(i);
    const bool stereo = u_right_start != nullptr && u_right_end != nullptr;
    g->members[(size_t)g->start[cell[i]] + fill[cell[i]]++] =
        Member{k.sx, k.sy, k.ex, k.ey, stereo ? u_right_start[i] : -1.0f, stereo ? u_right_end[i] : -1.0f, k.octave, i};
  }
}

struct KfGrid {
  const int* start;
  const Member* members;
  const uint8_t* desc;               // Nlines x 32, 4-byte aligned
  const float* scale_factors;        // mvLineScaleFactors
  const float* inv_level_sigma2;     // mvLineInvLevelSigma2
};

struct Result { int best_idx, best_dist, reached; };

struct Walk {
  const KfConst* K;
  const KfGrid* G;
  const Rep *pr, *rr;
  int level;
  const uint32_t* qd;
  int best, best_idx;
  bool any, gated;
  Gate gate;
  const uint8_t* claimed;   // may be null: the members a greedy overload's earlier pairs took, left out behind the gate
};
inline void walk_leaf(Walk& w, const Leaf& leaf) {
  const Cells c = leaf_cells(*w.K, leaf);
  if (!c.ok) return;
  for (int ix = c.c0; ix <= c.c1; ++ix) {
    const int s = w.G->start[ix * kRows + c.r0], e = w.G->start[ix * kRows + c.r1 + 1];
    for (int j = s; j < e; ++j) {
      const Member& m = w.G->members[j];
      w.any = true;
      if (!(w.gate == kGateSim3   ? candidate_gate<kGateSim3>(*w.pr, *w.rr, w.level, m, w.G->inv_level_sigma2)
            : w.gate == kGateBand ? candidate_gate<kGateBand>(*w.pr, *w.rr, w.level, m, w.G->inv_level_sigma2)
                                  : candidate_gate<kGateSE3>(*w.pr, *w.rr, w.level, m, w.G->inv_level_sigma2)))
        continue;
      w.gated = true;
      if (w.claimed && w.claimed[m.idx]) continue;
      uint32_t td[8];
      std::memcpy(td, w.G->desc + 32 * (size_t)m.idx, 32);
      const int d = hamming256(w.qd, td);
      if (d < w.best) { w.best = d; w.best_idx = m.idx; }
    }
  }
}
// KeyFrame::GetLineFeaturesInArea(thetaMin, thetaMax, dMin, dMax, ...) as the reference recurses (:1314-1357)
inline void walk_recursive(Walk& w, float tmin, float tmax, float dmin, float dmax, int depth) {
  if (depth > 8) return;   // (the reference's recursion ends after two levels for every interval no wider than pi)
  if ((double)tmin < -kPi2) {
    walk_recursive(w, (float)((double)tmin + kPi), (float)(kPi2 - (double)kEps), -dmax, -dmin, depth + 1);
    walk_recursive(w, (float)(-kPi2 + (double)kEps), tmax, dmin, dmax, depth + 1);
    return;
  }
  if ((double)tmax > kPi2) {
    walk_recursive(w, (float)(-kPi2 + (double)kEps), (float)((double)tmax - kPi), -dmax, -dmin, depth + 1);
    walk_recursive(w, tmin, (float)(kPi2 - (double)kEps), dmin, dmax, depth + 1);
    return;
  }
  walk_leaf(w, Leaf{tmin, tmax, dmin, dmax});
}

// :2124-2263 for a pair whose tests passed, serially, with the level and theta given (the host's).  cut: the largest distance taken
inline Result search_window(const KfConst& K, const KfGrid& G, const Front& f, int level, float theta, float th, const uint8_t* line_desc,
                            Gate gate = kGateSE3, const uint8_t* claimed = nullptr, int cut = kThLow) {
  const float scale = G.scale_factors[level];
  const float dtheta = (float)(10 * kPi / 180.f) * scale;   // Frame::kDeltaTheta (src/Frame.cc:99)
  const float dd = th * 100.0f * scale;                     // th * Frame::kDeltaD * scale, left to right
  const float tmin = theta - dtheta, tmax = theta + dtheta;
  if ((double)fabsf(tmin - tmax) > kPi) return Result{-1, -1, kFullTheta};
  uint32_t qd[8];
  std::memcpy(qd, line_desc, 32);
  const Rep rr = right_rep(K, f);
  Walk w{&K, &G, &f.rep, &rr, level, qd, 256, -1, false, false, gate, claimed};
  walk_recursive(w, tmin, tmax, f.rep.d - dd, f.rep.d + dd, 0);
  Result res{-1, -1, kEmptyWindow};
  if (!w.any) return res;
  res.reached = !w.gated ? kNoCandidate : (w.best <= cut ? kCandidate : kAboveThLow);
  if (res.reached == kCandidate) { res.best_idx = w.best_idx; res.best_dist = w.best; }
  return res;
}

// the whole pair on the host: level and theta are the reference's own expressions on the host's libm
inline Result pair_host(const KfConst& K, const KfGrid& G, const float* start, const float* end, const float* normal, float max_dist,
                        const uint8_t* line_desc, float th, int log_double_overload, int atan_double_overload, Gate gate = kGateSE3,
                        const uint8_t* claimed = nullptr, int cut = kThLow) {
  const Front f = front(K, start, end, normal, max_dist);
  if (f.reached != kEmptyWindow) return Result{-1, -1, f.reached};
  return search_window(K, G, f, predict_level_host(f.ratio, K.log_scale_factor, K.n_levels, log_double_overload),
                       theta_host(f.rep, atan_double_overload), th, line_desc, gate, claimed, cut);
}

}  // namespace linefuse
}  // namespace plvs
