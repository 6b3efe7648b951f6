// The level rule of the frustum test: MapPoint::PredictScale(const float&, Frame*) (reference src/MapPoint.cc:598-613) and
// MapLine::PredictScale (src/MapLine.cc:738-753),
//     ratio  = mfMaxDistance / dist                      (f32)
//     nScale = ceil(log(ratio) / logScaleFactor)         clamped to [0, levels - 1]
// where `log` is the HOST's libm — std::log(float) under the `using namespace std` of the reference's units, ::log(double)
// without it — and no device logarithm equals either bit for bit.  Shared by the kernel (frame_track.hip), the library's
// host code and tests/host/track_level_host.cpp.
//
// The kernel evaluates the quotient q in f64 and takes its ceiling; the element is AMBIGUOUS when q lies within eps of an
// integer, and only those go through the host's expression (predict_level_host) after the call's wait.
//
// eps.  Let Q be the exact quotient log(ratio) / factor of the two f32 inputs.
//   float overload:  logf errs by at most 1 ulp of its result, a relative 2^-23; the f32 division rounds once more,
//                    a relative 2^-24; so |q32 - Q| <= (2^-23 + 2^-24 + 2^-47) |Q| < 1.5 * 2^-23 |Q|.
//   double overload: log and the f64 division err by a few 2^-53 |Q|: nothing beside the above.
//   this rule's own q: an f64 log of at most a few ulp and one f64 division, again ~2^-51 |Q|.
// A host ceiling can differ from ceil(q) only if an integer lies between q and the host's quotient, i.e. within
// 1.5 * 2^-23 |Q| + 2^-50 |Q| of q.  eps = 6 * 2^-23 * |q| + 2^-40 is four times that bound (the constant covers |q| ~ 0,
// where ratio == 1 gives q == 0 exactly on every path).  |Q| only matters up to `levels`: beyond the clamps the ceiling is
// not looked at, so with 8 levels eps <= 5.8e-6; over the ratios the band admits the mean eps is about 2.5e-6 and a fraction
// of about 2 eps ~ 5e-6 of the elements is marked (tests/host/track_level_host.cpp counts 3e-6).
// The largest ratio the distance band admits is mfMaxDistance / (0.8f * mfMinDistance), about 1.2^levels / 0.8: |Q| stays
// below levels + 2.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define PLVS_LEVEL_HD __host__ __device__
#else
#define PLVS_LEVEL_HD
#endif

namespace plvs {

struct LevelChoice {
  int level;       // the rule's own choice
  int ambiguous;   // 1: the host's expression decides
};

PLVS_LEVEL_HD inline int clamp_level(int n, int levels) { return n < 0 ? 0 : (n >= levels ? levels - 1 : n); }

PLVS_LEVEL_HD inline LevelChoice predict_level(float ratio, float log_scale_factor, int levels) {
  LevelChoice c{0, 0};
  const double q = log((double)ratio) / (double)log_scale_factor;
  if (!(q > -1.0)) return c;                                   // ceil <= 0 on every path (and NaN / -inf): level 0
  if (q > (double)levels) { c.level = levels - 1; return c; }  // ceil >= levels on every path (and +inf)
  const double up = ceil(q);
  const double nearest = floor(q + 0.5);
  const double eps = 6.0 * 1.1920928955078125e-07 * fabs(q) + 9.094947017729282e-13;   // 6 * 2^-23 |q| + 2^-40
  c.level = clamp_level((int)up, levels);
  // an integer at or above levels - 1 (or below 0) cannot change the clamped level
  c.ambiguous = (fabs(q - nearest) <= eps && nearest >= 0.0 && nearest <= (double)(levels - 2)) ? 1 : 0;
  return c;
}

// The reference's expression, on the host's libm.  double_overload = 0: std::log(float) (what the compiled reference
// takes: tests/golden/track_local_reference_facts.json); 1: ::log(double).
inline int predict_level_host(float ratio, float log_scale_factor, int levels, int double_overload) {
  int n;
  if (double_overload) n = (int)std::ceil(std::log((double)ratio) / log_scale_factor);
  else n = (int)std::ceil(std::log(ratio) / log_scale_factor);
  return clamp_level(n, levels);
}

}  // namespace plvs
