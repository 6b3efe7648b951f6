// The loop-closing SearchByProjection overloads — ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming)
// (reference src/ORBmatcher.cc:509-615), the same with vpPointsKFs / vpMatchedKF (:617-730), and LineMatcher::SearchByProjection(pKF,
// Scw, vpLines, vpMatched, th, ratioHamming) (src/LineMatcher.cc:1767-1909) with its vpLinesKFs / vpMatchedKF overload (:1913-2037)
// — behind their fronts: what makes them GREEDY, in plain C++ that the device entries, the host twins and
// tests/host/loop_search_pair_host.cpp share: one text, two compilers.  Nothing here names HIP or the library's own headers but the
// two pair headers (fuse_pair.hpp, line_fuse_pair.hpp).  The line numbers below are the point overloads'; the line overloads have
// the same three statements at :1863 / :2008, :1894 and :1902.
//
// Per pair the front is fuse_pair.hpp's (gate kGateSim3: the level band alone; the projection policy tells the two overloads
// apart).  Three things differ from the Sim3 Fuse:
//   :587, :701   if(vpMatched[idx]) continue — a member an EARLIER point of the same call took (or that was taken on entry) is left
//                out.  A pair's result depends on the pairs before it: it cannot be one posted winner.
//   :606, :720   bestDist <= TH_LOW * ratioHamming: int * float is a float product, the int on the left is converted.  Every
//                distance is an integer in [0, 256], exact in f32, so d <= lim holds exactly when d <= floor(lim): the cut T.
//                T >= 256 would let a pair without a candidate (bestDist 256, bestIdx -1) write vpMatched[-1]: refused.
//   the match    vpMatched[bestIdx] = pMP: the member is claimed for the points that follow.
//
// So the search is split.  Order-free part (device or host): per pair the kListLen smallest keys (distance, enumeration position)
// among the members inside the level band at or below T, with the count of all such members.  Greedy part (greedy_keyframe, host,
// after the call's one wait): per key frame over the points in index order, a pair takes the first entry of its list nobody has
// claimed.  That is the reference's choice: its loop keeps the first minimum in enumeration order over the unclaimed banded members
// and takes it if it is at or below T, and the list holds exactly those members in (distance, position) order.  Only a list that
// was truncated (count > kListLen) and whose every entry is claimed says nothing about the members behind it: that pair is
// evaluated once more by search_window with the claims made so far.
#pragma once
#include <cstdint>

#include "fuse_pair.hpp"
#include "line_fuse_pair.hpp"

namespace plvs {
namespace loopsearch {

// Entries per posted list.  A pair reads past its first entry only when earlier pairs of the same key frame claimed what it wanted,
// and needs the host only when ALL its entries are claimed while more members stood at or below T.  In a loop candidate's window
// (th 3..8 at 1500 key points: a handful of banded members, of which those at or below T are fewer still) four covers all but
// crowds; each entry costs every lane two registers (key, index) and a round of cross-lane minimum per pair.  With 4 the window
// point kernel takes 38 VGPRs and no scratch (the build's resource report: what the Sim3 Fuse sieve beside it takes; 101 scalar
// registers hold it to 7 waves per SIMD, not these), the line kernel 66 VGPRs against the Sim3 line Fuse's 64, with the 144 bytes of
// scratch that theta's plan has in both; 8 would double the rounds for lists nobody reads.
constexpr int kListLen = 4;

enum Refusal : int { kCutOk = 0, kCutBadRatio = 1, kCutTooWide = 2 };
// the integer cut of (float)d <= (float)th_low * ratio; *cut in [0, 255] when kCutOk
inline Refusal threshold_cut(int th_low, float ratio, int* cut) {
  if (!(ratio >= 0.0f)) return kCutBadRatio;   // (and a NaN)
  const float lim = (float)th_low * ratio;
  if (!(lim < 256.0f)) return kCutTooWide;     // (and an infinity)
  *cut = (int)lim;                             // 0 <= lim < 256: the truncation is the floor, and an integer there is exact in f32
  return kCutOk;
}

// what the order-free part says of one pair
struct PairList {
  int reached;              // the front's rejection (or skipped), else the kind's EMPTY_WINDOW: the window was walked
  bool host;                // the host decides the whole pair at its turn (the level's or theta's ambiguous mark; the host twin: every pair)
  bool any, banded;         // the window had a member; a member passed the level band
  int n;                    // entries
  int count;                // members inside the band at or below T (saturates; > n: the list is truncated)
  int idx[kListLen], dist[kListLen];
};

// the kind's codes (fusepair::Reached / linefuse::Reached)
struct Codes { int empty_window, no_candidate, above_th_low, candidate; };
struct PairResult { int idx, dist, reached; };

struct GreedyCounts { int matches, host_pairs, truncated_pairs, windows; };

// One key frame's greedy pass.  list_of(i) -> PairList; recompute(i, claimed) -> PairResult of the whole pair by the host's code
// against `claimed`.  claimed: n_features bytes, seeded by the caller from `occupied`; match_idx / match_dist / reached (may be
// null): this key frame's m outputs.
template <typename ListOf, typename Recompute>
inline GreedyCounts greedy_keyframe(int m, const Codes& C, ListOf&& list_of, Recompute&& recompute, uint8_t* claimed, int32_t* match_idx,
                                    int32_t* match_dist, uint8_t* reached) {
  GreedyCounts n{0, 0, 0, 0};
  for (int i = 0; i < m; ++i) {
    const PairList L = list_of(i);
    PairResult r{-1, -1, L.reached};
    if (L.host) {
      r = recompute(i, claimed);
      ++n.host_pairs;
    } else if (L.reached == C.empty_window && L.any) {
      r.reached = L.banded ? C.above_th_low : C.no_candidate;
      int e = 0;
      while (e < L.n && claimed[L.idx[e]]) ++e;
      if (e < L.n) {
        r = PairResult{L.idx[e], L.dist[e], C.candidate};
      } else if (L.count > L.n) {   // truncated, every entry claimed: what lies behind the list is the host's to look at
        r = recompute(i, claimed);
        ++n.truncated_pairs;
      }
    }
    if (r.reached == C.candidate) {
      claimed[r.idx] = 1;
      ++n.matches;
    } else {
      r.idx = r.dist = -1;
    }
    if (r.reached >= C.empty_window) ++n.windows;
    match_idx[i] = r.idx;
    match_dist[i] = r.dist;
    if (reached) reached[i] = (uint8_t)r.reached;
  }
  return n;
}

// ---- points
constexpr int kPointThLow = fusepair::kThLow;   // ORBmatcher::TH_LOW
inline Codes point_codes() { return Codes{fusepair::kEmptyWindow, fusepair::kNoCandidate, fusepair::kAboveThLow, fusepair::kCandidate}; }

// one (key frame, point) pair on the host against `claimed`: :541-606 / :650-720 with the reference's own level expression
template <typename Member>
inline PairResult point_pair_host(const fusepair::KfConst& K, const fusepair::KfGrid<Member>& G, int projection, const float* pos,
                                  const float* normal, float min_dist, float max_dist, const uint8_t* point_desc, float th, int cut,
                                  const uint8_t* claimed, int double_overload) {
  const fusepair::Front f = projection == fusepair::kProjectInvz ? fusepair::front<fusepair::kProjectInvz>(K, pos, normal, min_dist, max_dist)
                                                                 : fusepair::front<fusepair::kProjectCamera>(K, pos, normal, min_dist, max_dist);
  if (f.reached != fusepair::kEmptyWindow) return PairResult{-1, -1, f.reached};
  const int level = predict_level_host(f.ratio, K.log_scale_factor, K.n_levels, double_overload);
  const fusepair::Result r = fusepair::search_window<fusepair::kGateSim3>(K, G, f, level, th, point_desc, claimed, cut);
  return PairResult{r.best_idx, r.best_dist, r.reached};
}

// ---- lines
constexpr int kLineThLow = linefuse::kThLow;   // LineMatcher::TH_LOW
inline Codes line_codes() { return Codes{linefuse::kEmptyWindow, linefuse::kNoCandidate, linefuse::kAboveThLow, linefuse::kCandidate}; }

// one (key frame, line) pair on the host against `claimed`: :1788-1894 with the reference's own level and theta expressions
// (reached may be linefuse::kFullTheta: the call is refused)
inline PairResult line_pair_host(const linefuse::KfConst& K, const linefuse::KfGrid& G, const float* start, const float* end, const float* normal,
                                 float max_dist, const uint8_t* line_desc, float th, int cut, const uint8_t* claimed, int log_double_overload,
                                 int atan_double_overload) {
  const linefuse::Result r = linefuse::pair_host(K, G, start, end, normal, max_dist, line_desc, th, log_double_overload, atan_double_overload,
                                                 linefuse::kGateBand, claimed, cut);
  return PairResult{r.best_idx, r.best_dist, r.reached};
}

}  // namespace loopsearch
}  // namespace plvs
