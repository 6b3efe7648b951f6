// ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12) (reference src/ORBmatcher.cc:853-997) and SearchByBoW(pKF, F, vpMapPointMatches)
// (:300-507) as independent jobs.  DBoW2::FeatureVector::addFeature puts a feature under exactly one node, so the greedy claims
// (vbMatched2[idx2] :918, vpMapPointMatches[realIdxF] :359) of one common node never reach another: a job is (pair k, node a of the
// SERIAL side — the side whose features the reference walks in its outer loop), its other side is the LANE side, whose members
// are claimed.  The two overloads are policies of one job:
//                      SearchByBoW(KF1, KF2)                 SearchByBoW(KF, F)
//   serial / lane      KF1 / KF2[k]                          KF[k] / F
//   serial gate        valid1 (:896-900)                     kf_valid[k] (:336-342)
//   lane gate          claimed || !valid2 (:918-922)         claimed (:359)
//   accept             bestDist1 <  TH_LOW (:940)            bestDist1 <= TH_LOW (:408)
//   ratio              (float)bestDist1 < nn_ratio * (float)bestDist2, in f32 (:942, :410)
// This header: the per-call table both the kernel (orb_bow_search.hip) and the host twin read, the record a serial-side list
// position posts, the host twin of a pair, and what create and the frame entry refuse of a feature vector.  Internal.
#pragma once
#include <vector>

#include "common.hpp"

namespace plvs {
namespace bowsearch {

constexpr int kThLow = 50;          // ORBmatcher::TH_LOW, src/ORBmatcher.cc:58
constexpr int kPosBits = 23;        // a key is dist << 23 | list position; handles and frames hold fewer than 2^23 key points
constexpr uint32_t kNoKey = (256u << kPosBits) | ((1u << kPosBits) - 1u);   // bestDist = 256, nobody

// one side of a pair: the feature vector (offsets from 0, `idx` the concatenated lists), the descriptors, the gate bytes (null: all pass)
struct Side {
  const uint32_t* node_id;
  const int32_t* off;
  const uint32_t* idx;
  const uint4* desc;
  const uint8_t* valid;
  int nnodes;
};

// pair k of a call.  rec_at: its first record (one per serial-side list position); gate_at: its first gate byte in the call's
// device scratch (one per lane-side list position; only jobs with more than 64 lane-side members use theirs)
struct Pair {
  Side s, l;
  int rec_at, gate_at;
};

// what a serial-side list position posts: x — the lane-side FEATURE it took, -1 none; y — bestDist1 | bestDist2 << 16, or -1 where
// nothing was evaluated (the feature failed the serial gate, or its node is not on the other side)
__host__ __device__ inline int2 pack(int taken, int d1, int d2) { return make_int2(taken, d1 | (d2 << 16)); }
__host__ __device__ inline int2 not_evaluated() { return make_int2(-1, -1); }

template <bool kFrameKind>
__host__ __device__ inline bool accepts(int d1, int d2, float nn_ratio) {
  return (kFrameKind ? d1 <= kThLow : d1 < kThLow) && (float)d1 < nn_ratio * (float)d2;
}

// ORBmatcher::DescriptorDistance (:2198-2225)
inline int distance_host(const uint4* a, const uint4* b) {   // (a caller's frame descriptors need not be aligned)
  uint64_t pa[4], pb[4];
  memcpy(pa, a, 32);
  memcpy(pb, b, 32);
  int d = 0;
  for (int w = 0; w < 4; ++w) d += __builtin_popcountll(pa[w] ^ pb[w]);
  return d;
}

// first position of `node` in ids[0, n), or n: std::map::lower_bound
__host__ __device__ inline int lower_bound(const uint32_t* ids, int n, uint32_t node) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ids[mid] < node) lo = mid + 1; else hi = mid;
  }
  return lo;
}

struct JobCounts { int common = 0, multi_pass = 0; };

// (pair, node) jobs with a common node, and those whose lane-side list is longer than one pass of 64: the intersection walk of :885-974
inline JobCounts count_jobs(const Side& s, const Side& l) {
  JobCounts c;
  int a = 0, b = 0;
  while (a < s.nnodes && b < l.nnodes) {
    if (s.node_id[a] == l.node_id[b]) {
      ++c.common;
      c.multi_pass += l.off[b + 1] - l.off[b] > 64;
      ++a; ++b;
    } else if (s.node_id[a] < l.node_id[b]) ++a;
    else ++b;
  }
  return c;
}

// The host twin: every job of pair T, serially, on host pointers; R: the pair's records.  `open` is scratch.
template <bool kFrameKind>
inline void pair_host(const Pair& T, float nn_ratio, int2* R, std::vector<uint8_t>* open) {
  for (int a = 0; a < T.s.nnodes; ++a) {
    const int s0 = T.s.off[a], s1 = T.s.off[a + 1];
    const int b = lower_bound(T.l.node_id, T.l.nnodes, T.s.node_id[a]);
    if (b == T.l.nnodes || T.l.node_id[b] != T.s.node_id[a]) {
      for (int p = s0; p < s1; ++p) R[p] = not_evaluated();
      continue;
    }
    const int l0 = T.l.off[b], len = T.l.off[b + 1] - l0;
    open->resize((size_t)len);
    for (int q = 0; q < len; ++q) (*open)[q] = T.l.valid ? T.l.valid[T.l.idx[l0 + q]] != 0 : 1;
    for (int p = s0; p < s1; ++p) {
      const uint32_t i1 = T.s.idx[p];
      if (!T.s.valid[i1]) { R[p] = not_evaluated(); continue; }
      int best1 = 256, best2 = 256, best = -1;
      for (int q = 0; q < len; ++q) {
        if (!(*open)[q]) continue;
        const int d = distance_host(T.s.desc + 2 * (size_t)i1, T.l.desc + 2 * (size_t)T.l.idx[l0 + q]);
        if (d < best1) { best2 = best1; best1 = d; best = q; }
        else if (d < best2) best2 = d;
      }
      if (accepts<kFrameKind>(best1, best2, nn_ratio)) {
        (*open)[best] = 0;
        R[p] = pack((int)T.l.idx[l0 + best], best1, best2);
      } else {
        R[p] = pack(-1, best1, best2);
      }
    }
  }
}

// What plvs_hip_keyframe_create_bow and the frame entry refuse of a feature vector over n features.  listed / longest: may be null.
inline int check_featvec(const plvs_featvec_view& v, int n, int* listed, int* longest) {
  PLVS_REQUIRE(v.nnodes >= 0, "negative node count");
  if (listed) *listed = 0;
  if (longest) *longest = 0;
  if (v.nnodes == 0) return PLVS_OK;
  PLVS_REQUIRE(v.node_id && v.offset, "null feature-vector array");
  PLVS_REQUIRE(v.offset[0] >= 0, "negative offset");
  int longest_ = 0;
  for (int a = 0; a < v.nnodes; ++a) {
    PLVS_REQUIRE(a == 0 || v.node_id[a - 1] < v.node_id[a], "node ids must ascend strictly (std::map order)");
    PLVS_REQUIRE(v.offset[a] <= v.offset[a + 1], "offsets not monotone");
    longest_ = std::max(longest_, v.offset[a + 1] - v.offset[a]);
  }
  const int total = v.offset[v.nnodes] - v.offset[0];
  PLVS_REQUIRE(total == 0 || v.index, "null feature-vector array");
  std::vector<uint8_t> seen((size_t)n, 0);
  for (int p = v.offset[0]; p < v.offset[v.nnodes]; ++p) {
    PLVS_REQUIRE(v.index[p] < (uint32_t)n, "feature index out of range");
    PLVS_REQUIRE(!seen[v.index[p]], "a feature index listed more than once (DBoW2 puts a feature under one node)");
    seen[v.index[p]] = 1;
  }
  if (listed) *listed = total;
  if (longest) *longest = longest_;
  return PLVS_OK;
}

}  // namespace bowsearch
}  // namespace plvs
