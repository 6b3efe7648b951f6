// The device side of the greedy searches' order-free part (loop_search_pair.hpp), shared by orb_loop_search.hip and
// line_loop_search.hip: the per-lane sorted list, the cross-lane rounds, the posted record and its reading on the host.
// HIP only.  Internal to the library.
#pragma once
#include <memory>

#include "common.hpp"
#include "loop_search_pair.hpp"

namespace plvs {
namespace loopsearch {

constexpr int kPosBits = 23;   // a key: distance (9 bits) above the enumeration position (the windows' own: fewer than 2^23 members)
constexpr uint32_t kNoKey = 0xffffffffu;
static_assert(kListLen == 4, "the posted record packs four 8-bit distances into one word and four indices into an int4");

// A pair's head: x = count (16 bits, saturating) | entries << 16 | banded << 19 | any << 20 | host << 21 | reached << 24,
// y = the entries' distances, 8 bits each (a distance at or below the cut is below 256).  The entries' indices: an int4 beside it,
// written only when there is an entry.
__host__ __device__ inline uint2 pack_head(int reached, int host, int any, int banded, int n, int count, uint32_t dists) {
  const uint32_t c = count > 0xffff ? 0xffffu : (uint32_t)count;
  return make_uint2(c | ((uint32_t)n << 16) | ((uint32_t)banded << 19) | ((uint32_t)any << 20) | ((uint32_t)host << 21) | ((uint32_t)reached << 24),
                    dists);
}

inline PairList unpack(const uint2& h, const int4& e) {
  PairList L;
  L.reached = (int)(h.x >> 24);
  L.host = ((h.x >> 21) & 1u) != 0;
  L.any = ((h.x >> 20) & 1u) != 0;
  L.banded = ((h.x >> 19) & 1u) != 0;
  L.n = (int)((h.x >> 16) & 7u);
  L.count = (int)(h.x & 0xffffu);
  const int idx[kListLen] = {e.x, e.y, e.z, e.w};
  for (int r = 0; r < kListLen; ++r) {
    L.idx[r] = r < L.n ? idx[r] : -1;
    L.dist[r] = (int)((h.y >> (8 * r)) & 0xffu);
  }
  return L;
}

#if defined(__HIPCC__)
// A lane's kListLen smallest keys with their members' indices, ascending.  Every index below is a constant after unrolling: the
// arrays live in registers.
struct LaneList {
  uint32_t key[kListLen];
  int idx[kListLen];
  int count;   // members this lane saw at or below the cut

  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int r = 0; r < kListLen; ++r) { key[r] = kNoKey; idx[r] = -1; }
    count = 0;
  }
  // the new key sinks to its place, the largest falls off the end
  __device__ __forceinline__ void insert(uint32_t k, int ki) {
    ++count;
#pragma unroll
    for (int r = 0; r < kListLen; ++r) {
      const bool lower = k < key[r];
      const uint32_t tk = key[r];
      const int ti = idx[r];
      key[r] = lower ? k : tk;
      idx[r] = lower ? ki : ti;
      k = lower ? tk : k;
      ki = lower ? ti : ki;
    }
  }
  // kListLen rounds: the wave's smallest head, popped from the lane that owns it (keys are distinct: one owner).  Called by the
  // whole wave; lane 0 posts.  any / banded: this lane's.
  __device__ __forceinline__ void post(int lane, int reached, int host, bool any, bool banded, uint2* __restrict__ head, int4* __restrict__ entries) {
    int total = count;
    for (int off = 32; off > 0; off >>= 1) total += __shfl_xor(total, off);
    const unsigned long long has_any = __ballot(any), has_banded = __ballot(banded);
    int out_idx[kListLen];
    uint32_t dists = 0;
    int n = 0;
#pragma unroll
    for (int r = 0; r < kListLen; ++r) {
      uint32_t lowest = key[0];
      for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)lowest, off);
        lowest = o < lowest ? o : lowest;
      }
      out_idx[r] = -1;
      if (lowest != kNoKey) {   // uniform: every lane holds the wave's minimum
        const unsigned long long owner = __ballot(key[0] == lowest);
        out_idx[r] = __shfl(idx[0], __ffsll((long long)owner) - 1);
        if (key[0] == lowest) {
#pragma unroll
          for (int q = 0; q + 1 < kListLen; ++q) { key[q] = key[q + 1]; idx[q] = idx[q + 1]; }
          key[kListLen - 1] = kNoKey;
          idx[kListLen - 1] = -1;
        }
        dists |= (lowest >> kPosBits) << (8 * r);
        ++n;
      }
    }
    if (lane == 0) {
      *head = pack_head(reached, host, has_any != 0, has_banded != 0, n, total, dists);
      if (n > 0) *entries = make_int4(out_idx[0], out_idx[1], out_idx[2], out_idx[3]);
    }
  }
};
#endif

// What a greedy part holds back until post(): a refusal found in the results (the line side's full theta interval) comes before
// ANY output is written.
struct HeldOutputs {
  int32_t *match_idx = nullptr, *match_dist = nullptr;
  uint8_t* reached = nullptr;
  int32_t* nmatches = nullptr;
  std::unique_ptr<int32_t[]> idx, dist, n;
  std::unique_ptr<uint8_t[]> code;
  size_t pairs = 0;
  int kfs = 0;
  void reserve(size_t n_pairs, int n_kfs) {
    pairs = n_pairs;
    kfs = n_kfs;
    idx.reset(new int32_t[n_pairs]);
    dist.reset(new int32_t[n_pairs]);
    code.reset(new uint8_t[n_pairs]);
    n.reset(new int32_t[(size_t)n_kfs]);
  }
  void write() const {
    for (size_t p = 0; p < pairs; ++p) {
      match_idx[p] = idx[p];
      match_dist[p] = dist[p];
      if (reached) reached[p] = code[p];
    }
    for (int k = 0; nmatches && k < kfs; ++k) nmatches[k] = n[k];
  }
};

}  // namespace loopsearch
}  // namespace plvs
