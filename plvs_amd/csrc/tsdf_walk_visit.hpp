// The two LDS words a visit adds to in the depth-image instances of the lean walk (tsdf_walk.hpp: walk_lean<.., kVisitWords>,
// walk_fast_tile<E, true>).  Plain C++17 — the kernels include it, tests/host/walk_visit_host.cpp compiles it with a host
// compiler and replays the packing on a CPU.
//
// All rays of such a tile belong to one image, and the key-frame id of a voxel is its image's: which ray of the tile came
// last decides nothing, so a visit keeps no last-visitor maximum.  It issues two atomics on its voxel's entry:
//   sums  (64 bits, one ds_add_u64)  += ((int64)wuu << 32) + q_w
//           low word : sum of q_w, the fixed-point weight.  scale_w keeps the sum over a whole call below 2^31, so it never
//                      carries into the high word
//           high word: sum of wuu = w * u in fixed point, modulo 2^32 — the int32 sum the records have always carried
//   count (32 bits, one ds_add_u32)  += (ray << kVisitCountBits) | 1
//           bits 0 .. kVisitCountBits-1 : visits (a ray visits a voxel at most once: at most kRays)
//           above                       : sum of the visiting rays' indices — THE ray where the count is 1, which is all the
//                                         one-ray shortcut of the flush asks for
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define PLVS_VISIT_FN __host__ __device__ __forceinline__
#else
#define PLVS_VISIT_FN inline
#endif

namespace plvs {
namespace tsdf {

constexpr int kVisitCountBits = 10;
constexpr uint32_t kVisitCountMask = (1u << kVisitCountBits) - 1u;

// The count word holds every ray of a tile of kRays rays at once: the count, and above it the sum 0 + 1 + ... + kRays-1.
template <int kRays>
constexpr bool visit_words_hold() {
  return (uint64_t)kRays <= (uint64_t)kVisitCountMask &&
         ((uint64_t)kRays * (uint64_t)(kRays - 1) / 2) < (1ull << (32 - kVisitCountBits));
}

PLVS_VISIT_FN unsigned long long visit_sums_word(int32_t wuu, uint32_t q_w) {
  return ((unsigned long long)(long long)wuu << 32) + (unsigned long long)q_w;
}
PLVS_VISIT_FN uint32_t visit_count_word(uint32_t ray) { return (ray << kVisitCountBits) | 1u; }

PLVS_VISIT_FN uint32_t visit_sum_wuu(unsigned long long sums) { return (uint32_t)(sums >> 32); }   // (the bits of an int32)
PLVS_VISIT_FN uint32_t visit_sum_w(unsigned long long sums) { return (uint32_t)sums; }
PLVS_VISIT_FN uint32_t visit_count(uint32_t word) { return word & kVisitCountMask; }
PLVS_VISIT_FN uint32_t visit_ray_sum(uint32_t word) { return word >> kVisitCountBits; }

}  // namespace tsdf
}  // namespace plvs
