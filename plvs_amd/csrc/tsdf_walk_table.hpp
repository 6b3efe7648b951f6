// The bucket arithmetic of the walk's LDS voxel tables (tsdf_walk.hpp: table_find_or_insert, table_find, the home-bucket
// probe of walk_lean): where a table key starts its search and which bucket comes next.  Plain C++17 — the kernels include
// it, tests/host/walk_table_host.cpp compiles it with a host compiler and replays the probing on a CPU.
//
// A table of kBuckets buckets of four keys.  A power-of-two table takes the top bits of the table key; any other count
// takes floor(tkey * kBuckets / 2^32) (one v_mul_hi_u32): both map the 32-bit table keys onto [0, kBuckets) in equal
// ranges, so a table of 384 buckets spreads the keys as evenly as one of 256 or 512.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define PLVS_TABLE_FN __host__ __device__ __forceinline__
#else
#define PLVS_TABLE_FN inline
#endif

namespace plvs {
namespace tsdf {

// The table stores a voxel key MULTIPLIED by an odd constant ("table key", a bijection of the 32-bit words).
constexpr uint32_t kTableKeyMul = 2654435761u, kTableKeyMulInv = 0x0E8B2F51u;
static_assert((uint32_t)(kTableKeyMul * kTableKeyMulInv) == 1u, "inverse of the table-key multiplier");
constexpr int kTableProbeCap = 24;   // buckets an insertion looks at before it calls the table full

constexpr bool table_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
constexpr int table_log2(int v) { return v <= 1 ? 0 : 1 + table_log2(v / 2); }

template <int kBuckets>
PLVS_TABLE_FN uint32_t home_bucket(uint32_t tkey) {
  if constexpr (table_pow2(kBuckets)) {
    return tkey >> (32 - table_log2(kBuckets));
  } else {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(tkey, (uint32_t)kBuckets);
#else
    return (uint32_t)(((uint64_t)tkey * (uint64_t)kBuckets) >> 32);
#endif
  }
}

template <int kBuckets>
PLVS_TABLE_FN uint32_t next_bucket(uint32_t b) {
  if constexpr (table_pow2(kBuckets)) {
    return (b + 1u) & (uint32_t)(kBuckets - 1);
  } else {
    return b + 1u == (uint32_t)kBuckets ? 0u : b + 1u;
  }
}

}  // namespace tsdf
}  // namespace plvs
