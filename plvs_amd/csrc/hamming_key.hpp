// The composite key of the exact k = 2 Hamming search (hamming.hip describes its fields) and the two steps every search
// built on it takes: keep the two smallest keys a lane has seen, merge the 64 sorted pairs of a wave.  Shared by
// hamming_knn2_kernel (hamming.hip) and the stereo line matcher (frame_stereo.hip): one statement of the reference's
// multi-index-hash discovery order.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace plvs {

constexpr unsigned long long kNoKey = ~0ull;

// x = query ^ train, eight dwords; t = train index.  kMih: the three tie fields of Mihasher(256, 32) are filled, otherwise
// they are zero ("lowest train index wins").
template <bool kMih>
__device__ __forceinline__ unsigned long long hamming_key(const uint32_t (&x)[8], int t) {
  if constexpr (kMih) {
    uint32_t d = 0, s = 9, k = 0, pat = 0;
#pragma unroll
    for (int w = 0; w < 8; ++w) {
      // per-byte popcounts of x[w]
      uint32_t c = x[w] - ((x[w] >> 1) & 0x55555555u);
      c = (c & 0x33333333u) + ((c >> 2) & 0x33333333u);
      c = (c + (c >> 4)) & 0x0f0f0f0fu;
      d += (c * 0x01010101u) >> 24;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t cb = (c >> (8 * j)) & 0xffu;
        if (cb < s) {  // strict: the first byte reaching the minimum wins
          s = cb;
          k = (uint32_t)(w * 4 + j);
          pat = (x[w] >> (8 * j)) & 0xffu;
        }
      }
    }
    return ((unsigned long long)d << 48) | ((unsigned long long)s << 44) | ((unsigned long long)k << 39) |
           ((unsigned long long)pat << 31) | (unsigned long long)(uint32_t)t;
  } else {
    uint32_t d = 0;
#pragma unroll
    for (int w = 0; w < 8; ++w) d += (uint32_t)__popc(x[w]);
    return ((unsigned long long)d << 48) | (unsigned long long)(uint32_t)t;
  }
}

__device__ __forceinline__ int key_index(unsigned long long key) { return (int)(key & 0x7fffffffull); }
__device__ __forceinline__ int key_distance(unsigned long long key) { return (int)(key >> 48); }

__device__ __forceinline__ void insert_key(unsigned long long key, unsigned long long& b1, unsigned long long& b2) {
  if (key < b1) {
    b2 = b1;
    b1 = key;
  } else if (key < b2) {
    b2 = key;
  }
}

// Butterfly merge of the 64 sorted pairs of a wave: afterwards every lane holds the wave's two smallest keys.
__device__ __forceinline__ void merge_keys_wave(unsigned long long& b1, unsigned long long& b2) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned long long p1 = __shfl_xor(b1, m, 64);
    const unsigned long long p2 = __shfl_xor(b2, m, 64);
    const unsigned long long lo = b1 < p1 ? b1 : p1;
    const unsigned long long hi = b1 < p1 ? p1 : b1;
    const unsigned long long s2 = b2 < p2 ? b2 : p2;
    b1 = lo;
    b2 = hi < s2 ? hi : s2;
  }
}

}  // namespace plvs
