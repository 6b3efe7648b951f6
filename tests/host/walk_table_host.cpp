// Host replay of the walk's LDS voxel table (plvs_amd/csrc/tsdf_walk_table.hpp, tsdf_walk.hpp: table_find_or_insert): the
// home bucket and the wrap of a table whose bucket count is not a power of two, and the probing of realistic tile key sets
// up to the table's entry limit.  A program of its own: prints one line per key set, exits 1 at the first failure.
// Test infrastructure only (tests/test_walk_table_buckets.py builds and runs it).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../plvs_amd/csrc/tsdf_walk_table.hpp"

using namespace plvs::tsdf;

namespace {

constexpr uint32_t kKeyEmpty = 0xFFFFFFFFu;

[[noreturn]] void fail(const char* what, long long a = 0, long long b = 0) {
  std::printf("FAIL %s (%lld, %lld)\n", what, a, b);
  std::exit(1);
}

// table_find_or_insert, one key after the other: the buckets looked at (1 = the home bucket held the key or a free slot),
// 0 when the search gave up at the cap.
template <int kBuckets>
int find_or_insert(std::vector<uint32_t>& ekey, uint32_t tkey) {
  uint32_t b = home_bucket<kBuckets>(tkey);
  for (int probe = 0; probe < kTableProbeCap; ++probe) {
    for (int j = 0; j < 4; ++j)
      if (ekey[4 * b + j] == tkey) return probe + 1;
    for (int j = 0; j < 4; ++j)
      if (ekey[4 * b + j] == kKeyEmpty) {
        ekey[4 * b + j] = tkey;
        return probe + 1;
      }
    b = next_bucket<kBuckets>(b);
  }
  return 0;
}

struct Vox {
  int x, y, z;
};

// ---- the voxels of a tile, relative to its key origin (before the set is moved to `at`)
// a wall patch perpendicular to `axis`, `thick` voxels deep, w x h across
std::vector<Vox> slab(int axis, int w, int h, int thick) {
  std::vector<Vox> v;
  for (int c = 0; c < thick; ++c)
    for (int b = 0; b < h; ++b)
      for (int a = 0; a < w; ++a) v.push_back(axis == 0 ? Vox{c, a, b} : axis == 1 ? Vox{a, c, b} : Vox{a, b, c});
  return v;
}
// the voxels of a 48^3 box within `thick` (in units of |n|) above the plane n . p = d0: a receding wall
std::vector<Vox> oblique(int nx, int ny, int nz, int d0, int thick) {
  std::vector<Vox> v;
  const int len2 = nx * nx + ny * ny + nz * nz;
  for (int z = 0; z < 48; ++z)
    for (int y = 0; y < 48; ++y)
      for (int x = 0; x < 48; ++x) {
        const long long d = (long long)nx * x + (long long)ny * y + (long long)nz * z - d0;
        if (d >= 0 && d * d < (long long)thick * thick * len2) v.push_back(Vox{x, y, z});
      }
  return v;
}
std::vector<Vox> box(int w, int h, int d) {
  std::vector<Vox> v;
  for (int z = 0; z < d; ++z)
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) v.push_back(Vox{x, y, z});
  return v;
}

struct Lcg {   // (the order in which the lanes of a tile reach the table is not the scan order of its voxels)
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
};

// The first `entries` voxels of the set at origin `at`, inserted in scan order and in a shuffled order: every key must
// find its place below the cap, and must be found again where it was put.  Returns the longest search.
template <int kBuckets>
int replay(const char* name, const std::vector<Vox>& set, Vox at, int entries) {
  if ((int)set.size() < entries) fail("a key set is smaller than the entry limit", (long long)set.size(), entries);
  std::vector<uint32_t> keys;
  for (int i = 0; i < entries; ++i) {
    const int x = set[i].x + at.x, y = set[i].y + at.y, z = set[i].z + at.z;
    if (x < 0 || y < 0 || z < 0 || x > 1023 || y > 1023 || z > 1023) fail("a voxel outside the 1024^3 key box", i);
    const uint32_t key = (uint32_t)x | ((uint32_t)y << 10) | ((uint32_t)z << 20);
    const uint32_t tkey = key * kTableKeyMul;
    if (tkey == kKeyEmpty) fail("a voxel key maps to the empty key", key);
    if (tkey * kTableKeyMulInv != key) fail("the table key does not invert", key);
    if (home_bucket<kBuckets>(tkey) >= (uint32_t)kBuckets) fail("home bucket out of range", tkey);
    keys.push_back(tkey);
  }
  int worst = 0;
  for (int order = 0; order < 3; ++order) {
    if (order > 0) {
      Lcg r{(uint64_t)(1000 * order + entries)};
      for (size_t i = keys.size(); i > 1; --i) std::swap(keys[i - 1], keys[r.next() % i]);
    }
    std::vector<uint32_t> ekey(4 * (size_t)kBuckets, kKeyEmpty);
    for (uint32_t k : keys) {
      const int p = find_or_insert<kBuckets>(ekey, k);
      if (p == 0) fail("an insertion reached the probe cap", kBuckets, entries);
      worst = std::max(worst, p);
    }
    size_t used = 0;
    for (uint32_t k : ekey) used += k != kKeyEmpty;
    if (used != keys.size()) fail("entries in use differ from the keys inserted", (long long)used, (long long)keys.size());
    for (uint32_t k : keys) {   // (a second visit of the voxel: found, nothing inserted)
      const int p = find_or_insert<kBuckets>(ekey, k);
      if (p == 0) fail("a key in the table was not found below the cap", kBuckets, entries);
    }
    used = 0;
    for (uint32_t k : ekey) used += k != kKeyEmpty;
    if (used != keys.size()) fail("a second visit inserted a key again", (long long)used, (long long)keys.size());
  }
  std::printf("buckets %d entries %d set %s at %d,%d,%d longest_search %d\n", kBuckets, entries, name, at.x, at.y, at.z, worst);
  return worst;
}

template <int kBuckets>
void check_index_functions() {
  // every table key maps into [0, kBuckets), in non-decreasing order of the key, every bucket taken
  std::vector<uint32_t> hits((size_t)kBuckets, 0u);
  uint32_t last = 0;
  for (uint64_t k = 0; k <= 0xFFFFFFFFull; k += 4093) {
    const uint32_t b = home_bucket<kBuckets>((uint32_t)k);
    if (b >= (uint32_t)kBuckets) fail("home bucket out of range", (long long)k, b);
    if (b < last) fail("home buckets are not monotone in the key", (long long)k, b);
    last = b;
    ++hits[b];
  }
  const uint32_t edge[] = {0u, 1u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu};
  for (uint32_t k : edge)
    if (home_bucket<kBuckets>(k) >= (uint32_t)kBuckets) fail("home bucket out of range", k);
  if (home_bucket<kBuckets>(0u) != 0u || home_bucket<kBuckets>(0xFFFFFFFFu) != (uint32_t)kBuckets - 1u) fail("end buckets");
  const uint32_t lo = *std::min_element(hits.begin(), hits.end()), hi = *std::max_element(hits.begin(), hits.end());
  if (lo == 0u || hi - lo > 1u) fail("the buckets do not take equal ranges of keys", lo, hi);
  // the wrap: from any bucket, kBuckets steps visit every bucket once and come back
  for (int b0 = 0; b0 < kBuckets; ++b0) {
    std::vector<uint8_t> seen((size_t)kBuckets, 0);
    uint32_t b = (uint32_t)b0;
    for (int i = 0; i < kBuckets; ++i) {
      if (b >= (uint32_t)kBuckets) fail("next bucket out of range", b0, b);
      if (seen[b]) fail("the wrap visits a bucket twice", b0, b);
      seen[b] = 1;
      b = next_bucket<kBuckets>(b);
    }
    if (b != (uint32_t)b0) fail("the wrap does not close", b0, b);
  }
  std::printf("buckets %d index functions ok\n", kBuckets);
}

// The key sets of one table: `entries` = its entry limit (7/8 of its slots).
template <int kBuckets>
void check_table(int entries) {
  check_index_functions<kBuckets>();
  const Vox origins[] = {{0, 0, 0}, {500, 500, 500}, {975, 30, 511}, {37, 975, 3}, {512, 0, 975}};
  for (const Vox& at : origins) {
    // (a 32 x 16 pixel tile on a frontal wall: ~28 x 16 voxels across, as deep as the truncation band)
    replay<kBuckets>("slab_x", slab(0, 28, 16, 4), at, entries);
    replay<kBuckets>("slab_y", slab(1, 28, 16, 4), at, entries);
    replay<kBuckets>("slab_z", slab(2, 28, 16, 4), at, entries);
    replay<kBuckets>("slab_z_thin", slab(2, 48, 40, 1), at, entries);
    replay<kBuckets>("oblique_123", oblique(1, 2, 3, 60, 2), at, entries);
    replay<kBuckets>("oblique_2m11", oblique(2, -1, 1, 10, 2), at, entries);
    replay<kBuckets>("oblique_5m27", oblique(5, -2, 7, 100, 3), at, entries);
    replay<kBuckets>("box_12x12x9", box(12, 12, 9), at, std::min(entries, 12 * 12 * 9));
    // (and sets well below the limit: the ordinary tile)
    replay<kBuckets>("slab_z_half", slab(2, 28, 16, 3), at, entries / 2);
  }
}

}  // namespace

int main() {
  check_table<384>(1536 * 7 / 8);   // the small table of the lean walk: 1344 entries
  check_table<256>(1024 * 7 / 8);   // ... and the power-of-two table of the same load it replaced: 896 entries
  check_table<512>(2048 * 7 / 8);
  std::printf("ok\n");
  return 0;
}
