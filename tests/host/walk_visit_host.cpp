// The two visit words of the depth-image lean walk (plvs_amd/csrc/tsdf_walk_visit.hpp) replayed on a CPU: what a tile's
// rays add into an entry unpacks to the sums kept separately.  tests/test_walk_visit_words.py compiles and runs this.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../plvs_amd/csrc/tsdf_walk_visit.hpp"

using namespace plvs::tsdf;

constexpr int kRays = 512;   // kWalkRays of tsdf_walk.hpp
static_assert(visit_words_hold<kRays>(), "count and ray sum of a whole tile fit the count word");
static_assert(!visit_words_hold<1024>(), "1024 rays would not: the count needs an eleventh bit");
static_assert(kVisitCountBits == 10, "the packing the kernels' comments state");

static int fails = 0;
#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);             \
      ++fails;                                                       \
    }                                                                \
  } while (0)

struct Entry {   // the LDS words of one table entry: plain adds, as ds_add_u64 / ds_add_u32 do them
  unsigned long long sums = 0;
  uint32_t count = 0;
  void visit(uint32_t ray, int32_t wuu, uint32_t q_w) {
    sums += visit_sums_word(wuu, q_w);
    count += visit_count_word(ray);
  }
};

int main() {
  // every single ray: (1, ray)
  for (uint32_t r = 0; r < (uint32_t)kRays; ++r) {
    Entry e;
    e.visit(r, -7, 3u);
    CHECK(visit_count(e.count) == 1u && visit_ray_sum(e.count) == r);
    CHECK(visit_sum_wuu(e.sums) == (uint32_t)-7 && visit_sum_w(e.sums) == 3u);
  }
  std::printf("single rays ok\n");
  // all rays together: (512, 130 816), with the largest weight a whole tile may carry and the extremes of w * u
  {
    const uint32_t q_max = 0x7FFFFFFFu / (uint32_t)kRays;   // sum of q_w stays below 2^31 (how scale_w is chosen)
    Entry e;
    uint32_t wuu_sum = 0;
    unsigned long long w_sum = 0;
    for (uint32_t r = 0; r < (uint32_t)kRays; ++r) {
      const int32_t wuu = (r & 1u) ? INT32_MIN : INT32_MAX;
      e.visit(r, wuu, q_max);
      wuu_sum += (uint32_t)wuu;
      w_sum += q_max;
    }
    CHECK(visit_count(e.count) == (uint32_t)kRays && visit_ray_sum(e.count) == 130816u);
    CHECK(w_sum < (1ull << 31) && visit_sum_w(e.sums) == (uint32_t)w_sum && visit_sum_wuu(e.sums) == wuu_sum);
    std::printf("all rays ok: count %u ray sum %u\n", visit_count(e.count), visit_ray_sum(e.count));
  }
  // seeded random subsets, in random order; w * u at the ends of int32 and around zero, weights at their bound; the halves of
  // the 64-bit word never carry into each other: each equals its own 32-bit sum
  std::mt19937 rng(12345u);
  int subsets = 0;
  for (int round = 0; round < 2000; ++round) {
    std::vector<uint32_t> rays(kRays);
    for (uint32_t r = 0; r < (uint32_t)kRays; ++r) rays[r] = r;
    for (int i = kRays - 1; i > 0; --i) std::swap(rays[i], rays[rng() % (uint32_t)(i + 1)]);
    const uint32_t n = 1u + rng() % (uint32_t)kRays;
    const uint32_t q_bound = 0x7FFFFFFFu / n;
    Entry e;
    uint32_t cnt = 0, rsum = 0, wuu_sum = 0;
    unsigned long long w_sum = 0;
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t pick = rng() % 6u;
      const int32_t wuu = pick == 0 ? INT32_MAX : pick == 1 ? INT32_MIN : pick == 2 ? -1 : pick == 3 ? 0 : (int32_t)rng();
      const uint32_t q_w = (rng() & 1u) ? q_bound : rng() % (q_bound + 1u);
      e.visit(rays[i], wuu, q_w);
      ++cnt;
      rsum += rays[i];
      wuu_sum += (uint32_t)wuu;
      w_sum += q_w;
    }
    CHECK(w_sum < (1ull << 31));
    CHECK(visit_count(e.count) == cnt && visit_ray_sum(e.count) == rsum);
    CHECK(visit_sum_w(e.sums) == (uint32_t)w_sum);
    CHECK(visit_sum_wuu(e.sums) == wuu_sum);
    if (cnt == 1u) CHECK(visit_ray_sum(e.count) == rays[0]);
    ++subsets;
  }
  std::printf("random subsets ok: %d\n", subsets);
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
