// plvs_amd/csrc/loop_search_pair.hpp with fuse_pair.hpp and line_fuse_pair.hpp compiled for the host, stand-alone: the greedy pass,
// the cut, the projection policy, the band gate and the exclusion — the text the kernels and the library's loop-search entries share.
//   loop_search_pair_host points|lines|lists <input file> <extra file>
// <input file>: the binary file of tests/host/fuse_pair_host.cpp (points, lists) or line_fuse_pair_host.cpp (lines), as
// tests/test_orb_fuse.py / tests/test_line_fuse.py write them; the pose in it is the caller's decomposition of Scw, Ow the kind's own.
// <extra file>: float ratio_hamming, int32 projection, then per key frame int32 n (-1: occupied[k] is NULL) and n bytes.
// points, lines: every pair by the host's code in the greedy pass (the host twins' path).  lists: the points once more with each
// pair's list built here, serially, as the kernel posts it (the kListLen smallest (distance, position) at or below the cut, the
// count, the flags), so that the greedy pass reads lists and recomputes only a truncated, wholly claimed one — the device entry's path.
// Prints match_idx, match_dist and reached of every pair and `nmatches k n` per key frame; tests/test_loop_search.py holds them
// against the reference's recorded run.
#include <cmath>
#include <cstdint>
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "../../plvs_amd/csrc/loop_search_pair.hpp"

namespace {

namespace fp = plvs::fusepair;
namespace lf = plvs::linefuse;
namespace ls = plvs::loopsearch;
struct Member { float x, y; int octave, idx; };

struct Extra {
  float ratio = 0;
  int32_t projection = 0;
  std::vector<std::vector<uint8_t>> occupied;   // per key frame
  std::vector<int> has;
};

bool read_exact(std::FILE* f, void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }
template <typename T>
bool read_vec(std::FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return read_exact(f, v.data(), sizeof(T) * n);
}

// the order-free part of one pair as orb_loop_search.hip posts it, serially (the walk is fuse_pair.hpp's search_window's)
ls::PairList list_of_pair(const fp::KfConst& K, const fp::KfGrid<Member>& G, int projection, const float* pos, const float* normal, float min_dist,
                          float max_dist, const uint8_t* desc, float th, int cut) {
  ls::PairList L{};
  const fp::Front f = projection == fp::kProjectInvz ? fp::front<fp::kProjectInvz>(K, pos, normal, min_dist, max_dist)
                                                    : fp::front<fp::kProjectCamera>(K, pos, normal, min_dist, max_dist);
  L.reached = f.reached;
  if (f.reached != fp::kEmptyWindow) return L;
  L.host = f.ambiguous != 0;
  const float radius = th * G.scale_factors[f.level];
  fp::Cells w;
  if (!fp::window_cells(K, f.u, f.v, radius, &w)) return L;
  uint32_t qd[8], td[8];
  std::memcpy(qd, desc, 32);
  std::vector<std::pair<uint32_t, int>> keys;
  uint32_t position = 0;
  for (int ix = w.c0; ix <= w.c1; ++ix) {
    const int s = G.start[ix * fp::kGridRows + w.r0], e = G.start[ix * fp::kGridRows + w.r1 + 1];
    for (int j = s; j < e; ++j, ++position) {
      const Member& m = G.members[j];
      if (!fp::in_area(m.x, m.y, f.u, f.v, radius)) continue;
      L.any = true;
      if (!fp::candidate_gate<fp::kGateSim3>(f.u, f.v, 0.0f, f.level, m.x, m.y, m.octave, -1.0f, nullptr)) continue;
      L.banded = true;
      std::memcpy(td, G.desc + 32 * (size_t)m.idx, 32);
      const int d = fp::hamming256(qd, td);
      if (d <= cut) keys.push_back({((uint32_t)d << 23) | position, m.idx});
    }
  }
  std::sort(keys.begin(), keys.end());
  L.count = (int)keys.size();
  L.n = L.count < ls::kListLen ? L.count : ls::kListLen;
  for (int r = 0; r < L.n; ++r) { L.idx[r] = keys[r].second; L.dist[r] = (int)(keys[r].first >> 23); }
  return L;
}

void seed(const Extra& X, int k, size_t n, std::vector<uint8_t>* claimed) {
  claimed->assign(n, 0);
  if (X.has[k])
    for (size_t j = 0; j < n && j < X.occupied[k].size(); ++j) (*claimed)[j] = X.occupied[k][j] != 0;
}

void print_kf(int k, int M, const ls::GreedyCounts& n, const std::vector<int32_t>& idx, const std::vector<int32_t>& dist, const std::vector<uint8_t>& code) {
  for (int i = 0; i < M; ++i) std::printf("pair %d %d %d\n", idx[i], dist[i], (int)code[i]);
  std::printf("nmatches %d %d %d\n", k, n.matches, n.truncated_pairs);
}

int points(std::FILE* f, int K, int M, float th, const Extra& X, bool lists) {
  struct Kf {
    fp::KfConst c;
    std::vector<float> x, y, ur, sf, sig;
    std::vector<int32_t> octave;
    std::vector<uint8_t> desc;
    std::vector<int> start;
    std::vector<Member> members;
  };
  std::vector<Kf> kfs((size_t)K);
  for (Kf& kf : kfs) {
    float h[24];
    int32_t levels = 0, N = 0;
    if (!read_exact(f, h, sizeof h) || !read_exact(f, &levels, 4) || !read_exact(f, &N, 4) || levels < 1 || levels > 64 || N < 0 || N > (1 << 20)) return 3;
    fp::KfConst& c = kf.c;
    for (int i = 0; i < 4; ++i) c.q[i] = h[i];
    for (int i = 0; i < 3; ++i) { c.t[i] = h[4 + i]; c.Ow[i] = h[7 + i]; }
    c.fx = h[10]; c.fy = h[11]; c.cx = h[12]; c.cy = h[13]; c.mbf = h[14];
    c.min_x = h[15]; c.max_x = h[16]; c.min_y = h[17]; c.max_y = h[18];
    c.grid_min_x = h[19]; c.grid_min_y = h[20]; c.grid_w_inv = h[21]; c.grid_h_inv = h[22];
    c.log_scale_factor = h[23];
    c.n_levels = levels;
    if (!read_vec(f, kf.x, N) || !read_vec(f, kf.y, N) || !read_vec(f, kf.octave, N) || !read_vec(f, kf.ur, N) || !read_vec(f, kf.desc, 32 * (size_t)N) ||
        !read_vec(f, kf.sf, levels) || !read_vec(f, kf.sig, levels))
      return 3;
    // Frame::AssignFeaturesToGrid: cell lists in key point order, laid out column after column
    std::vector<int> cell((size_t)N);
    kf.start.assign(fp::kGridCols * fp::kGridRows + 1, 0);
    for (int i = 0; i < N; ++i) {
      if (kf.octave[i] < 0 || kf.octave[i] >= levels) return 3;
      const int px = (int)std::round((kf.x[i] - c.grid_min_x) * c.grid_w_inv), py = (int)std::round((kf.y[i] - c.grid_min_y) * c.grid_h_inv);
      cell[i] = (px < 0 || px >= fp::kGridCols || py < 0 || py >= fp::kGridRows) ? -1 : px * fp::kGridRows + py;
      if (cell[i] >= 0) ++kf.start[cell[i] + 1];
    }
    for (int k = 0; k < fp::kGridCols * fp::kGridRows; ++k) kf.start[k + 1] += kf.start[k];
    std::vector<int> fill(kf.start.begin(), kf.start.end() - 1);
    kf.members.resize((size_t)N);
    for (int i = 0; i < N; ++i)
      if (cell[i] >= 0) kf.members[fill[cell[i]]++] = Member{kf.x[i], kf.y[i], kf.octave[i], i};
  }
  std::vector<float> pos, normal, min_dist, max_dist;
  std::vector<uint8_t> desc, skip;
  if (!read_vec(f, pos, 3 * (size_t)M) || !read_vec(f, normal, 3 * (size_t)M) || !read_vec(f, min_dist, M) || !read_vec(f, max_dist, M) ||
      !read_vec(f, desc, 32 * (size_t)M) || !read_vec(f, skip, (size_t)K * M))
    return 3;
  int cut = 0;
  if (ls::threshold_cut(ls::kPointThLow, X.ratio, &cut) != ls::kCutOk) return 4;
  std::vector<uint8_t> claimed, code((size_t)M);
  std::vector<int32_t> idx((size_t)M), dist((size_t)M);
  for (int k = 0; k < K; ++k) {
    const Kf& kf = kfs[k];
    const fp::KfGrid<Member> G{kf.start.data(), kf.members.data(), kf.ur.data(), kf.desc.data(), kf.sf.data(), kf.sig.data()};
    seed(X, k, kf.x.size(), &claimed);
    const uint8_t* sk = skip.data() + (size_t)k * M;
    const ls::GreedyCounts n = ls::greedy_keyframe(
        M, ls::point_codes(),
        [&](int i) {
          ls::PairList L{};
          L.reached = fp::kSkipped;
          if (sk[i]) return L;
          if (!lists) { L.host = true; return L; }
          return list_of_pair(kf.c, G, X.projection, pos.data() + 3 * (size_t)i, normal.data() + 3 * (size_t)i, min_dist[i], max_dist[i],
                              desc.data() + 32 * (size_t)i, th, cut);
        },
        [&](int i, const uint8_t* c) {
          return ls::point_pair_host(kf.c, G, X.projection, pos.data() + 3 * (size_t)i, normal.data() + 3 * (size_t)i, min_dist[i], max_dist[i],
                                     desc.data() + 32 * (size_t)i, th, cut, c, 0);
        },
        claimed.data(), idx.data(), dist.data(), code.data());
    print_kf(k, M, n, idx, dist, code);
  }
  return 0;
}

int lines(std::FILE* f, int K, int M, float th, const Extra& X) {
  struct Kf {
    lf::KfConst c;
    std::vector<float> segs, urs, ure, sf, sig;
    std::vector<int32_t> octave;
    std::vector<uint8_t> desc;
    lf::Grid grid;
  };
  std::vector<Kf> kfs((size_t)K);
  for (Kf& kf : kfs) {
    float h[26];   // Rcw9, t3, Ow3, K4, mbf, bounds4, max_diag, log scale factor
    int32_t levels = 0, N = 0, has_right = 0;
    if (!read_exact(f, h, sizeof h) || !read_exact(f, &levels, 4) || !read_exact(f, &N, 4) || !read_exact(f, &has_right, 4) || levels < 1 ||
        levels > 64 || N < 0 || N > (1 << 20) || !(h[24] > 0.0f))
      return 3;
    lf::KfConst& c = kf.c;
    for (int i = 0; i < 9; ++i) c.R[i] = h[i];
    for (int i = 0; i < 3; ++i) { c.t[i] = h[9 + i]; c.Ow[i] = h[12 + i]; }
    c.fx = h[15]; c.fy = h[16]; c.cx = h[17]; c.cy = h[18]; c.mbf = h[19];
    c.min_x = h[20]; c.max_x = h[21]; c.min_y = h[22]; c.max_y = h[23];
    const float max_diag = h[24];
    c.diag = (float)(int)max_diag;
    c.theta_inv = (float)lf::kRows / (float)lf::kPi;
    c.d_inv = (float)lf::kCols / (2.0f * max_diag);
    c.log_scale_factor = h[25];
    c.n_levels = levels;
    if (!read_vec(f, kf.segs, 4 * (size_t)N) || !read_vec(f, kf.octave, N)) return 3;
    if (has_right && (!read_vec(f, kf.urs, N) || !read_vec(f, kf.ure, N))) return 3;
    if (!read_vec(f, kf.desc, 32 * (size_t)N) || !read_vec(f, kf.sf, levels) || !read_vec(f, kf.sig, levels)) return 3;
    for (int i = 0; i < N; ++i)
      if (kf.octave[i] < 0 || kf.octave[i] >= levels) return 3;
    const Kf* self = &kf;
    lf::build_grid(N, [self](int i) { return lf::KeyLineIn{self->segs[4 * (size_t)i], self->segs[4 * (size_t)i + 1], self->segs[4 * (size_t)i + 2],
                                                           self->segs[4 * (size_t)i + 3], self->octave[i]}; },
                   has_right ? kf.urs.data() : nullptr, has_right ? kf.ure.data() : nullptr, max_diag, c.theta_inv, c.d_inv, 0, &kf.grid);
  }
  std::vector<float> start, end, normal, max_dist;
  std::vector<uint8_t> desc, skip;
  if (!read_vec(f, start, 3 * (size_t)M) || !read_vec(f, end, 3 * (size_t)M) || !read_vec(f, normal, 3 * (size_t)M) || !read_vec(f, max_dist, M) ||
      !read_vec(f, desc, 32 * (size_t)M) || !read_vec(f, skip, (size_t)K * M))
    return 3;
  int cut = 0;
  if (ls::threshold_cut(ls::kLineThLow, X.ratio, &cut) != ls::kCutOk) return 4;
  std::vector<uint8_t> claimed, code((size_t)M);
  std::vector<int32_t> idx((size_t)M), dist((size_t)M);
  for (int k = 0; k < K; ++k) {
    const Kf& kf = kfs[k];
    const lf::KfGrid G{kf.grid.start.data(), kf.grid.members.data(), kf.desc.data(), kf.sf.data(), kf.sig.data()};
    seed(X, k, kf.octave.size(), &claimed);
    const uint8_t* sk = skip.data() + (size_t)k * M;
    const ls::GreedyCounts n = ls::greedy_keyframe(
        M, ls::line_codes(),
        [&](int i) {
          ls::PairList L{};
          L.reached = lf::kSkipped;
          L.host = !sk[i];
          return L;
        },
        [&](int i, const uint8_t* c) {
          return ls::line_pair_host(kf.c, G, start.data() + 3 * (size_t)i, end.data() + 3 * (size_t)i, normal.data() + 3 * (size_t)i, max_dist[i],
                                    desc.data() + 32 * (size_t)i, th, cut, c, 0, 0);
        },
        claimed.data(), idx.data(), dist.data(), code.data());
    print_kf(k, M, n, idx, dist, code);
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: %s points|lines|lists <input file> <extra file>\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[2], "rb");
  if (!f) {
    std::perror(argv[2]);
    return 2;
  }
  int32_t K = 0, M = 0;
  float th = 0;
  if (!read_exact(f, &K, 4) || !read_exact(f, &M, 4) || !read_exact(f, &th, 4) || K < 0 || K > 64 || M < 0 || M > (1 << 16)) return 3;
  Extra X;
  std::FILE* x = std::fopen(argv[3], "rb");
  if (!x) {
    std::perror(argv[3]);
    return 2;
  }
  if (!read_exact(x, &X.ratio, 4) || !read_exact(x, &X.projection, 4)) return 3;
  X.occupied.resize((size_t)K);
  X.has.assign((size_t)K, 0);
  for (int k = 0; k < K; ++k) {
    int32_t n = 0;
    if (!read_exact(x, &n, 4) || n < -1 || n > (1 << 20)) return 3;
    X.has[k] = n >= 0;
    if (n > 0 && !read_vec(x, X.occupied[k], (size_t)n)) return 3;
  }
  std::fclose(x);
  const std::string mode = argv[1];
  const int rc = mode == "lines" ? lines(f, K, M, th, X) : points(f, K, M, th, X, mode == "lists");
  std::fclose(f);
  if (rc) return rc;
  std::printf("loop_search_pair ok\n");
  return 0;
}
