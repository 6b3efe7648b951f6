// plvs_amd/csrc/fuse_pair.hpp and line_fuse_pair.hpp compiled for the host, stand-alone, with the gate policy of the Sim3 Fuse
// overloads (kGateSim3): the text the kernels and the library's _loop_ host entries share.
//   loop_fuse_pair_host points <input file>    the binary file of tests/host/fuse_pair_host.cpp (tests/test_orb_fuse.py writes it)
//   loop_fuse_pair_host lines <input file>     the binary file of tests/host/line_fuse_pair_host.cpp (tests/test_line_fuse.py)
// The pose in the file is the caller's decomposition of Scw; Ow is the kind's own (Ow_points / Ow_lines).  Prints best_idx, best_dist
// and reached of every pair; tests/test_loop_fuse.py holds them against the reference's recorded run.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../plvs_amd/csrc/fuse_pair.hpp"
#include "../../plvs_amd/csrc/line_fuse_pair.hpp"

namespace {

namespace fp = plvs::fusepair;
namespace lf = plvs::linefuse;
struct Member { float x, y; int octave, idx; };

bool read_exact(std::FILE* f, void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }
template <typename T>
bool read_vec(std::FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return read_exact(f, v.data(), sizeof(T) * n);
}

int points(std::FILE* f, int K, int M, float th) {
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
  for (int k = 0; k < K; ++k) {
    const Kf& kf = kfs[k];
    const fp::KfGrid<Member> G{kf.start.data(), kf.members.data(), kf.ur.data(), kf.desc.data(), kf.sf.data(), kf.sig.data()};
    for (int i = 0; i < M; ++i) {
      fp::Result r{-1, -1, fp::kSkipped};
      if (!skip[(size_t)k * M + i])
        r = fp::pair_host<fp::kGateSim3>(kf.c, G, pos.data() + 3 * (size_t)i, normal.data() + 3 * (size_t)i, min_dist[i], max_dist[i],
                                         desc.data() + 32 * (size_t)i, th, 0);
      std::printf("pair %d %d %d\n", r.best_idx, r.best_dist, r.reached);
    }
  }
  return 0;
}

int lines(std::FILE* f, int K, int M, float th) {
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
  for (int k = 0; k < K; ++k) {
    const Kf& kf = kfs[k];
    const lf::KfGrid G{kf.grid.start.data(), kf.grid.members.data(), kf.desc.data(), kf.sf.data(), kf.sig.data()};
    for (int i = 0; i < M; ++i) {
      lf::Result r{-1, -1, lf::kSkipped};
      if (!skip[(size_t)k * M + i])
        r = lf::pair_host(kf.c, G, start.data() + 3 * (size_t)i, end.data() + 3 * (size_t)i, normal.data() + 3 * (size_t)i, max_dist[i],
                          desc.data() + 32 * (size_t)i, th, 0, 0, lf::kGateSim3);
      std::printf("pair %d %d %d\n", r.best_idx, r.best_dist, r.reached);
    }
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s points|lines <input file>\n", argv[0]);
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
  const int rc = std::string(argv[1]) == "points" ? points(f, K, M, th) : lines(f, K, M, th);
  std::fclose(f);
  if (rc) return rc;
  std::printf("loop_fuse_pair ok\n");
  return 0;
}
