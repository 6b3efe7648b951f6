// plvs_amd/csrc/line_fuse_pair.hpp compiled for the host, stand-alone: the projection, the tests, the level choice, the (theta, d)
// window and the per-candidate gates the kernel of line_fuse.hip and the library's host entry share.  Reads one binary file
// (tests/test_line_fuse.py writes it from a scenario): int32 K, M; float th; per key frame 26 floats (Rcw9, t3, Ow3, K4, mbf,
// bounds4, max_diag (the Frame's float), log scale factor), int32 n_levels, N, has_right, then segs[4 N], octave[N],
// u_right_start[N], u_right_end[N] (both only if has_right), desc[32 N], scale_factors[n_levels], inv_level_sigma2[n_levels];
// then start[3 M], end[3 M], normal[3 M], max_dist[M], desc[32 M], skip[K M].
// Every pair is evaluated twice: by pair_host (the host entry's path, printed: best_idx, best_dist, reached — the test holds
// them against the reference's recorded run) and by the kernel's rule walked serially (theta from the f64 arctangent, theta_plan,
// the two sub-windows); a pair the rule does not mark ambiguous must give the host's result, or the program fails.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../plvs_amd/csrc/line_fuse_pair.hpp"

namespace {

namespace lf = plvs::linefuse;

bool read_exact(std::FILE* f, void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }
template <typename T>
bool read_vec(std::FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return read_exact(f, v.data(), sizeof(T) * n);
}

// the kernel's walk (line_fuse.hip), one lane: -> the result, *ambiguous = the host decides
lf::Result kernel_rule(const lf::KfConst& K, const lf::KfGrid& G, int n_members, const float* start, const float* end, const float* normal,
                       float max_dist, const uint8_t* desc, float th, int* ambiguous) {
  *ambiguous = 0;
  const lf::Front f = lf::front(K, start, end, normal, max_dist);
  if (f.reached != lf::kEmptyWindow) return lf::Result{-1, -1, f.reached};
  const float scale = G.scale_factors[f.level];
  const float dtheta = (float)(10 * lf::kPi / 180.f) * scale;
  const float dd = th * 100.0f * scale;
  const float theta = lf::theta_device(f.rep);
  const lf::ThetaPlan plan = lf::theta_plan(K, theta, dtheta);
  *ambiguous = (f.ambiguous || plan.nested || lf::theta_ambiguous(K, theta, dtheta, plan)) ? 1 : 0;
  if (*ambiguous) return lf::Result{-1, -1, lf::kEmptyWindow};
  if (plan.full) return lf::Result{-1, -1, lf::kFullTheta};
  if (n_members == 0) return lf::Result{-1, -1, lf::kEmptyWindow};
  uint32_t qd[8];
  std::memcpy(qd, desc, 32);
  const lf::Rep rr = lf::right_rep(K, f);
  const float dmin = f.rep.d - dd, dmax = f.rep.d + dd;
  uint32_t best = 0xffffffffu, pos0 = 0;
  int best_idx = -1;
  bool gated = false;
  for (int s = 0; s < plan.n; ++s) {
    const lf::Cells c = lf::leaf_cells(K, lf::plan_leaf(plan, s, dmin, dmax));
    if (!c.ok) continue;
    for (int ix = c.c0; ix <= c.c1; ++ix) {
      const int a = G.start[ix * lf::kRows + c.r0], e = G.start[ix * lf::kRows + c.r1 + 1];
      for (int j = a; j < e; ++j) {
        const lf::Member& mb = G.members[j];
        if (!lf::candidate_gate(f.rep, rr, f.level, mb, G.inv_level_sigma2)) continue;
        gated = true;
        uint32_t td[8];
        std::memcpy(td, G.desc + 32 * (size_t)mb.idx, 32);
        const uint32_t key = ((uint32_t)lf::hamming256(qd, td) << 23) | (pos0 + (uint32_t)(j - a));
        if (key < best) { best = key; best_idx = mb.idx; }
      }
      if (e > a) pos0 += (uint32_t)(e - a);
    }
  }
  if (pos0 == 0) return lf::Result{-1, -1, lf::kEmptyWindow};
  if (!gated) return lf::Result{-1, -1, lf::kNoCandidate};
  const int d = (int)(best >> 23);
  if (d > lf::kThLow) return lf::Result{-1, -1, lf::kAboveThLow};
  return lf::Result{best_idx, d, lf::kCandidate};
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s <input file>\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  int32_t K = 0, M = 0;
  float th = 0;
  if (!read_exact(f, &K, 4) || !read_exact(f, &M, 4) || !read_exact(f, &th, 4) || K < 0 || K > 64 || M < 0 || M > (1 << 16)) return 3;
  struct Kf {
    lf::KfConst c;
    std::vector<float> segs, urs, ure, sf, sig;
    std::vector<int32_t> octave;
    std::vector<uint8_t> desc;
    lf::Grid grid;
  };
  std::vector<Kf> kfs((size_t)K);
  for (Kf& kf : kfs) {
    // Rcw9, t3, Ow3, K4, mbf, bounds4, max_diag, log scale factor
    float h[26];
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
  std::fclose(f);
  int marked = 0, windows = 0, mismatches = 0;
  for (int k = 0; k < K; ++k) {
    const Kf& kf = kfs[k];
    const lf::KfGrid G{kf.grid.start.data(), kf.grid.members.data(), kf.desc.data(), kf.sf.data(), kf.sig.data()};
    for (int i = 0; i < M; ++i) {
      lf::Result r{-1, -1, lf::kSkipped};
      if (!skip[(size_t)k * M + i]) {
        const float *s = start.data() + 3 * (size_t)i, *e = end.data() + 3 * (size_t)i, *n = normal.data() + 3 * (size_t)i;
        r = lf::pair_host(kf.c, G, s, e, n, max_dist[i], desc.data() + 32 * (size_t)i, th, 0, 0);
        int ambiguous = 0;
        const lf::Result d = kernel_rule(kf.c, G, (int)kf.grid.members.size(), s, e, n, max_dist[i], desc.data() + 32 * (size_t)i, th, &ambiguous);
        marked += ambiguous;
        if (r.reached >= lf::kEmptyWindow) ++windows;
        if (!ambiguous && (d.best_idx != r.best_idx || d.best_dist != r.best_dist || d.reached != r.reached)) {
          std::fprintf(stderr, "pair %d %d: the kernel's rule gives %d %d %d, the host %d %d %d\n", k, i, d.best_idx, d.best_dist, d.reached,
                       r.best_idx, r.best_dist, r.reached);
          ++mismatches;
        }
      }
      std::printf("pair %d %d %d\n", r.best_idx, r.best_dist, r.reached);
    }
  }
  std::printf("marked %d of %d\n", marked, windows);
  if (mismatches) return 4;
  std::printf("line_fuse_pair ok\n");
  return 0;
}
