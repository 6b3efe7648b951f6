// LineMatcher::FuseSearch and FuseSearchPointsAndLines of include/plvs_hip.hpp against nothing but the C ABI.  Reads the binary
// file of tests/host/line_fuse_pair_host.cpp (tests/test_line_fuse.py writes it) and prints best_idx, best_dist and reached of
// every pair:
//   line_fuse_smoke <input file> host      plvs_hip_line_fuse_search_host: no device call
//   line_fuse_smoke <input file> device    plvs_hip_line_fuse_search
//   line_fuse_smoke <input file> both      plvs_hip_fuse_search_points_and_lines with the lines and no points' key frames (an empty
//                                          point set): the lines' results after the call's one wait
// After the search it asks for a two-camera key frame and for a fisheye one, which the entries refuse before anything is launched.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "plvs_hip.hpp"

namespace {

bool read_exact(std::FILE* f, void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }
template <typename T>
bool read_vec(std::FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return read_exact(f, v.data(), sizeof(T) * n);
}
struct Kf {
  float h[26];   // Rcw9, t3, Ow3, K4, mbf, bounds4, max_diag, log scale factor
  std::vector<float> segs, urs, ure, sf, sig;
  std::vector<int32_t> octave;
  std::vector<uint8_t> desc;
  std::vector<plvs_keyline> kl;
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s <input file> host|device|both\n", argv[0]);
    return 2;
  }
  const std::string where = argv[2];
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  int32_t K = 0, M = 0;
  float th = 0;
  if (!read_exact(f, &K, 4) || !read_exact(f, &M, 4) || !read_exact(f, &th, 4) || K < 0 || K > 64 || M < 0 || M > (1 << 16)) return 3;
  std::vector<Kf> store((size_t)K);
  std::vector<plvs_line_fuse_keyframe> kfs((size_t)K);
  for (int k = 0; k < K; ++k) {
    Kf& s = store[k];
    int32_t levels = 0, N = 0, has_right = 0;
    if (!read_exact(f, s.h, sizeof s.h) || !read_exact(f, &levels, 4) || !read_exact(f, &N, 4) || !read_exact(f, &has_right, 4) || levels < 1 ||
        levels > 64 || N < 0 || N > (1 << 20))
      return 3;
    if (!read_vec(f, s.segs, 4 * (size_t)N) || !read_vec(f, s.octave, N)) return 3;
    if (has_right && (!read_vec(f, s.urs, N) || !read_vec(f, s.ure, N))) return 3;
    if (!read_vec(f, s.desc, 32 * (size_t)N) || !read_vec(f, s.sf, levels) || !read_vec(f, s.sig, levels)) return 3;
    s.kl.assign((size_t)N, plvs_keyline());
    for (int i = 0; i < N; ++i) {
      std::memset(&s.kl[i], 0, sizeof(plvs_keyline));
      s.kl[i].startPointX = s.segs[4 * (size_t)i]; s.kl[i].startPointY = s.segs[4 * (size_t)i + 1];
      s.kl[i].endPointX = s.segs[4 * (size_t)i + 2]; s.kl[i].endPointY = s.segs[4 * (size_t)i + 3];
      s.kl[i].octave = s.octave[i];
    }
    plvs_line_fuse_keyframe& kf = kfs[k];
    std::memset(&kf, 0, sizeof kf);
    kf.view.n = N;
    kf.view.keylines_un = s.kl.data();
    kf.view.descriptors = s.desc.data();
    kf.view.u_right_start = has_right ? s.urs.data() : nullptr;
    kf.view.u_right_end = has_right ? s.ure.data() : nullptr;
    kf.view.bf = s.h[19];
    kf.view.n_levels = levels;
    kf.view.line_scale_factors = s.sf.data();
    kf.view.line_inv_level_sigma2 = s.sig.data();
    kf.view.max_diag = s.h[24];
    kf.line_log_scale_factor = s.h[25];
    kf.n_line_levels = levels;
    kf.n_cameras = 1;
    kf.camera_model = PLVS_CAMERA_PINHOLE;
    kf.Rcw = s.h; kf.tcw = s.h + 9; kf.Ow = s.h + 12; kf.K4 = s.h + 15; kf.bounds4 = s.h + 20;
  }
  std::vector<float> start, end, normal, max_dist;
  std::vector<uint8_t> desc, skip;
  if (!read_vec(f, start, 3 * (size_t)M) || !read_vec(f, end, 3 * (size_t)M) || !read_vec(f, normal, 3 * (size_t)M) || !read_vec(f, max_dist, M) ||
      !read_vec(f, desc, 32 * (size_t)M) || !read_vec(f, skip, (size_t)K * M))
    return 3;
  std::fclose(f);
  const plvs_fuse_lines L{M, start.data(), end.data(), normal.data(), max_dist.data(), desc.data()};
  const PLVS2hip::LineMatcher matcher;
  PLVS2hip::LineMatcher::FuseResult res;
  int found = 0;
  int32_t both_stats[2] = {-1, -1};
  if (where == "both") {
    const std::vector<plvs_fuse_keyframe> no_kfs;
    const plvs_fuse_points no_points{0, nullptr, nullptr, nullptr, nullptr, nullptr};
    PLVS2hip::ORBmatcher::FuseResult pres;
    found = PLVS2hip::FuseSearchPointsAndLines(no_kfs, no_points, nullptr, 3.0f, pres, kfs, L, skip.data(), th, res, both_stats);
  } else {
    found = matcher.FuseSearch(kfs, L, skip.data(), th, res, where == "host");
  }
  for (size_t p = 0; p < res.bestIdx.size(); ++p) std::printf("pair %d %d %d\n", res.bestIdx[p], res.bestDist[p], (int)res.reached[p]);
  std::printf("found %d stats %d %d %d both %d %d\n", found, res.stats[0], res.stats[1], res.stats[2], both_stats[0], both_stats[1]);
  int refused = 0;
  for (int what = 0; what < 2 && K > 0; ++what) {
    std::vector<plvs_line_fuse_keyframe> bad = kfs;
    if (what == 0) bad.back().n_cameras = 2;
    else bad.back().camera_model = PLVS_CAMERA_PINHOLE + 1;
    try {
      matcher.FuseSearch(bad, L, skip.data(), th, res, where == "host");
    } catch (const std::runtime_error&) {
      ++refused;
    }
  }
  std::printf("refused %d\n", refused);
  std::printf("line_fuse_smoke ok\n");
  return 0;
}
