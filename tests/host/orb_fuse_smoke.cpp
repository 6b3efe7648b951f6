// ORBmatcher::FuseSearch of include/plvs_hip.hpp against nothing but the C ABI.  Reads the binary file of
// tests/host/fuse_pair_host.cpp (tests/test_orb_fuse.py writes it) and prints best_idx, best_dist and reached of every pair:
//   orb_fuse_smoke <input file> host      plvs_hip_orb_fuse_search_host: no device call
//   orb_fuse_smoke <input file> device    plvs_hip_orb_fuse_search
// After the search it asks for a two-camera key frame and for a fisheye one, which both entries refuse before anything is launched.
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
  float h[24];
  std::vector<float> x, y, ur, sf, sig;
  std::vector<int32_t> octave;
  std::vector<uint8_t> desc;
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s <input file> host|device\n", argv[0]);
    return 2;
  }
  const bool on_host = std::string(argv[2]) == "host";
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  int32_t K = 0, M = 0;
  float th = 0;
  if (!read_exact(f, &K, 4) || !read_exact(f, &M, 4) || !read_exact(f, &th, 4) || K < 0 || K > 64 || M < 0 || M > (1 << 16)) return 3;
  std::vector<Kf> store((size_t)K);
  std::vector<plvs_fuse_keyframe> kfs((size_t)K);
  for (int k = 0; k < K; ++k) {
    Kf& s = store[k];
    int32_t levels = 0, N = 0;
    if (!read_exact(f, s.h, sizeof s.h) || !read_exact(f, &levels, 4) || !read_exact(f, &N, 4) || levels < 1 || levels > 64 || N < 0 || N > (1 << 20)) return 3;
    if (!read_vec(f, s.x, N) || !read_vec(f, s.y, N) || !read_vec(f, s.octave, N) || !read_vec(f, s.ur, N) || !read_vec(f, s.desc, 32 * (size_t)N) ||
        !read_vec(f, s.sf, levels) || !read_vec(f, s.sig, levels))
      return 3;
    plvs_fuse_keyframe& kf = kfs[k];
    std::memset(&kf, 0, sizeof kf);
    kf.view.n = N;
    kf.view.x = s.x.data(); kf.view.y = s.y.data(); kf.view.octave = s.octave.data(); kf.view.u_right = s.ur.data(); kf.view.desc = s.desc.data();
    kf.view.min_x = s.h[19]; kf.view.min_y = s.h[20]; kf.view.grid_w_inv = s.h[21]; kf.view.grid_h_inv = s.h[22];
    kf.view.scale_factors = s.sf.data();
    kf.inv_level_sigma2 = s.sig.data();
    kf.n_levels = levels;
    kf.log_scale_factor = s.h[23];
    kf.n_cameras = 1;
    kf.camera_model = PLVS_CAMERA_PINHOLE;
    kf.q_cw = s.h; kf.tcw = s.h + 4; kf.Ow = s.h + 7; kf.K4 = s.h + 10; kf.mbf = s.h[14]; kf.bounds4 = s.h + 15;
  }
  std::vector<float> pos, normal, min_dist, max_dist;
  std::vector<uint8_t> desc, skip;
  if (!read_vec(f, pos, 3 * (size_t)M) || !read_vec(f, normal, 3 * (size_t)M) || !read_vec(f, min_dist, M) || !read_vec(f, max_dist, M) ||
      !read_vec(f, desc, 32 * (size_t)M) || !read_vec(f, skip, (size_t)K * M))
    return 3;
  std::fclose(f);
  const plvs_fuse_points P{M, pos.data(), normal.data(), min_dist.data(), max_dist.data(), desc.data()};
  const PLVS2hip::ORBmatcher matcher;
  PLVS2hip::ORBmatcher::FuseResult res;
  const int found = matcher.FuseSearch(kfs, P, skip.data(), th, res, on_host);
  for (size_t p = 0; p < res.bestIdx.size(); ++p) std::printf("pair %d %d %d\n", res.bestIdx[p], res.bestDist[p], (int)res.reached[p]);
  std::printf("found %d stats %d %d %d\n", found, res.stats[0], res.stats[1], res.stats[2]);
  int refused = 0;
  for (int what = 0; what < 2 && K > 0; ++what) {
    std::vector<plvs_fuse_keyframe> bad = kfs;
    if (what == 0) bad.back().n_cameras = 2;
    else bad.back().camera_model = PLVS_CAMERA_PINHOLE + 1;
    try {
      matcher.FuseSearch(bad, P, skip.data(), th, res, on_host);
    } catch (const std::runtime_error&) {
      ++refused;
    }
  }
  std::printf("refused %d\n", refused);
  std::printf("orb_fuse_smoke ok\n");
  return 0;
}
