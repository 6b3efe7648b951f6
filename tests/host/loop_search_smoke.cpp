// The LoopSearchByProjection overloads of include/plvs_hip.hpp (the loop-closing SearchByProjection(pKF, Scw, ...) over
// KeyFrameHandle) against nothing but the C ABI.  Reads the binary file of tests/host/fuse_pair_host.cpp (tests/test_orb_fuse.py
// writes it; the pose in it is the caller's decomposition of Scw, Ow = Ow_points), creates one handle per key frame, searches with
// PLVS_LOOP_PROJECT_CAMERA, ratio 1.5 and key point `occupied` of key frame 0 marked (-1: none), and prints match_idx, match_dist
// and reached of every pair:
//   loop_search_smoke <input file> host|device <occupied>
// host: host-only handles and the _kf_host entry, no device call.  Then it lists one handle twice with two poses, and asks for what
// the entries refuse.
#include <cstdio>
#include <cstdlib>
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
  if (argc != 4) {
    std::fprintf(stderr, "usage: %s <input file> host|device <occupied>\n", argv[0]);
    return 2;
  }
  const int marked = std::atoi(argv[3]);
  const bool on_host = std::string(argv[2]) == "host";
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  int32_t K = 0, M = 0;
  float th = 0;
  if (!read_exact(f, &K, 4) || !read_exact(f, &M, 4) || !read_exact(f, &th, 4) || K < 1 || K > 64 || M < 0 || M > (1 << 16)) return 3;
  std::vector<Kf> store((size_t)K);
  std::vector<PLVS2hip::KeyFrameHandle> handles;
  std::vector<plvs_keyframe_sim3_pose> poses((size_t)K);
  for (int k = 0; k < K; ++k) {
    Kf& s = store[k];
    int32_t levels = 0, N = 0;
    if (!read_exact(f, s.h, sizeof s.h) || !read_exact(f, &levels, 4) || !read_exact(f, &N, 4) || levels < 1 || levels > 64 || N < 0 || N > (1 << 20)) return 3;
    if (!read_vec(f, s.x, N) || !read_vec(f, s.y, N) || !read_vec(f, s.octave, N) || !read_vec(f, s.ur, N) || !read_vec(f, s.desc, 32 * (size_t)N) ||
        !read_vec(f, s.sf, levels) || !read_vec(f, s.sig, levels))
      return 3;
    plvs_fuse_keyframe kf;
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
    kf.K4 = s.h + 10; kf.mbf = s.h[14]; kf.bounds4 = s.h + 15;   // q_cw, tcw, Ow stay null: the pose is the call's
    plvs_keyframe_sim3_pose& pose = poses[k];
    std::memset(&pose, 0, sizeof pose);   // Rcw, Ow_lines: the line side's, not read by a point search
    std::memcpy(pose.q_cw, s.h, 16); std::memcpy(pose.tcw, s.h + 4, 12); std::memcpy(pose.Ow_points, s.h + 7, 12);
    handles.emplace_back(&kf, nullptr, on_host);
  }
  std::vector<float> pos, normal, min_dist, max_dist;
  std::vector<uint8_t> desc, skip;
  if (!read_vec(f, pos, 3 * (size_t)M) || !read_vec(f, normal, 3 * (size_t)M) || !read_vec(f, min_dist, M) || !read_vec(f, max_dist, M) ||
      !read_vec(f, desc, 32 * (size_t)M) || !read_vec(f, skip, (size_t)K * M))
    return 3;
  std::fclose(f);
  const plvs_fuse_points P{M, pos.data(), normal.data(), min_dist.data(), max_dist.data(), desc.data()};
  std::vector<const PLVS2hip::KeyFrameHandle*> list;
  for (const PLVS2hip::KeyFrameHandle& h : handles) list.push_back(&h);
  std::vector<std::vector<uint8_t>> occupied((size_t)K);   // entries 1 .. K - 1 stay empty: NULL
  if (marked >= 0 && marked < (int)store[0].x.size()) {
    occupied[0].assign(store[0].x.size(), 0);
    occupied[0][(size_t)marked] = 1;
  } else {
    occupied.clear();
  }
  const float ratio = 1.5f;
  PLVS2hip::LoopSearchResult res;
  const int found = PLVS2hip::LoopSearchByProjection(list, poses, P, skip.data(), occupied, th, ratio, PLVS_LOOP_PROJECT_CAMERA, res, on_host);
  for (size_t p = 0; p < res.matchIdx.size(); ++p) std::printf("pair %d %d %d\n", res.matchIdx[p], res.matchDist[p], (int)res.reached[p]);
  std::printf("found %d stats %d %d %d %d %d\n", found, res.stats[0], res.stats[1], res.stats[2], res.stats[3], res.stats[4]);
  for (int k = 0; k < K; ++k) std::printf("nmatches %d %d\n", k, res.nmatches[k]);
  // the last key frame listed twice, the second time with the first key frame's pose: row 0 of the answer is its row in the search above
  {
    std::vector<const PLVS2hip::KeyFrameHandle*> twice{list.back(), list.back()};
    std::vector<plvs_keyframe_sim3_pose> two{poses.back(), poses.front()};
    PLVS2hip::LoopSearchResult r2;
    PLVS2hip::LoopSearchByProjection(twice, two, P, skip.data() + (size_t)(K - 1) * M, {}, th, ratio, PLVS_LOOP_PROJECT_CAMERA, r2, on_host);
    int same = 0;
    for (int i = 0; i < M; ++i)
      same += (r2.matchIdx[i] == res.matchIdx[(size_t)(K - 1) * M + i] && r2.reached[i] == res.reached[(size_t)(K - 1) * M + i]) ? 1 : 0;
    std::printf("twice %d of %d\n", same, M);
  }
  int refused = 0;
  for (int what = 0; what < 5; ++what) {
    try {
      const plvs_fuse_lines L{0, nullptr, nullptr, nullptr, nullptr, nullptr};
      PLVS2hip::LoopSearchResult lr;
      if (what == 0) {   // a null handle in the list
        std::vector<const PLVS2hip::KeyFrameHandle*> bad = list;
        bad.back() = nullptr;
        PLVS2hip::LoopSearchByProjection(bad, poses, P, skip.data(), {}, th, ratio, PLVS_LOOP_PROJECT_CAMERA, res, on_host);
      } else if (what == 1) {   // a points-only handle in a line search
        PLVS2hip::LoopSearchByProjection(list, poses, L, nullptr, {}, th, ratio, lr, on_host);
      } else if (what == 2) {   // TH_LOW * ratio >= 256
        PLVS2hip::LoopSearchByProjection(list, poses, P, skip.data(), {}, th, 5.12f, PLVS_LOOP_PROJECT_CAMERA, res, on_host);
      } else if (what == 3) {   // an unknown projection
        PLVS2hip::LoopSearchByProjection(list, poses, P, skip.data(), {}, th, ratio, 2, res, on_host);
      } else {   // and the combined search with points-only handles (a device entry: host-only handles are refused there as well)
        PLVS2hip::LoopSearchResult pr;
        PLVS2hip::LoopSearchByProjectionPointsAndLines(list, poses, P, skip.data(), th, ratio, PLVS_LOOP_PROJECT_CAMERA, pr, L, nullptr, th, ratio, lr);
      }
    } catch (const std::runtime_error&) {
      ++refused;
    }
  }
  std::printf("refused %d\n", refused);
  std::printf("loop_search_smoke ok\n");
  return 0;
}
