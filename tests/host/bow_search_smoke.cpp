// BowSearch of include/plvs_hip.hpp against nothing but the C ABI: reads the sides tests/test_bow_search_cpp_mirror.py wrote, makes the
// handles, runs both SearchByBoW kinds on the host or on the device and prints every output.
//   bow_search_smoke <inputs.bin> <host|device> <nn_ratio> <check_orientation>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "plvs_hip.hpp"

namespace {

struct Side {
  int32_t n = 0;
  std::vector<uint8_t> desc, valid;
  std::vector<float> angle, x, y, u_right;
  std::vector<int32_t> octave;
  std::map<unsigned int, std::vector<unsigned int>> vec;
};

bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

bool read_side(FILE* f, Side* s) {
  int32_t nnodes = 0;
  if (!read_exact(f, &s->n, 4) || !read_exact(f, &nnodes, 4)) return false;
  const size_t n = (size_t)s->n;
  s->desc.resize(n * 32); s->valid.resize(n); s->angle.resize(n);
  if (!read_exact(f, s->desc.data(), n * 32) || !read_exact(f, s->angle.data(), n * 4) || !read_exact(f, s->valid.data(), n)) return false;
  for (int a = 0; a < nnodes; ++a) {
    uint32_t id = 0;
    int32_t len = 0;
    if (!read_exact(f, &id, 4) || !read_exact(f, &len, 4)) return false;
    std::vector<unsigned int>& list = s->vec[id];
    list.resize((size_t)len);
    if (!read_exact(f, list.data(), (size_t)len * 4)) return false;
  }
  s->x.resize(n); s->y.resize(n); s->u_right.assign(n, -1.0f); s->octave.assign(n, 0);
  for (size_t i = 0; i < n; ++i) { s->x[i] = 10.0f + 37.0f * (float)(i % 16); s->y[i] = 10.0f + 23.0f * (float)(i / 16); }
  return true;
}

const float kScale[2] = {1.0f, 1.2f}, kSigma[2] = {1.0f, 1.0f / 1.44f}, kK4[4] = {500, 500, 320, 240}, kBounds[4] = {0, 640, 0, 480};

PLVS2hip::KeyFrameHandle make(const Side& s, bool host_only) {
  plvs_fuse_keyframe kf;
  memset(&kf, 0, sizeof kf);
  kf.view = plvs_frame_view{s.n, s.x.data(), s.y.data(), s.octave.data(), s.u_right.data(), s.desc.data(), 0.0f, 0.0f, 64 / 640.0f, 48 / 480.0f, kScale};
  kf.inv_level_sigma2 = kSigma;
  kf.n_levels = 2;
  kf.log_scale_factor = 0.18232156f;
  kf.n_cameras = 1;
  kf.camera_model = PLVS_CAMERA_PINHOLE;
  kf.K4 = kK4;
  kf.mbf = 40.0f;
  kf.bounds4 = kBounds;
  return PLVS2hip::BowSearch::MakeKeyFrame(kf, nullptr, s.vec, s.angle, host_only);
}

void print(const char* kind, const PLVS2hip::BowSearch::Result& r, int total) {
  printf("%s total %d stats %d %d %d %d %d %d\n", kind, total, r.stats[0], r.stats[1], r.stats[2], r.stats[3], r.stats[4], r.stats[5]);
  printf("%s nmatches", kind);
  for (int32_t v : r.nmatches) printf(" %d", v);
  printf("\n");
  for (size_t i = 0; i < r.match.size(); ++i)
    if (r.match[i] >= 0) printf("%s match %zu %d %d\n", kind, i, r.match[i], r.matchDist[i]);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  const bool on_host = std::string(argv[2]) == "host";
  int32_t K = 0;
  Side a;
  if (!read_exact(f, &K, 4) || !read_side(f, &a)) return 3;
  std::vector<Side> bs((size_t)K);
  for (Side& b : bs)
    if (!read_side(f, &b)) return 3;
  fclose(f);
  try {
    const PLVS2hip::KeyFrameHandle ha = make(a, on_host);
    std::vector<PLVS2hip::KeyFrameHandle> hb;
    std::vector<const PLVS2hip::KeyFrameHandle*> list;
    std::vector<std::vector<uint8_t>> valid;
    for (const Side& b : bs) hb.push_back(make(b, on_host));
    for (size_t k = 0; k < bs.size(); ++k) { list.push_back(&hb[k]); valid.push_back(bs[k].valid); }
    const PLVS2hip::KeyFrameHandle::BowInfo info = ha.bowInfo();
    printf("bow_info %lld %lld %lld\n", (long long)info.nodes, (long long)info.listed, (long long)info.longest);
    const PLVS2hip::BowSearch matcher((float)atof(argv[3]), atoi(argv[4]) != 0);
    PLVS2hip::BowSearch::Result r;
    int total = matcher.SearchByBoW(ha, a.valid, list, valid, r, on_host);
    print("kf", r, total);
    total = matcher.SearchByBoW(list, valid, a.desc.data(), a.angle, a.vec, r, on_host);
    print("frame", r, total);
    bool refused = false;
    try {
      const PLVS2hip::BowSearch bad(-1.0f, true);
      bad.SearchByBoW(ha, a.valid, list, valid, r, on_host);
    } catch (const std::exception&) {
      refused = true;
    }
    printf("refused %d\n", refused ? 1 : 0);
  } catch (const std::exception& e) {
    printf("error %s\n", e.what());
    return 1;
  }
  printf("bow_search_smoke ok\n");
  return 0;
}
