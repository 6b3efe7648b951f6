// Exercises the stereo part of include/plvs_hip.hpp (ComputeStereoLineMatches, StereoFrame) and dumps the raw arrays into
// <out_dir>; tests/test_frame_stereo_cpp_mirror.py compares them with the same calls made through the Python mirror.
// Usage: frame_stereo_smoke <left.pgm> <right.pgm> <out_dir>
//        frame_stereo_smoke --args-only     the argument checks that return before any HIP call (runs without a GPU; the
//                                           build with the host side of frame_stereo.hip under ASan / UBSan runs this)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

#include "plvs_hip.hpp"

using namespace PLVS2hip;

static std::string g_out;
static void dump(const std::string& name, const void* p, size_t n) {
  std::ofstream f(g_out + "/" + name + ".bin", std::ios::binary);
  f.write(static_cast<const char*>(p), (std::streamsize)n);
}
template <class T>
static void dump(const std::string& name, const std::vector<T>& v) { dump(name, v.data(), v.size() * sizeof(T)); }

static std::vector<uint8_t> read_pgm(const char* path, int* w, int* h) {
  std::ifstream f(path, std::ios::binary);
  if (!f) { std::fprintf(stderr, "cannot open %s\n", path); std::exit(2); }
  std::string magic;
  int maxv;
  f >> magic >> *w >> *h >> maxv;
  f.get();
  std::vector<uint8_t> img((size_t)*w * *h);
  f.read(reinterpret_cast<char*>(img.data()), (std::streamsize)img.size());
  return img;
}

static int g_failed = 0;
static void expect(int got, int want, const char* what) {
  if (got != want) {
    std::fprintf(stderr, "%s: returned %d, expected %d\n", what, got, want);
    ++g_failed;
  }
}

// Every call here returns from its argument checks: no HIP call is made, no output is written.
static int args_only() {
  const int cap = 512, n = 5, nr = 4;
  std::vector<KeyLine> kl((size_t)cap + 1), klr((size_t)cap + 1);
  std::vector<uint8_t> d(32 * ((size_t)cap + 1), 0x5a), dr(32 * ((size_t)cap + 1), 0xa5);
  for (size_t i = 0; i < kl.size(); ++i) {
    std::memset(&kl[i], 0, sizeof(KeyLine));
    std::memset(&klr[i], 0, sizeof(KeyLine));
    kl[i].octave = klr[i].octave = (int)(i % 3);
  }
  const float sigma2[3] = {1.0f, 1.44f, 2.0736f}, K4[4] = {718.856f, 718.856f, 607.1928f, 185.2157f};
  std::vector<float> o0((size_t)cap + 1, 77.0f), o1(o0), o2(o0), o3(o0);
  int ns = -5;
  auto call = [&](const KeyLine* a, const uint8_t* da, int na, const KeyLine* b, const uint8_t* db, int nb, const float* s2, int levels,
                  const float* K, float* out) {
    return plvs_hip_frame_compute_stereo_line_matches(a, da, na, b, db, nb, s2, levels, K, 386.1448f, 20.0f, 0.01f, 0.7f, 1, 50, out,
                                                      o1.data(), o2.data(), o3.data(), &ns, nullptr);
  };
  expect(call(kl.data(), d.data(), -1, klr.data(), dr.data(), nr, sigma2, 3, K4, o0.data()), PLVS_ERR_INVALID_ARG, "n < 0");
  expect(call(nullptr, d.data(), n, klr.data(), dr.data(), nr, sigma2, 3, K4, o0.data()), PLVS_ERR_INVALID_ARG, "null left lines");
  expect(call(kl.data(), d.data(), n, klr.data(), nullptr, nr, sigma2, 3, K4, o0.data()), PLVS_ERR_INVALID_ARG, "null right descriptors");
  expect(call(kl.data(), d.data(), n, klr.data(), dr.data(), nr, nullptr, 3, K4, o0.data()), PLVS_ERR_INVALID_ARG, "null level table");
  expect(call(kl.data(), d.data(), n, klr.data(), dr.data(), nr, sigma2, 3, nullptr, o0.data()), PLVS_ERR_INVALID_ARG, "null K4");
  expect(call(kl.data(), d.data(), n, klr.data(), dr.data(), nr, sigma2, 3, K4, nullptr), PLVS_ERR_INVALID_ARG, "null output");
  expect(call(kl.data(), d.data(), n, klr.data(), dr.data(), nr, sigma2, 2, K4, o0.data()), PLVS_ERR_INVALID_ARG, "octave outside the table");
  kl[3].octave = -1;
  expect(call(kl.data(), d.data(), n, klr.data(), dr.data(), nr, sigma2, 3, K4, o0.data()), PLVS_ERR_INVALID_ARG, "negative octave");
  kl[3].octave = 0;
  expect(call(kl.data(), d.data(), cap + 1, klr.data(), dr.data(), nr, sigma2, 3, K4, o0.data()), PLVS_ERR_CAPACITY, "capacity + 1 left");
  expect(call(kl.data(), d.data(), n, klr.data(), dr.data(), cap + 1, sigma2, 3, K4, o0.data()), PLVS_ERR_CAPACITY, "capacity + 1 right");
  for (size_t i = 0; i < o0.size(); ++i)
    if (o0[i] != 77.0f || o1[i] != 77.0f || o2[i] != 77.0f || o3[i] != 77.0f || ns != -5) {
      std::fprintf(stderr, "a refused call wrote an output\n");
      ++g_failed;
      break;
    }
  // the reference's early return: all -1, zero lines with depth, nothing launched
  expect(call(kl.data(), d.data(), n, klr.data(), dr.data(), 0, sigma2, 3, K4, o0.data()), PLVS_OK, "n_right == 0");
  for (int i = 0; i < n; ++i)
    if (o0[(size_t)i] != -1.0f || o1[(size_t)i] != -1.0f || o2[(size_t)i] != -1.0f || o3[(size_t)i] != -1.0f) ++g_failed;
  if (ns != 0 || o0[(size_t)n] != 77.0f) ++g_failed;
  expect(call(nullptr, nullptr, 0, klr.data(), dr.data(), nr, sigma2, 3, K4, nullptr), PLVS_OK, "n == 0");
  // the one-call entry: null arguments (the checks that need no handle)
  plvs_stereo_calib c;
  plvs_stereo_frame f;
  std::memset(&c, 0, sizeof c);
  std::memset(&f, 0, sizeof f);
  expect(plvs_hip_frame_stereo_dev(nullptr, nullptr, nullptr, nullptr, nullptr, d.data(), d.data(), 64, 48, 64, &c, &f, nullptr),
         PLVS_ERR_INVALID_ARG, "null handles");
  std::printf("args_only %s\n", g_failed ? "FAILED" : "ok");
  return g_failed ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && std::string(argv[1]) == "--args-only") return args_only();
  if (argc < 4) return 2;
  g_out = argv[3];
  int w, h, wr, hr;
  std::vector<uint8_t> left = read_pgm(argv[1], &w, &h), right = read_pgm(argv[2], &wr, &hr);
  if (w != wr || h != hr) { std::fprintf(stderr, "the two images differ in size\n"); return 2; }
  const Image8U imLeft{h, w, (size_t)w, left.data()}, imRight{h, w, (size_t)w, right.data()};
  const float K4[4] = {718.856f, 718.856f, 607.1928f, 185.2157f}, mbf = 386.1448f;   // KITTI00-02.yaml
  std::vector<float> sigma2;   // mvLineLevelSigma2 of three octaves at scale 1.2
  float scale = 1.0f;
  for (int i = 0; i < 3; ++i, scale *= 1.2f) sigma2.push_back(scale * scale);

  // ---- the line call on separately extracted lines (host flavours of the extractors)
  ORBextractor orbL(2000, 1.2f, 8, 20, 7), orbR(2000, 1.2f, 8, 20, 7);
  LineExtractor linesL(100), linesR(100);
  std::vector<KeyLine> kl, klr;
  std::vector<uint8_t> kld, kldr;
  linesL(imLeft, kl, kld);
  linesR(imRight, klr, kldr);
  std::vector<float> uS, zS, uE, zE;
  const int stereo = ComputeStereoLineMatches(kl, kld, klr, kldr, sigma2, K4, mbf, uS, zS, uE, zE);
  std::printf("line_call %d %d %d\n", (int)kl.size(), (int)klr.size(), stereo);
  dump("s_keylines", kl); dump("s_keylines_right", klr); dump("s_line_desc", kld); dump("s_line_desc_right", kldr);
  dump("s_u_right_start", uS); dump("s_depth_start", zS); dump("s_u_right_end", uE); dump("s_depth_end", zE);

  // ---- the constructor in one call, both images in device memory
  void *dLeft = nullptr, *dRight = nullptr;
  check(plvs_hip_malloc(&dLeft, left.size()));
  check(plvs_hip_malloc(&dRight, right.size()));
  check(plvs_hip_memcpy_h2d(dLeft, left.data(), left.size()));
  check(plvs_hip_memcpy_h2d(dRight, right.data(), right.size()));
  const ImageBounds b = ComputeImageBounds(w, h, K4, std::vector<float>());
  plvs_stereo_calib c;
  std::memset(&c, 0, sizeof c);
  for (int k = 0; k < 4; ++k) c.K4[k] = K4[k];
  c.mbf = mbf;
  c.bounds4[0] = b.mnMinX; c.bounds4[1] = b.mnMaxX; c.bounds4[2] = b.mnMinY; c.bounds4[3] = b.mnMaxY;
  c.grid_w_inv = 64.0f / (b.mnMaxX - b.mnMinX);
  c.grid_h_inv = 48.0f / (b.mnMaxY - b.mnMinY);
  c.min_line_length_3d = 0.01f;
  c.line_stereo_max_dist = 20.0f;
  c.nn_ratio = 0.7f;
  c.check_orientation = 1;
  c.descriptor_dist = 50;
  c.n_line_levels = (int)sigma2.size();
  c.line_level_sigma2 = sigma2.data();
  plvs_stereo* sm = nullptr;
  check(plvs_hip_stereo_create(orbL.handle(), orbR.handle(), &sm));
  StereoFrameMembers F;
  StereoFrame(orbL, orbR, &linesL, &linesR, sm, static_cast<const uint8_t*>(dLeft), static_cast<const uint8_t*>(dRight), w, h, w, c, F);
  std::printf("one_call %d %d %d %d %d %d %d %d\n", F.monoLeft, (int)F.mvKeys.size(), (int)F.mvKeysRight.size(), (int)F.mvKeyLines.size(),
              (int)F.mvKeyLinesRight.size(), (int)F.cellItems.size(), F.stereoPoints, F.stereoLines);
  dump("f_keys", F.mvKeys); dump("f_keys_un", F.mvKeysUn); dump("f_desc", F.mDescriptors); dump("f_u_right", F.mvuRight);
  dump("f_depth", F.mvDepth); dump("f_keys_right", F.mvKeysRight); dump("f_desc_right", F.mDescriptorsRight);
  dump("f_keylines", F.mvKeyLines); dump("f_keylines_un", F.mvKeyLinesUn); dump("f_line_desc", F.mLineDescriptors);
  dump("f_keylines_right", F.mvKeyLinesRight); dump("f_keylines_right_un", F.mvKeyLinesRightUn);
  dump("f_line_desc_right", F.mLineDescriptorsRight);
  dump("f_u_right_start", F.mvuRightLineStart); dump("f_depth_start", F.mvDepthLineStart);
  dump("f_u_right_end", F.mvuRightLineEnd); dump("f_depth_end", F.mvDepthLineEnd);
  dump("f_cell_start", F.cellStart); dump("f_cell_items", F.cellItems);
  check(plvs_hip_stereo_destroy(sm));
  check(plvs_hip_free(dLeft));
  check(plvs_hip_free(dRight));
  return 0;
}
