// Exercises the frame glue and the RGB-D part of include/plvs_hip.hpp (UndistortKeyPoints, ComputeImageBounds, UndistortKeyLines,
// AssignFeaturesToGrid, ComputeStereoFromRGBD, ComputeStereoLinesFromRGBD, ComputeSceneMedianDepth, rgbd_frame) and dumps the raw
// arrays into <out_dir>; tests/test_frame_rgbd_cpp_mirror.py compares them with the same calls made through the Python mirror.
// Usage: frame_rgbd_smoke <grey.pgm> <depth.bin: rows x pitch float32> <pitch> <out_dir>
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

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const int pitch = std::atoi(argv[3]);
  g_out = argv[4];
  int w, h;
  std::vector<uint8_t> grey = read_pgm(argv[1], &w, &h);
  std::vector<float> depth((size_t)pitch * h);
  {
    std::ifstream f(argv[2], std::ios::binary);
    f.read(reinterpret_cast<char*>(depth.data()), (std::streamsize)(depth.size() * sizeof(float)));
    if (!f || pitch < w) { std::fprintf(stderr, "bad depth file\n"); return 2; }
  }
  const Image8U image{h, w, (size_t)w, grey.data()};
  const Image32F imDepth{h, w, sizeof(float) * (size_t)pitch, depth.data()};
  const float K4[4] = {517.3f, 516.5f, 318.6f, 255.3f}, mbf = 40.0f;
  const std::vector<float> dist = {0.2624f, -0.9531f, -0.0054f, 0.0026f, 1.1633f};

  // ---- the constructor's steps one by one (host flavours)
  ORBextractor orb(1000, 1.2f, 8, 20, 7);
  LineExtractor lines(100);
  std::vector<KeyPoint> keys, keysUn;
  std::vector<uint8_t> desc, lineDesc;
  std::vector<KeyLine> keylines, keylinesUn;
  const int mono = orb(image, keys, desc);
  lines(image, keylines, lineDesc);
  const size_t extracted = keylines.size();
  ImageBounds b = ComputeImageBounds(w, h, K4, dist);
  const float gw = 64.0f / (b.mnMaxX - b.mnMinX), gh = 48.0f / (b.mnMaxY - b.mnMinY);
  dump("bounds", &b, sizeof b);
  b.mnMaxX -= 60.0f;   // the caller's bounds: narrower on the right, so that lines are dropped
  UndistortKeyPoints(keys, K4, dist, keysUn);
  std::vector<float> uR, z, uS, zS, uE, zE;
  ComputeStereoFromRGBD(keys, keysUn, imDepth, mbf, uR, z);
  const float median = ComputeSceneMedianDepth(z);
  UndistortKeyLines(keylines, lineDesc, K4, dist, b, keylinesUn);
  ComputeStereoLinesFromRGBD(keylines, keylinesUn, imDepth, K4, mbf, uS, zS, uE, zE);
  std::vector<int32_t> cellStart, cellItems;
  AssignFeaturesToGrid(keysUn, b.mnMinX, b.mnMinY, gw, gh, cellStart, cellItems);
  std::printf("steps %d %d %d %d %d %.9g\n", mono, (int)keys.size(), (int)extracted, (int)keylines.size(), (int)cellItems.size(), (double)median);
  dump("s_keys", keys); dump("s_keys_un", keysUn); dump("s_desc", desc); dump("s_u_right", uR); dump("s_depth", z);
  dump("s_keylines", keylines); dump("s_keylines_un", keylinesUn); dump("s_line_desc", lineDesc);
  dump("s_u_right_start", uS); dump("s_depth_start", zS); dump("s_u_right_end", uE); dump("s_depth_end", zE);
  dump("s_cell_start", cellStart); dump("s_cell_items", cellItems);

  // ---- the constructor in one call, image and depth in device memory
  void *dImage = nullptr, *dDepth = nullptr;
  check(plvs_hip_malloc(&dImage, grey.size()));
  check(plvs_hip_malloc(&dDepth, depth.size() * sizeof(float)));
  check(plvs_hip_memcpy_h2d(dImage, grey.data(), grey.size()));
  check(plvs_hip_memcpy_h2d(dDepth, depth.data(), depth.size() * sizeof(float)));
  plvs_rgbd_calib c;
  std::memset(&c, 0, sizeof c);
  for (int k = 0; k < 4; ++k) c.K4[k] = K4[k];
  for (size_t k = 0; k < dist.size(); ++k) c.dist[k] = dist[k];
  c.ndist = (int)dist.size();
  c.mbf = mbf;
  c.bounds4[0] = b.mnMinX; c.bounds4[1] = b.mnMaxX; c.bounds4[2] = b.mnMinY; c.bounds4[3] = b.mnMaxY;
  c.grid_w_inv = gw; c.grid_h_inv = gh;
  c.min_line_length_3d = 0.01f;
  c.use_median_depth = 1;
  c.median_fallback = 1.5f;
  RgbdFrame F;
  rgbd_frame(orb, &lines, static_cast<const uint8_t*>(dImage), w, h, w, static_cast<const float*>(dDepth), pitch, c, F);
  std::printf("one_call %d %d %d %d %.9g\n", F.monoLeft, (int)F.mvKeys.size(), (int)F.mvKeyLines.size(), (int)F.cellItems.size(),
              (double)F.mMedianDepth);
  dump("f_keys", F.mvKeys); dump("f_keys_un", F.mvKeysUn); dump("f_desc", F.mDescriptors); dump("f_u_right", F.mvuRight);
  dump("f_depth", F.mvDepth); dump("f_keylines", F.mvKeyLines); dump("f_keylines_un", F.mvKeyLinesUn);
  dump("f_line_desc", F.mLineDescriptors); dump("f_u_right_start", F.mvuRightLineStart); dump("f_depth_start", F.mvDepthLineStart);
  dump("f_u_right_end", F.mvuRightLineEnd); dump("f_depth_end", F.mvDepthLineEnd); dump("f_cell_start", F.cellStart);
  dump("f_cell_items", F.cellItems);
  check(plvs_hip_free(dImage));
  check(plvs_hip_free(dDepth));
  return 0;
}
