// Exercises the local-map part of include/plvs_hip.hpp (IsInFrustum, SearchLocalMap) on a hand-made map and prints the fields as
// raw bits; tests/test_track_local_cpp_mirror.py compares them with the same calls made through the Python mirror.
// Usage: track_local_smoke              the calls on the GPU
//        track_local_smoke --args-only  the requests that are refused before anything is launched (runs without a GPU)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "plvs_hip.hpp"

using namespace PLVS2hip;

static int g_failed = 0;
static void expect(int got, int want, const char* what) {
  if (got != want) {
    std::fprintf(stderr, "%s: returned %d, expected %d\n", what, got, want);
    ++g_failed;
  }
}

struct Scene {
  float K4[4] = {517.306408f, 516.469215f, 318.643040f, 255.313989f}, bounds4[4] = {0, 640, 0, 480};
  float Rcw[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tcw[3] = {0.1f, -0.05f, 0.2f}, Ow[3] = {-0.1f, 0.05f, -0.2f};
  // in view; behind the camera; left of the image; too far; grazing
  uint8_t skip[6] = {0, 0, 0, 0, 0, 1};
  float pos[18] = {0.2f, 0.1f, 3.0f, 0.0f, 0.0f, -2.0f, -9.0f, 0.0f, 3.0f, 0.1f, 0.1f, 4.0f, 0.3f, -0.2f, 2.5f, 0.2f, 0.1f, 3.0f};
  float normal[18] = {0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 1, 0, 0, 0, 0, 1};
  float min_dist[6] = {0.5f, 0.5f, 0.5f, 0.2f, 0.5f, 0.5f}, max_dist[6] = {5.0f, 5.0f, 20.0f, 2.0f, 5.0f, 5.0f};
  uint8_t lskip[2] = {0, 0};
  float start[6] = {-0.5f, 0.2f, 3.0f, 0.5f, 0.0f, 3.0f}, end[6] = {0.5f, 0.3f, 3.5f, 0.9f, 0.4f, -1.0f};
  float lnormal[6] = {0, 0, 1, 0, 0, 1}, lmax[2] = {3.2f, 1.6f};
  uint8_t desc[6 * 32], ldesc[2 * 32];
  plvs_track_camera cam;
  plvs_track_points P;
  plvs_track_lines L;
  Scene() {
    std::memset(desc, 0x5a, sizeof desc);
    std::memset(ldesc, 0xa5, sizeof ldesc);
    std::memset(&cam, 0, sizeof cam);
    std::memset(&P, 0, sizeof P);
    std::memset(&L, 0, sizeof L);
    cam.n_cameras = 1; cam.camera_model = PLVS_CAMERA_PINHOLE; cam.K4 = K4; cam.mbf = 40.0f; cam.bounds4 = bounds4;
    cam.Rcw = Rcw; cam.tcw = tcw; cam.Ow = Ow; cam.viewing_cos_limit = 0.5f;
    cam.log_scale_factor = cam.line_log_scale_factor = std::log(1.2f);
    cam.n_levels = 8; cam.n_line_levels = 3;
    P.m = 6; P.skip = skip; P.pos = pos; P.normal = normal; P.min_dist = min_dist; P.max_dist = max_dist; P.desc = desc;
    L.m = 2; L.skip = lskip; L.start = start; L.end = end; L.normal = lnormal; L.max_dist = lmax; L.desc = ldesc;
  }
};

// Every request here is refused by the argument checks: nothing is launched, no output is written.
static int args_only() {
  Scene s;
  LocalMapFields out;
  detail::bind(out, &s.P, &s.L);
  out.trackProjX.assign(6, 77.0f);
  s.P.proj_x = out.trackProjX.data();
  int nv = -5, nvl = -5;
  auto call = [&]() { return plvs_hip_frame_is_in_frustum(&s.cam, &s.P, &s.L, &nv, &nvl, nullptr, nullptr); };
  s.cam.n_cameras = 2; expect(call(), PLVS_ERR_INVALID_ARG, "two cameras"); s.cam.n_cameras = 1;
  s.cam.camera_model = 1; expect(call(), PLVS_ERR_INVALID_ARG, "a fisheye camera"); s.cam.camera_model = PLVS_CAMERA_PINHOLE;
  s.cam.n_levels = -1; expect(call(), PLVS_ERR_INVALID_ARG, "negative point levels"); s.cam.n_levels = 8;
  s.cam.n_line_levels = 0; expect(call(), PLVS_ERR_INVALID_ARG, "no line levels"); s.cam.n_line_levels = 3;
  s.P.pos = nullptr; expect(call(), PLVS_ERR_INVALID_ARG, "null positions"); s.P.pos = s.pos;
  s.L.start = nullptr; expect(call(), PLVS_ERR_INVALID_ARG, "null line starts"); s.L.start = s.start;
  s.P.level = nullptr; expect(call(), PLVS_ERR_INVALID_ARG, "null level output"); s.P.level = out.trackScaleLevel.data();
  s.P.m = -1; expect(call(), PLVS_ERR_INVALID_ARG, "negative count"); s.P.m = 6;
  s.cam.Rcw = nullptr; expect(call(), PLVS_ERR_INVALID_ARG, "null pose"); s.cam.Rcw = s.Rcw;
  expect(plvs_hip_frame_is_in_frustum(nullptr, &s.P, &s.L, &nv, &nvl, nullptr, nullptr), PLVS_ERR_INVALID_ARG, "null camera");
  if (std::string(plvs_hip_last_error()).empty()) { std::fprintf(stderr, "no message with the refusal\n"); ++g_failed; }
  // the search: a missing frame view, map lines without a line view, missing descriptors
  plvs_frame_view F;
  std::memset(&F, 0, sizeof F);
  int nm = -5, nml = -5;
  int32_t assigned[1] = {77};
  auto search = [&](const plvs_frame_view* f, const plvs_line_frame_view* lf) {
    return plvs_hip_frame_search_local_map(&s.cam, f, lf, &s.P, &s.L, 1.0f, 0, 0.0f, 0.8f, 0, nullptr, nullptr, assigned, &nm, nullptr, &nml, &nv, &nvl,
                                           nullptr, nullptr);
  };
  expect(search(nullptr, nullptr), PLVS_ERR_INVALID_ARG, "null frame view");
  expect(search(&F, nullptr), PLVS_ERR_INVALID_ARG, "map lines without a line frame view");
  s.cam.camera_model = 2; expect(search(&F, nullptr), PLVS_ERR_INVALID_ARG, "search with a fisheye camera"); s.cam.camera_model = 0;
  for (float v : out.trackProjX)
    if (v != 77.0f) { std::fprintf(stderr, "a refused call wrote an output\n"); ++g_failed; }
  if (nv != -5 || nvl != -5 || nm != -5 || assigned[0] != 77) { std::fprintf(stderr, "a refused call wrote a count\n"); ++g_failed; }
  if (!g_failed) std::printf("args_only ok\n");
  return g_failed ? 1 : 0;
}

static void print_bits(const char* name, const std::vector<float>& v) {
  std::printf("%s", name);
  for (float f : v) { uint32_t u; std::memcpy(&u, &f, 4); std::printf(" %08x", u); }
  std::printf("\n");
}
template <class T>
static void print_ints(const char* name, const std::vector<T>& v) {
  std::printf("%s", name);
  for (T x : v) std::printf(" %d", (int)x);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc > 1 && std::string(argv[1]) == "--args-only") return args_only();
  Scene s;
  LocalMapFields out;
  IsInFrustum(s.cam, &s.P, &s.L, out);
  std::printf("n_to_match %d %d\n", out.nToMatchPoints, out.nToMatchLines);
  print_ints("point_in_view", out.pointInView);
  print_bits("proj_x", out.trackProjX); print_bits("proj_y", out.trackProjY); print_bits("proj_xr", out.trackProjXR);
  print_bits("track_depth", out.trackDepth); print_bits("view_cos", out.trackViewCos);
  print_ints("level", out.trackScaleLevel);
  print_ints("line_in_view", out.lineInView);
  print_bits("line_proj", out.lineProj); print_bits("line_proj_xr", out.lineProjXR); print_bits("line_view_cos", out.lineViewCos);
  print_ints("line_level", out.lineScaleLevel);
  // the search on a frame of two key points, one where map point 0 projects
  float x[2] = {out.trackProjX[0] + 0.5f, 600.0f}, y[2] = {out.trackProjY[0] - 0.5f, 20.0f}, ur[2] = {-1.0f, -1.0f};
  int32_t octave[2] = {out.trackScaleLevel[0], 0};
  uint8_t fdesc[64];
  std::memset(fdesc, 0x5a, sizeof fdesc);
  fdesc[0] = 0x5b;
  float sf[8] = {1.0f, 1.2f, 1.44f, 1.728f, 2.0736f, 2.48832f, 2.985984f, 3.5831808f};
  plvs_frame_view F;
  std::memset(&F, 0, sizeof F);
  F.n = 2; F.x = x; F.y = y; F.octave = octave; F.u_right = ur; F.desc = fdesc; F.grid_w_inv = 0.1f; F.grid_h_inv = 0.1f; F.scale_factors = sf;
  LocalMapFields found;
  SearchLocalMap(s.cam, F, nullptr, s.P, nullptr, 1.0f, false, 0.0f, 0.8f, false, nullptr, nullptr, found);
  std::printf("nmatches %d %d\n", found.nMatchesPoints, found.nMatchesLines);
  print_ints("assigned_points", found.assignedPoints);
  return 0;
}
