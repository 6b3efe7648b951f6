// Exercises the motion-model part of include/plvs_hip.hpp (TrackWithMotionModelSearch) on a set of inputs read from one binary
// file and prints the results; tests/test_track_motion_cpp_mirror.py writes the file from tests/track_motion_scenario.py and holds
// the output against the reference's recorded run.
// Usage: track_motion_smoke <file> <th> <check> <min points> <min lines>   the call on the GPU
//        track_motion_smoke --args-only                                     the requests refused before anything is launched
// File: int32 N, n, NL, nl, levels, line_levels; then
//   frame   x[N] y[N] octave[N] u_right[N] desc[32 N] cur_angle[N] scale_factors[levels]
//   lines   keylines[NL] (68 bytes each) line_desc[32 NL] u_right_start[NL] u_right_end[NL] line_scale[line_levels] line_inv_sigma2[line_levels]
//   poses   q_cw[4] tcw[3] Rcw[9] Ow[3] q_lw[4] tlw[3] mb mbf bounds4[4] K4[4] max_diag grid_w_inv grid_h_inv
//   points  valid[n] pos[3 n] octave[n] angle[n] desc[32 n] has_obs[n]
//   last    valid[nl] start[3 nl] end[3 nl] max_dist[nl] octave[nl] angle[nl] desc[32 nl] has_obs[nl]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "plvs_hip.hpp"

using namespace PLVS2hip;

static int g_failed = 0;
static void expect(int got, int want, const char* what) {
  if (got != want) {
    std::fprintf(stderr, "%s: returned %d, expected %d\n", what, got, want);
    ++g_failed;
  }
}

template <class T>
static std::vector<T> take(std::FILE* f, size_t count) {
  std::vector<T> v(count);
  if (count && std::fread(v.data(), sizeof(T), count, f) != count) {
    std::fprintf(stderr, "short input file\n");
    std::exit(3);
  }
  return v;
}

// Every request here is refused by the argument checks: nothing is launched.
static int args_only() {
  float q[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0}, R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, b[4] = {0, 640, 0, 480}, K[4] = {500, 500, 320, 240};
  plvs_motion_poses M;
  std::memset(&M, 0, sizeof M);
  M.n_cameras = 1; M.camera_model = PLVS_CAMERA_PINHOLE; M.q_cw = q; M.tcw = t; M.Rcw = R; M.Ow = t; M.q_lw = q; M.tlw = t;
  M.mb = 0.08f; M.mbf = 40.0f; M.bounds4 = b; M.K4 = K;
  float x[1] = {10}, sf[1] = {1};
  int32_t oct[1] = {0}, assigned[1] = {-5};
  uint8_t desc[32] = {0}, valid[1] = {1};
  plvs_frame_view F;
  std::memset(&F, 0, sizeof F);
  F.n = 1; F.x = x; F.y = x; F.octave = oct; F.u_right = x; F.desc = desc; F.grid_w_inv = F.grid_h_inv = 0.1f; F.scale_factors = sf;
  plvs_motion_points P;
  std::memset(&P, 0, sizeof P);
  float pos[3] = {0, 0, 2}, ang[1] = {0};
  P.n = 1; P.valid = valid; P.pos = pos; P.octave = oct; P.angle = ang; P.desc = desc;
  plvs_motion_policy pol = {15.0f, 0.9f, 0.9f, 1, 0, 0};
  plvs_motion_result res;
  auto call = [&]() { return plvs_hip_frame_search_last_frame(&M, &F, ang, nullptr, &P, nullptr, &pol, nullptr, nullptr, assigned, nullptr, &res, nullptr, nullptr); };
  M.n_cameras = 2;
  expect(call(), PLVS_ERR_INVALID_ARG, "two cameras");
  M.n_cameras = 1; M.camera_model = 1;
  expect(call(), PLVS_ERR_INVALID_ARG, "a non-pinhole model");
  M.camera_model = PLVS_CAMERA_PINHOLE; oct[0] = -1;
  expect(call(), PLVS_ERR_INVALID_ARG, "a negative octave");
  oct[0] = 0; P.pos = nullptr;
  expect(call(), PLVS_ERR_INVALID_ARG, "a NULL position array");
  P.pos = pos; M.q_cw = nullptr;
  expect(call(), PLVS_ERR_INVALID_ARG, "a NULL quaternion");
  M.q_cw = q;
  bool threw = false;
  try {
    MotionModelMatches out;
    M.n_cameras = 2;
    const plvs_motion_points& Pconst = P;   // the inputs are taken const
    TrackWithMotionModelSearch(M, F, ang, nullptr, Pconst, nullptr, 15.0f, true, out);
  } catch (const std::exception&) {
    threw = true;
  }
  expect(threw ? 1 : 0, 1, "the wrapper throws on a refused request");
  expect(P.proj_valid == nullptr && P.u == nullptr && P.v == nullptr && P.invz == nullptr ? 1 : 0, 1,
         "the wrapper leaves the caller's structure as it is: no pointer into `out` outlives it");
  expect(assigned[0], -5, "nothing is written by a refused request");
  if (!g_failed) std::printf("args_only ok\n");
  return g_failed ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && std::string(argv[1]) == "--args-only") return args_only();
  if (argc != 6) {
    std::fprintf(stderr, "usage: %s <file> <th> <check> <min points> <min lines> | --args-only\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  const std::vector<int32_t> hd = take<int32_t>(f, 6);
  const size_t N = (size_t)hd[0], n = (size_t)hd[1], NL = (size_t)hd[2], nl = (size_t)hd[3], levels = (size_t)hd[4], line_levels = (size_t)hd[5];
  auto x = take<float>(f, N), y = take<float>(f, N);
  auto octave = take<int32_t>(f, N);
  auto u_right = take<float>(f, N);
  auto desc = take<uint8_t>(f, 32 * N);
  auto cur_angle = take<float>(f, N), sf = take<float>(f, levels);
  auto keylines = take<plvs_keyline>(f, NL);
  auto line_desc = take<uint8_t>(f, 32 * NL);
  auto urs = take<float>(f, NL), ure = take<float>(f, NL), lsf = take<float>(f, line_levels), lis2 = take<float>(f, line_levels);
  auto pose = take<float>(f, 4 + 3 + 9 + 3 + 4 + 3 + 2 + 4 + 4 + 3);
  auto pvalid = take<uint8_t>(f, n);
  auto pos = take<float>(f, 3 * n);
  auto poct = take<int32_t>(f, n);
  auto pang = take<float>(f, n);
  auto pdesc = take<uint8_t>(f, 32 * n);
  auto pobs = take<uint8_t>(f, n);
  auto lvalid = take<uint8_t>(f, nl);
  auto start = take<float>(f, 3 * nl), end = take<float>(f, 3 * nl), lmax = take<float>(f, nl);
  auto loct = take<int32_t>(f, nl);
  auto lang = take<float>(f, nl);
  auto ldesc = take<uint8_t>(f, 32 * nl);
  auto lobs = take<uint8_t>(f, nl);
  std::fclose(f);

  const float* p = pose.data();
  plvs_motion_poses M;
  std::memset(&M, 0, sizeof M);
  M.n_cameras = 1; M.camera_model = PLVS_CAMERA_PINHOLE; M.mono = 0;
  M.q_cw = p; M.tcw = p + 4; M.Rcw = p + 7; M.Ow = p + 16; M.q_lw = p + 19; M.tlw = p + 23; M.mb = p[26]; M.mbf = p[27];
  M.bounds4 = p + 28; M.K4 = p + 32; M.K4_linear = nullptr;
  plvs_frame_view F;
  std::memset(&F, 0, sizeof F);
  F.n = (int32_t)N; F.x = x.data(); F.y = y.data(); F.octave = octave.data(); F.u_right = u_right.data(); F.desc = desc.data();
  F.min_x = M.bounds4[0]; F.min_y = M.bounds4[2]; F.grid_w_inv = p[37]; F.grid_h_inv = p[38]; F.scale_factors = sf.data();
  plvs_line_frame_view LF;
  std::memset(&LF, 0, sizeof LF);
  LF.n = (int32_t)NL; LF.keylines_un = keylines.data(); LF.descriptors = line_desc.data(); LF.u_right_start = urs.data(); LF.u_right_end = ure.data();
  LF.bf = M.mbf; LF.n_levels = (int32_t)line_levels; LF.line_scale_factors = lsf.data(); LF.line_inv_level_sigma2 = lis2.data(); LF.max_diag = p[36];
  plvs_motion_points P;
  std::memset(&P, 0, sizeof P);
  P.n = (int32_t)n; P.valid = pvalid.data(); P.pos = pos.data(); P.octave = poct.data(); P.angle = pang.data(); P.desc = pdesc.data(); P.has_obs = pobs.data();
  plvs_motion_lines L;
  std::memset(&L, 0, sizeof L);
  L.n = (int32_t)nl; L.valid = lvalid.data(); L.start = start.data(); L.end = end.data(); L.max_dist = lmax.data(); L.octave = loct.data();
  L.angle = lang.data(); L.desc = ldesc.data(); L.has_obs = lobs.data();

  MotionModelMatches out;
  try {
    TrackWithMotionModelSearch(M, F, cur_angle.data(), NL ? &LF : nullptr, P, nl ? &L : nullptr, (float)std::atof(argv[2]), std::atoi(argv[3]) != 0, out,
                               nullptr, nullptr, std::atoi(argv[4]), std::atoi(argv[5]));
  } catch (const std::exception& e) {
    std::fprintf(stderr, "TrackWithMotionModelSearch: %s\n", e.what());
    return 1;
  }
  std::printf("nmatches %d %d\n", out.nPointMatches, out.nLineMatches);
  std::printf("flags %d %d %d %g\n", out.bForward ? 1 : 0, out.bBackward ? 1 : 0, out.bLargerLineSearch ? 1 : 0, (double)out.thUsed);
  std::printf("stats %d %d %d %d\n", out.stats[0], out.stats[1], out.stats[2], out.stats[3]);
  std::printf("assigned_points");
  for (int32_t a : out.assignedPoints) std::printf(" %d", a);
  std::printf("\nassigned_lines");
  for (int32_t a : out.assignedLines) std::printf(" %d", a);
  std::printf("\nproj_valid_points");
  for (uint8_t a : out.projValidPoints) std::printf(" %d", (int)a);
  std::printf("\nu");
  for (float a : out.u) { uint32_t b; std::memcpy(&b, &a, 4); std::printf(" %08x", (unsigned)b); }
  std::printf("\nline_proj");
  for (float a : out.lineProj) { uint32_t b; std::memcpy(&b, &a, 4); std::printf(" %08x", (unsigned)b); }
  std::printf("\n");
  return 0;
}
