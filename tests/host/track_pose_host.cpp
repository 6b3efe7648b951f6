// plvs_amd/csrc/track_pose.hpp compiled for the host, stand-alone: the quaternion action and the bForward / bBackward decision
// the projection kernel and its host driver share.  Reads one binary file (tests/test_track_motion.py writes it from the
// scenario): int32 n, q_cw[4], tcw[3], pos[3 n]; int32 ncases, then per case q_lw[4], tlw[3], Ow[3], mb, int32 mono.  Prints the
// bits of every Tcw * x3Dw and the two flags of every case; the test holds them against the reference's recorded run.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../plvs_amd/csrc/track_pose.hpp"

namespace {

bool read_exact(std::FILE* f, void* p, size_t bytes) { return std::fread(p, 1, bytes, f) == bytes; }

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
  int32_t n = 0;
  float q[4], t[3];
  if (!read_exact(f, &n, 4) || n < 0 || n > (1 << 20) || !read_exact(f, q, sizeof q) || !read_exact(f, t, sizeof t)) return 3;
  std::vector<float> pos(3 * (size_t)n);
  if (n && !read_exact(f, pos.data(), sizeof(float) * pos.size())) return 3;
  for (int i = 0; i < n; ++i) {
    const plvs::trackpose::V3 pc = plvs::trackpose::se3_act(q, t, plvs::trackpose::V3{pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]});
    uint32_t b[3];
    std::memcpy(&b[0], &pc.x, 4);
    std::memcpy(&b[1], &pc.y, 4);
    std::memcpy(&b[2], &pc.z, 4);
    std::printf("pc %08x %08x %08x\n", (unsigned)b[0], (unsigned)b[1], (unsigned)b[2]);
  }
  int32_t ncases = 0;
  if (!read_exact(f, &ncases, 4) || ncases < 0 || ncases > 1024) return 3;
  for (int c = 0; c < ncases; ++c) {
    float ql[4], tl[3], ow[3], mb;
    int32_t mono;
    if (!read_exact(f, ql, sizeof ql) || !read_exact(f, tl, sizeof tl) || !read_exact(f, ow, sizeof ow) || !read_exact(f, &mb, 4) ||
        !read_exact(f, &mono, 4))
      return 3;
    int fw = -1, bw = -1;
    plvs::trackpose::direction(ql, tl, ow, mb, mono, &fw, &bw);
    std::printf("direction %d %d\n", fw, bw);
  }
  std::fclose(f);
  std::printf("track_pose ok\n");
  return 0;
}
