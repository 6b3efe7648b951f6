// What a caller of plvs_hip_orb_search_by_projection_ff + plvs_hip_lines_search_by_projection_ff has to run on the host before the
// two calls: the projection of every last-frame map point and map line into the current frame, in the arithmetic of
// tests/track_motion_restatement.py (plvs_amd/csrc/track_pose.hpp for the points), one core.  Built and timed by
// scripts/measure_track_motion.py; not part of the library.
#include <cmath>
#include <cstdint>

#include "../plvs_amd/csrc/track_pose.hpp"

using plvs::trackpose::V3;

namespace {
inline V3 to_camera(const float* R, const float* t, const V3& p) {
  return V3{(R[0] * p.x + (R[3] * p.y + R[6] * p.z)) + t[0], (R[1] * p.x + (R[4] * p.y + R[7] * p.z)) + t[1],
            (R[2] * p.x + (R[5] * p.y + R[8] * p.z)) + t[2]};
}
inline bool outside(const float* b, float u, float v) { return u < b[0] || u > b[1] || v < b[2] || v > b[3]; }
}  // namespace

extern "C" void host_loop(const float* q, const float* t, const float* R, const float* K, const float* b, int n, const uint8_t* valid,
                          const float* pos, uint8_t* pv, float* u, float* v, float* invz, int nl, const uint8_t* lvalid, const float* start,
                          const float* end, const float* max_dist, uint8_t* lv, float* proj6) {
  for (int i = 0; i < n; ++i) {
    pv[i] = 0; u[i] = v[i] = -1.0f; invz[i] = 0.0f;
    if (!valid[i]) continue;
    const V3 pc = plvs::trackpose::se3_act(q, t, V3{pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]});
    invz[i] = (float)(1.0 / (double)pc.z);
    if (invz[i] < 0) continue;
    u[i] = K[0] * pc.x / pc.z + K[2];
    v[i] = K[1] * pc.y / pc.z + K[3];
    pv[i] = outside(b, u[i], v[i]) ? 0 : 1;
  }
  for (int i = 0; i < nl; ++i) {
    float* o = proj6 + 6 * i;
    o[0] = o[1] = o[2] = o[3] = -1.0f; o[4] = o[5] = 0.0f;
    lv[i] = 0;
    if (!lvalid[i]) continue;
    const V3 S{start[3 * i], start[3 * i + 1], start[3 * i + 2]}, E{end[3 * i], end[3 * i + 1], end[3 * i + 2]};
    const V3 Mc = to_camera(R, t, V3{(S.x + E.x) * 0.5f, (S.y + E.y) * 0.5f, (S.z + E.z) * 0.5f});
    if (Mc.z < 0.0f) continue;
    if (outside(b, K[0] * Mc.x / Mc.z + K[2], K[1] * Mc.y / Mc.z + K[3])) continue;
    const float dist = std::sqrt(Mc.x * Mc.x + (Mc.y * Mc.y + Mc.z * Mc.z));
    if (dist < 0.8f * max_dist[i] || dist > 1.2f * max_dist[i]) continue;
    const V3 Sc = to_camera(R, t, S);
    if (Sc.z < 0.0f) continue;
    const V3 Ec = to_camera(R, t, E);
    if (Ec.z < 0.0f) continue;
    o[4] = 1.0f / Sc.z; o[0] = K[0] * Sc.x / Sc.z + K[2]; o[1] = K[1] * Sc.y / Sc.z + K[3];
    if (outside(b, o[0], o[1])) continue;
    o[5] = 1.0f / Ec.z; o[2] = K[0] * Ec.x / Ec.z + K[2]; o[3] = K[1] * Ec.y / Ec.z + K[3];
    if (outside(b, o[2], o[3])) continue;
    lv[i] = 1;
  }
}
