// One call, one wait for both halves of LocalMapping::SearchInNeighbors' search (reference src/LocalMapping.cc:1372-1470): the
// point search of orb_fuse.hip and the line search of line_fuse.hip share the calling thread's staging block — both parts are sized
// first, the block is reserved once, each kind fills its part at its offset — one host-to-device copy, the two kernels back to back
// on the same stream, one wait, then each kind's host pass.  The two kinds read disjoint data and the key frames' poses do not
// change in between.  run_parts also is what the two single-kind entries run, with one part.
#include "fuse_jobs.hpp"

namespace plvs {
namespace fusejob {

int run_parts(Part* a, Part* b, hipStream_t stream, bool own_stream, bool copy_only, int* launches, int* waits, size_t* copied) {
  Part* parts[2] = {a, b};
  if (launches) *launches = 0;
  if (waits) *waits = 0;
  if (copied) *copied = 0;
  size_t in_total = 0, scratch_total = 0, out_total = 0;
  bool device = false;
  for (Part* p : parts) {
    if (!p) continue;
    p->prepare();
    if (!p->device) continue;
    device = true;
    in_total += p->in_bytes;
    scratch_total += p->scratch_bytes;
    out_total += p->out_bytes;
  }
  if (device) {
    plvs::HostStage& st = plvs::thread_stage();
    PLVS_HIP_TRY(st.reserve(in_total + scratch_total + out_total + 16));
    if (own_stream) stream = st.stream;
    size_t in_at = 0, scratch_at = in_total, out_at = in_total + scratch_total;
    for (Part* p : parts) {
      if (!p || !p->device) continue;
      p->in_at = in_at;
      p->scratch_at = scratch_at;
      p->out_at = out_at;
      p->fill(st.pinned);
      in_at += p->in_bytes;
      scratch_at += p->scratch_bytes;
      out_at += p->out_bytes;
    }
    plvs::StreamGuard guard{stream};
    PLVS_HIP_TRY(hipMemcpyAsync(st.dev, st.pinned, in_total, hipMemcpyHostToDevice, stream));
    guard.armed = true;
    if (copied) *copied = in_total;
    if (!copy_only)
      for (Part* p : parts) {
        if (!p || !p->device) continue;
        const int rc = p->launch(st.dev, st.pinned, stream);
        if (rc != PLVS_OK) return rc;
        if (launches) *launches += p->launches;
      }
    PLVS_HIP_TRY(hipStreamSynchronize(stream));   // the call's one wait
    guard.armed = false;
    if (waits) *waits = 1;
    if (copy_only) return PLVS_OK;   // nothing launched, the outputs untouched
    for (Part* p : parts)
      if (p && p->device) p->collect(st.pinned);
  }
  for (Part* p : parts)
    if (p && !p->device) p->host_all();
  for (Part* p : parts) {
    if (!p) continue;
    const int rc = p->refused();
    if (rc != PLVS_OK) return rc;
  }
  for (Part* p : parts)
    if (p) p->post();
  return PLVS_OK;
}

int run_single(Part* p, int32_t* stats, int n_stats, void* stream, bool on_host, bool copy_only) {
  for (int s = 0; stats && s < n_stats; ++s) stats[s] = 0;
  if (!p) return PLVS_OK;
  p->on_host = on_host;
  return run_parts(p, nullptr, static_cast<hipStream_t>(stream), stream == nullptr, copy_only, nullptr, nullptr);
}

}  // namespace fusejob
}  // namespace plvs

extern "C" int plvs_hip_fuse_search_points_and_lines(const plvs_fuse_keyframe* point_kfs, int n_point_kfs, const plvs_fuse_points* P,
                                                     const uint8_t* skip_points, float th_points, int32_t* point_best_idx,
                                                     int32_t* point_best_dist, uint8_t* point_reached, int32_t* point_stats,
                                                     const plvs_line_fuse_keyframe* line_kfs, int n_line_kfs, const plvs_fuse_lines* L,
                                                     const uint8_t* skip_lines, float th_lines, int32_t* line_best_idx, int32_t* line_best_dist,
                                                     uint8_t* line_reached, int32_t* line_stats, int32_t* stats, void* stream) {
  PLVS_REQUIRE(P || L, "neither points nor lines");
  std::unique_ptr<plvs::fusejob::Part> points, lines;
  if (P) {   // both kinds' refusals before anything is launched or written
    const int rc = plvs::fusejob::make_point_part(point_kfs, n_point_kfs, P, skip_points, th_points, point_best_idx, point_best_dist,
                                                  point_reached, point_stats, &points);
    if (rc != PLVS_OK) return rc;
  }
  if (L) {
    const int rc = plvs::fusejob::make_line_part(line_kfs, n_line_kfs, L, skip_lines, th_lines, line_best_idx, line_best_dist, line_reached,
                                                 line_stats, &lines);
    if (rc != PLVS_OK) return rc;
  }
  if (P && point_stats) point_stats[0] = point_stats[1] = point_stats[2] = 0;
  if (L && line_stats) line_stats[0] = line_stats[1] = line_stats[2] = 0;
  if (stats) stats[0] = stats[1] = 0;
  int launches = 0, waits = 0;
  const int rc = plvs::fusejob::run_parts(points.get(), lines.get(), static_cast<hipStream_t>(stream), stream == nullptr, false, &launches, &waits);
  if (stats) { stats[0] = launches; stats[1] = waits; }
  return rc;
}
