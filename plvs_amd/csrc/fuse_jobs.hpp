// The two halves of LocalMapping::SearchInNeighbors' search — ORBmatcher::Fuse (orb_fuse.hip) and LineMatcher::Fuse
// (line_fuse.hip) — as parts of ONE call: each kind sizes its share of the calling thread's staging block, fills it at the
// offset it is given, launches its kernel, and after the call's one wait turns its records into its outputs.  run_parts
// (fuse_both.hip) drives one part (the two single-kind entries) or both (plvs_hip_fuse_search_points_and_lines):
//   [ A's inputs | B's inputs ]  one host-to-device copy      [ A's device scratch | B's ]      [ A's records | B's ]  pinned side
// Internal to the library.
#pragma once
#include <memory>

#include "common.hpp"

namespace plvs {
namespace fusejob {

struct Part {
  virtual ~Part() {}
  bool device = false;                                  // after prepare(): something is launched
  size_t in_bytes = 0, scratch_bytes = 0, out_bytes = 0;   // after prepare(), multiples of 16
  int launches = 0;
  virtual void prepare() = 0;                           // grids, sizes; no HIP call
  virtual void fill(char* pinned, size_t in_at, size_t scratch_at, size_t out_at) = 0;
  virtual int launch(char* dev, char* pinned, hipStream_t stream) = 0;
  virtual void host_all() = 0;                          // every pair by the host's code (nothing is launched for this part)
  virtual void collect(const char* pinned) = 0;         // after the wait: the records, the ambiguous pairs once more on the host
  virtual int refused() { return PLVS_OK; }             // a refusal found in the results: before ANY part writes an output
  virtual void post() = 0;                              // the outputs and stats
};

// which of its 4 stats a resident part adds to the non-resident three: the bytes it put into the call's copy in
inline int32_t copy_in_stat(const Part& p) { return p.device ? (int32_t)p.in_bytes : 0; }

// the refusals of an entry (before anything is launched or written), then its part
int make_point_part(const plvs_fuse_keyframe* kfs, int n_kfs, const plvs_fuse_points* P, const uint8_t* skip, float th, int32_t* best_idx,
                    int32_t* best_dist, uint8_t* reached, int32_t* stats, std::unique_ptr<Part>* out);
int make_line_part(const plvs_line_fuse_keyframe* kfs, int n_kfs, const plvs_fuse_lines* L, const uint8_t* skip, float th, int32_t* best_idx,
                   int32_t* best_dist, uint8_t* reached, int32_t* stats, std::unique_ptr<Part>* out);

// The same over resident key frames (keyframe_handle.hpp): key frame k = (kfs[k], poses[k]).  host_entry: the _kf_host entries
// (PLVS_KEYFRAME_HOST_ONLY handles are taken, no HIP call is made, not even for the device id).
int make_point_part_kf(const plvs_keyframe* const* kfs, const plvs_keyframe_pose* poses, int n_kfs, const plvs_fuse_points* P,
                       const uint8_t* skip, float th, int32_t* best_idx, int32_t* best_dist, uint8_t* reached, int32_t* stats, bool host_entry,
                       std::unique_ptr<Part>* out);
int make_line_part_kf(const plvs_keyframe* const* kfs, const plvs_keyframe_pose* poses, int n_kfs, const plvs_fuse_lines* L,
                      const uint8_t* skip, float th, int32_t* best_idx, int32_t* best_dist, uint8_t* reached, int32_t* stats, bool host_entry,
                      std::unique_ptr<Part>* out);
// the refusals of a handle list, in this order: a NULL handle or a handle without the side the call needs (side: 1 = points,
// 2 = lines), for a device entry a host-only handle — all before any HIP call — and then a handle of another device
int check_handles(const plvs_keyframe* const* kfs, const plvs_keyframe_pose* poses, int n_kfs, int side, bool host_entry);
// a part alone on the host (the _host entries): every pair by the host's code, the refusal, the outputs
int run_part_on_host(Part* p);

// a (and b, may be null): prepare, one reserve, fill, one copy in, the launches back to back on one stream, one wait, collect, post.
// copy_only: the staging and the copy alone (a measurement hook of the point entry).  launches / waits: may be null.
int run_parts(Part* a, Part* b, hipStream_t stream, bool own_stream, bool copy_only, int* launches, int* waits, size_t* copied = nullptr);

}  // namespace fusejob
}  // namespace plvs
