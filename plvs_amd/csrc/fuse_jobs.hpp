// The two halves of LocalMapping::SearchInNeighbors' search — ORBmatcher::Fuse (orb_fuse.hip) and LineMatcher::Fuse
// (line_fuse.hip) — as parts of ONE call: each kind sizes its share of the calling thread's staging block, fills it at the
// offset it is given, launches its kernel, and after the call's one wait turns its records into its outputs.  run_parts
// (fuse_both.hip) drives one part (the single-kind entries, through run_single) or both (plvs_hip_fuse_search_points_and_lines):
//   [ A's inputs | B's inputs ]  one host-to-device copy      [ A's device scratch | B's ]      [ A's records | B's ]  pinned side
// ONE part per kind (PointPart, LinePart); where its key frames come from — staged per call, or resident in HBM
// (keyframe_handle.hpp) — is the part's key-frame source, a small subclass.
// Internal to the library.
#pragma once
#include <memory>

#include "common.hpp"

namespace plvs {
namespace fusejob {

struct Part {
  virtual ~Part() {}
  bool on_host = false;                                 // set before prepare(): nothing is launched whatever the work (the _host entries)
  bool device = false;                                  // after prepare(): something is launched
  size_t in_bytes = 0, scratch_bytes = 0, out_bytes = 0;   // after prepare(), multiples of 16
  size_t in_at = 0, scratch_at = 0, out_at = 0;         // before fill(): the part's places in the block
  int launches = 0;
  virtual void prepare() = 0;                           // grids, sizes; no HIP call
  virtual void fill(char* pinned) = 0;
  virtual int launch(char* dev, char* pinned, hipStream_t stream) = 0;
  virtual void host_all() = 0;                          // every pair by the host's code (nothing is launched for this part)
  virtual void collect(const char* pinned) = 0;         // after the wait: the records, the ambiguous pairs once more on the host
  virtual int refused() { return PLVS_OK; }             // a refusal found in the results: before ANY part writes an output
  virtual void post() = 0;                              // the outputs and stats
};

// which of its 4 stats a resident part adds to the non-resident three: the bytes it put into the call's copy in
inline int32_t copy_in_stat(const Part& p) { return p.device ? (int32_t)p.in_bytes : 0; }

// ---- what the two kinds' parts share: textually the same on both sides, and blind to the element type
using plvs::Take;   // the allocator of a part's share of the block (common.hpp)
using plvs::up16;

// the record a pair posts (pack() of either kernel file): best_idx, and best_dist (16 bits, 0xffff = -1) | reached << 16 | ambiguous << 24
struct Record {
  int idx, dist, reached;
  bool ambiguous;   // the host decides: the pair once more by the host's code
};
inline Record unpack(const int2& r) { return Record{r.x, (int)(int16_t)(r.y & 0xffff), (r.y >> 16) & 0xff, ((r.y >> 24) & 1) != 0}; }

// is any of `count` pairs not skipped?  skip: may be null (none is)
inline bool any_unskipped(const uint8_t* skip, size_t count) {
  if (!skip) return count > 0;
  for (size_t p = 0; p < count; ++p)
    if (!skip[p]) return true;
  return false;
}

// the refusals of every entry that are not a key frame's, in their order.  m: the query's size, -1 for a null query; arrays: all of
// its arrays are there
inline int check_common(const void* kfs, int n_kfs, int m, bool arrays, float th, const int32_t* best_idx, const int32_t* best_dist,
                        const char* null_query, const char* null_array) {
  PLVS_REQUIRE(n_kfs >= 0 && m >= 0, null_query);
  PLVS_REQUIRE(best_idx && best_dist, "null output");
  PLVS_REQUIRE(n_kfs == 0 || kfs, "null key frames");
  PLVS_REQUIRE(th >= 0.0f && th <= 1.0e6f, "th outside [0, 1e6]");
  PLVS_REQUIRE((long long)n_kfs * m <= (1ll << 30), "more than 2^30 pairs");
  PLVS_REQUIRE(m == 0 || arrays, null_array);
  return PLVS_OK;
}

// the refusals of an entry (before anything is launched or written), then its part
int make_point_part(const plvs_fuse_keyframe* kfs, int n_kfs, const plvs_fuse_points* P, const uint8_t* skip, float th, int32_t* best_idx,
                    int32_t* best_dist, uint8_t* reached, int32_t* stats, std::unique_ptr<Part>* out);
int make_line_part(const plvs_line_fuse_keyframe* kfs, int n_kfs, const plvs_fuse_lines* L, const uint8_t* skip, float th, int32_t* best_idx,
                   int32_t* best_dist, uint8_t* reached, int32_t* stats, std::unique_ptr<Part>* out);

// The same over resident key frames (keyframe_handle.hpp): key frame k = (kfs[k], poses[k]).  host_entry: the _kf_host entries
// (PLVS_KEYFRAME_HOST_ONLY handles are taken, no HIP call is made, not even for the device id).  sim3: not null — the Sim3 overloads
// of loop closing (the kGateSim3 policy of the pair headers) with these poses, `poses` is not read.
int make_point_part_kf(const plvs_keyframe* const* kfs, const plvs_keyframe_pose* poses, int n_kfs, const plvs_fuse_points* P,
                       const uint8_t* skip, float th, int32_t* best_idx, int32_t* best_dist, uint8_t* reached, int32_t* stats, bool host_entry,
                       std::unique_ptr<Part>* out, const plvs_keyframe_sim3_pose* sim3 = nullptr);
int make_line_part_kf(const plvs_keyframe* const* kfs, const plvs_keyframe_pose* poses, int n_kfs, const plvs_fuse_lines* L,
                      const uint8_t* skip, float th, int32_t* best_idx, int32_t* best_dist, uint8_t* reached, int32_t* stats, bool host_entry,
                      std::unique_ptr<Part>* out, const plvs_keyframe_sim3_pose* sim3 = nullptr);
// The loop-closing SearchByProjection overloads (loop_search_pair.hpp; orb_loop_search.hip, line_loop_search.hip): the refusals,
// then the part.  Its collect() and host_all() run the greedy pass; nmatches of an empty part is the entry's to zero.
int make_loop_search_point_part(const plvs_keyframe* const* kfs, const plvs_keyframe_sim3_pose* sim3, int n_kfs, const plvs_fuse_points* P,
                                const uint8_t* skip, const uint8_t* const* occupied, float th, float ratio_hamming, int projection,
                                int32_t* match_idx, int32_t* match_dist, uint8_t* reached, int32_t* nmatches, int32_t* stats, bool host_entry,
                                std::unique_ptr<Part>* out);
int make_loop_search_line_part(const plvs_keyframe* const* kfs, const plvs_keyframe_sim3_pose* sim3, int n_kfs, const plvs_fuse_lines* L,
                               const uint8_t* skip, const uint8_t* const* occupied, float th, float ratio_hamming, int32_t* match_idx,
                               int32_t* match_dist, uint8_t* reached, int32_t* nmatches, int32_t* stats, bool host_entry,
                               std::unique_ptr<Part>* out);
// SearchByBoW over handles (orb_bow_search.hip): the refusals, then the part (null for a call without key frames; nmatches is then
// the entry's to zero).  kf1 != null: SearchByBoW(kf1, kfs[k]) with valid1 / valid[k]; else SearchByBoW(kfs[k], F) with valid[k].
int make_bow_search_part(const plvs_keyframe* kf1, const uint8_t* valid1, const plvs_keyframe* const* kfs, const uint8_t* const* valid,
                         int n_kfs, const plvs_bow_frame* F, bool frame_kind, float nn_ratio, int check_orientation, int32_t* match,
                         int32_t* match_dist, int32_t* nmatches, int32_t* stats, bool host_entry, std::unique_ptr<Part>* out);
// the refusals of a handle list, in this order: a NULL handle or a handle without the side the call needs (side: 1 = points,
// 2 = lines), for a device entry a host-only handle — all before any HIP call — and then a handle of another device
int check_handles(const plvs_keyframe* const* kfs, const void* poses, int n_kfs, int side, bool host_entry);
// A single-kind entry after its make_*: the n_stats (3, a resident part's 4) stats zeroed, nothing more for an empty part (null),
// else run_parts over the one part — on the host (the _host entries: every pair by the host's code, no HIP call) or on `stream`
// (null: the calling thread's own)
int run_single(Part* p, int32_t* stats, int n_stats, void* stream, bool on_host, bool copy_only = false);

// a (and b, may be null): prepare, one reserve, fill, one copy in, the launches back to back on one stream, one wait, collect, post.
// copy_only: the staging and the copy alone (a measurement hook of the point entry).  launches / waits: may be null.
int run_parts(Part* a, Part* b, hipStream_t stream, bool own_stream, bool copy_only, int* launches, int* waits, size_t* copied = nullptr);

}  // namespace fusejob
}  // namespace plvs
