// A key frame resident in HBM (plvs_keyframe of plvs_hip.h): everything the key-frame-side searches read of a KeyFrame that its
// constructor fixes — key points or key lines, octaves, right coordinates, descriptors, the grid, the level tables, the camera and the
// bounds — copied once.  The pose (bundle adjustment moves it) and which features carry a map point (`skip`) travel with each call.
//
// ONE block, two copies of it: `host` (always) and `dev` (unless PLVS_KEYFRAME_HOST_ONLY), the same bytes at the same offsets, every
// array 16-byte aligned.  The host copy serves the pairs the device hands back (predict_level's and theta's ambiguous marks), the
// launch-free shapes and the _kf_host entries; the grids in it are built on the host at creation (the line grid needs the host's
// atan2f, the point grid has to exist on the host anyway).  Immutable after creation: any number of threads may read it at once.
// Internal: orb_fuse.hip fills and reads the point side (ResidentPoints), line_fuse.hip the line side (ResidentLines), keyframe_resident.hip owns the life cycle.
#pragma once
#include <vector>

#include "common.hpp"
#include "fuse_pair.hpp"
#include "line_fuse_pair.hpp"

struct plvs_keyframe {
  uint32_t flags = 0;
  int device = -1;             // hipGetDevice() at creation; -1: host only
  std::vector<char> host;      // the block
  char* dev = nullptr;         // its copy in HBM, host.size() bytes
  struct Points {              // offsets into the block; the grid is orbwin::FrameGrid's (members in enumeration order, CSR cell starts)
    bool present = false;
    plvs::fusepair::KfConst c; // q, t, Ow left at 0: the call's pose goes there
    int n = 0, n_levels = 0;
    size_t o_mem = 0, o_start = 0, o_ur = 0, o_desc = 0, o_sf = 0, o_sig = 0;
  } pt;
  struct Lines {               // the grid is linefuse::Grid's; the members carry the key lines' end points and right coordinates
    bool present = false;
    plvs::linefuse::KfConst c; // R, t, Ow left at 0
    int n = 0, n_members = 0, n_levels = 0;
    size_t o_mem = 0, o_start = 0, o_desc = 0, o_sf = 0, o_sig = 0;
  } ln;
  struct Bow {                 // mFeatVec and the angles (bow_search_pair.hpp): offsets rebased to 0, index holds the listed features alone
    bool present = false;
    int nnodes = 0, listed = 0, longest = 0;
    size_t o_node = 0, o_off = 0, o_idx = 0, o_angle = 0, bytes = 0;
  } bow;
};

namespace plvs {
namespace kfhandle {

// appends `bytes` of src (may be null with bytes == 0) at the next multiple of 16; -> its offset
inline size_t put(std::vector<char>* block, const void* src, size_t bytes) {
  const size_t at = (block->size() + 15) & ~(size_t)15;
  block->resize(at + bytes);
  if (bytes) memcpy(block->data() + at, src, bytes);
  return at;
}

// what create refuses of one side (the per-key-frame part of the searches' own refusals; need_pose = false: the pose pointers of
// the struct are not looked at), and the side's arrays appended to the handle's block.  No HIP call.
int check_point_keyframe(const plvs_fuse_keyframe& kf, bool need_pose);
int check_line_keyframe(const plvs_line_fuse_keyframe& kf, bool need_pose);
void stage_points(const plvs_fuse_keyframe& kf, plvs_keyframe* h);
void stage_lines(const plvs_line_fuse_keyframe& kf, plvs_keyframe* h);
// the BoW side over the point side's n key points (orb_bow_search.hip): the refusals (-> the listed features and the longest node
// list), and the side appended to the block — after stage_points
int check_bow(const plvs_keyframe_bow& bow, int n, int* listed, int* longest);
void stage_bow(const plvs_keyframe_bow& bow, int listed, int longest, plvs_keyframe* h);

}  // namespace kfhandle
}  // namespace plvs
