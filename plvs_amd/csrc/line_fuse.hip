// The search stage of LineMatcher::Fuse(pKF, vpMapLines, th, bRight = false) (reference src/LineMatcher.cc:2043-2276) as
// LocalMapping::SearchInNeighbors calls it (src/LocalMapping.cc:1434-1470): K key frames x M map lines in ONE call — one copy in,
// one launch, one wait.  Single-camera pinhole key frames only (NlinesLeft == -1, no mpCamera2).
//
// A pair's result depends on nobody else's.  A wave takes one (key frame, line) pair; the projection and the tests of
// line_fuse_pair.hpp are uniform across it and a rejected pair leaves at once; an accepted pair walks the one or two sub-windows
// of KeyFrame::GetLineFeaturesInArea on the (theta, d) grid — the rows of a column are one contiguous CSR range — in 64-member
// strides, every lane keeping the smallest (distance, enumeration position) it has seen; one cross-lane minimum, and lane 0 posts
// the pair's record straight into the pinned block.  No candidate list, no spill.
//
// The level needs the host's logarithm (track_level.hpp) and theta the host's arctangent (line_fuse_pair.hpp): the pairs either
// rule marks ambiguous are evaluated once more by the host entry's code after the wait, and their result is simply the host's.
//
// Map mutation (AddObservation, AddMapLine, Replace) stays the caller's: INTEGRATION.md has the replay.
//
// The Sim3 overload of LoopClosing::SearchAndFuse (src/LineMatcher.cc:2321-2561, line_fuse_pair.hpp's kGateSim3) runs over resident
// key frames only, by the resident kernel with the other gate: there are few lines, and the front is the larger part of the work.
#include <cmath>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "fuse_jobs.hpp"
#include "keyframe_handle.hpp"
#include "line_fuse_pair.hpp"
#include "line_fuse_tables.hpp"

namespace {

namespace lf = plvs::linefuse;
namespace fj = plvs::fusejob;
using lf::Front;
using lf::KfConst;
using lf::Member;
using plvs::linefusetab::arrays_at;
using plvs::linefusetab::FuseLines;
using plvs::linefusetab::KfArrays;
using plvs::linefusetab::KfRes;
using plvs::linefusetab::kPosBits;

constexpr int kMaxLevels = 64;

// one key frame in the staged block: the constants and where its arrays start (bytes from the block's start)
struct KfDev {
  KfConst k;
  int n_members, pad;
  unsigned long long o_mem, o_start, o_desc, o_sf, o_sig;
};

// the record a pair posts: best_idx, and best_dist (16 bits, 0xffff = -1) | reached << 16 | ambiguous << 24
__host__ __device__ inline int2 pack(int best_idx, int best_dist, int reached, int ambiguous) {
  return make_int2(best_idx, (best_dist & 0xffff) | (reached << 16) | (ambiguous << 24));
}

// One wave, one pair past front(): theta's plan and its ambiguity, the walk of the one or two sub-windows in 64-member strides, the
// gates, the (distance, enumeration position) key, the cross-lane minimum and the posted record.  ONE text: the staged kernel and
// the resident kernel both call it.
template <lf::Gate kGate>
__device__ __forceinline__ void walk_pair(const KfConst& K, const KfArrays& A, const FuseLines& L, int i, const Front& f, float th, int lane,
                                          int2* __restrict__ rec) {
  if (f.reached != lf::kEmptyWindow) {
    if (lane == 0) *rec = pack(-1, -1, f.reached, 0);
    return;
  }
  // :2124-2127 and the head of GetLineFeaturesInArea, uniform across the wave
  const float scale = A.sf[f.level];
  const float dtheta = (float)(10 * lf::kPi / 180.f) * scale;
  const float dd = th * 100.0f * scale;
  const float theta = lf::theta_device(f.rep);
  const lf::ThetaPlan plan = lf::theta_plan(K, theta, dtheta);
  const int ambiguous = (f.ambiguous || plan.nested || lf::theta_ambiguous(K, theta, dtheta, plan)) ? 1 : 0;
  if (ambiguous || plan.full || A.n_members == 0) {   // (the host decides; the refusal; nothing to walk)
    if (lane == 0) *rec = pack(-1, -1, plan.full ? lf::kFullTheta : lf::kEmptyWindow, ambiguous);
    return;
  }
  const Member* members = A.members;
  const int* start = A.start;
  const uint4* desc = A.desc;
  const float* sig = A.sig;
  const uint4 qa = L.desc[2 * (size_t)i], qb = L.desc[2 * (size_t)i + 1];
  const lf::Rep rr = kGate == lf::kGateSE3 ? lf::right_rep(K, f) : lf::Rep{0.0f, 0.0f, 0.0f};
  const float dmin = f.rep.d - dd, dmax = f.rep.d + dd;
  uint32_t best = 0xffffffffu;
  int best_idx = -1;
  bool gated = false;
  uint32_t pos0 = 0;   // enumeration position of the range's first member; it runs on across the sub-windows
  for (int s = 0; s < plan.n; ++s) {
    const lf::Cells c = lf::leaf_cells(K, lf::plan_leaf(plan, s, dmin, dmax));
    if (!c.ok) continue;
    for (int ix = c.c0; ix <= c.c1; ++ix) {   // c0 >= 0, c1 <= kCols - 1, 0 <= r0, r1 <= kRows - 1: inside the kCols * kRows + 1 starts
      const int a = start[ix * lf::kRows + c.r0], e = start[ix * lf::kRows + c.r1 + 1];
      for (int j = a + lane; j < e; j += 64) {
        const Member mb = members[j];
        if (!lf::candidate_gate<kGate>(f.rep, rr, f.level, mb, sig)) continue;
        gated = true;
        const uint4 ta = desc[2 * (size_t)mb.idx], tb = desc[2 * (size_t)mb.idx + 1];
        const uint32_t d = __popc(qa.x ^ ta.x) + __popc(qa.y ^ ta.y) + __popc(qa.z ^ ta.z) + __popc(qa.w ^ ta.w) +
                           __popc(qb.x ^ tb.x) + __popc(qb.y ^ tb.y) + __popc(qb.z ^ tb.z) + __popc(qb.w ^ tb.w);
        const uint32_t key = (d << kPosBits) | (pos0 + (uint32_t)(j - a));
        if (key < best) { best = key; best_idx = mb.idx; }
      }
      if (e > a) pos0 += (uint32_t)(e - a);
    }
  }
  // one reduction: the smallest key is the first minimum in enumeration order; keys are distinct
  uint32_t lowest = best;
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)lowest, off);
    lowest = o < lowest ? o : lowest;
  }
  const unsigned long long has_gated = __ballot(gated);
  const unsigned long long owner = __ballot(gated && best == lowest);
  int win_idx = -1;
  if (owner) win_idx = __shfl(best_idx, __ffsll((long long)owner) - 1);
  if (lane == 0) {
    int reached = lf::kEmptyWindow, idx = -1, dist = -1;
    if (pos0 > 0) {   // vIndices is not empty
      const int d = (int)(lowest >> kPosBits);
      reached = !has_gated ? lf::kNoCandidate : (d <= lf::kThLow ? lf::kCandidate : lf::kAboveThLow);
      if (reached == lf::kCandidate) { idx = win_idx; dist = d; }
    }
    *rec = pack(idx, dist, reached, 0);
  }
}

__global__ __launch_bounds__(256) void line_fuse_window_kernel(const char* __restrict__ base, const KfDev* __restrict__ kfs, FuseLines L, float th,
                                                               int2* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int pair = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= L.n_pairs) return;
  const int k = pair / L.m, i = pair - k * L.m;
  if (L.skip && L.skip[pair]) {
    if (lane == 0) out[pair] = pack(-1, -1, lf::kSkipped, 0);
    return;
  }
  const KfDev& D = kfs[k];
  const Front f = lf::front(D.k, L.start + 3 * (size_t)i, L.end + 3 * (size_t)i, L.normal + 3 * (size_t)i, L.max_dist[i]);
  const KfArrays A{reinterpret_cast<const Member*>(base + D.o_mem), reinterpret_cast<const int*>(base + D.o_start),
                   reinterpret_cast<const uint4*>(base + D.o_desc), reinterpret_cast<const float*>(base + D.o_sf),
                   reinterpret_cast<const float*>(base + D.o_sig), D.n_members};
  walk_pair<lf::kGateSE3>(D.k, A, L, i, f, th, lane, out + pair);
}

// The resident layout: the table holds pointers into the handles' own allocations (keyframe_handle.hpp), nothing of a key frame is in
// the call's block.  The pair index is the wave's: taken through readfirstlane, so the compiler knows it uniform and the pair's table
// entry — pose, constants, pointers — is read by scalar loads and stays in scalar registers.
template <lf::Gate kGate>
__global__ __launch_bounds__(256) void line_fuse_window_resident_kernel(const KfRes* __restrict__ kfs, FuseLines L, float th, int2* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int pair = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (pair >= L.n_pairs) return;
  const int k = pair / L.m, i = pair - k * L.m;
  if (L.skip && L.skip[pair]) {
    if (lane == 0) out[pair] = pack(-1, -1, lf::kSkipped, 0);
    return;
  }
  const KfRes& D = kfs[k];
  const Front f = lf::front(D.k, L.start + 3 * (size_t)i, L.end + 3 * (size_t)i, L.normal + 3 * (size_t)i, L.max_dist[i]);
  walk_pair<kGate>(D.k, D.a, L, i, f, th, lane, out + pair);
}

// pose = false: a handle's constants, the pose left at 0 (a resident call puts its own there)
KfConst kf_const(const plvs_line_fuse_keyframe& kf, bool pose = true) {
  KfConst c;
  for (int i = 0; i < 9; ++i) c.R[i] = pose ? kf.Rcw[i] : 0.0f;
  for (int i = 0; i < 3; ++i) { c.t[i] = pose ? kf.tcw[i] : 0.0f; c.Ow[i] = pose ? kf.Ow[i] : 0.0f; }
  c.fx = kf.K4[0]; c.fy = kf.K4[1]; c.cx = kf.K4[2]; c.cy = kf.K4[3];
  c.mbf = kf.view.bf;
  c.min_x = kf.bounds4[0]; c.max_x = kf.bounds4[1]; c.min_y = kf.bounds4[2]; c.max_y = kf.bounds4[3];
  c.diag = (float)(int)kf.view.max_diag;                             // KeyFrame::mnMaxDiag is an int (src/KeyFrame.cc:144)
  c.theta_inv = (float)lf::kRows / (float)M_PI;                      // mfLineGridElementThetaInv, src/Frame.cc:264
  c.d_inv = (float)lf::kCols / (2.0f * kf.view.max_diag);            // mfLineGridElementDInv, :265
  c.log_scale_factor = kf.line_log_scale_factor;
  c.n_levels = kf.n_line_levels;
  return c;
}

void make_grid(const plvs_line_fuse_keyframe& kf, const KfConst& c, lf::Grid* g) {
  const plvs_keyline* kl = kf.view.keylines_un;
  lf::build_grid(kf.view.n, [kl](int i) { return lf::KeyLineIn{kl[i].startPointX, kl[i].startPointY, kl[i].endPointX, kl[i].endPointY, kl[i].octave}; },
                 kf.view.u_right_start, kf.view.u_right_end, kf.view.max_diag, c.theta_inv, c.d_inv, 0, g);
}

// the refusals of every entry that are not a key frame's: before anything is launched or written
int check_call(const void* kfs, int n_kfs, const plvs_fuse_lines* L, float th, const int32_t* best_idx, const int32_t* best_dist) {
  return fj::check_common(kfs, n_kfs, L ? L->m : -1, L && L->start && L->end && L->normal && L->max_dist && L->desc, th, best_idx, best_dist,
                          "null lines / negative size", "null map line array");
}

const char* const kFullThetaMessage =
    "GetLineFeaturesInArea: search over the full theta interval (deltaTheta above pi / 2: the reference terminates here)";

// One call's line search as a part of the staging block (fuse_jobs.hpp): everything that depends on the query and the outputs
// alone.  Where a key frame comes from is its source's, one of the two subclasses below:
// [the source's key-frame table | lines | skip | what else the source stages] copied in one piece, [records, posted into the pinned side]
struct LinePart : fj::Part {
  const int n_kfs;
  const plvs_fuse_lines* const L;
  const uint8_t* const skip;
  const float th;
  int32_t *const best_idx, *const best_dist;
  uint8_t* const reached;
  int32_t* const stats;
  const int n_stats;   // 4: the source writes stats[3], the bytes it put into the call's copy in
  lf::Gate gate = lf::kGateSE3;   // kGateSim3: the loop-closing overload (a resident source's)

  std::vector<lf::Result> results;   // held back: a full-theta pair refuses the call before anything is written
  size_t o_tab = 0, o_start = 0, o_end = 0, o_nrm = 0, o_maxd = 0, o_desc = 0, o_skip = 0;   // from the part's inputs
  int st_host = 0;

  LinePart(int n_kfs_, const plvs_fuse_lines* L_, const uint8_t* skip_, float th_, int32_t* best_idx_, int32_t* best_dist_, uint8_t* reached_,
           int32_t* stats_, int n_stats_)
      : n_kfs(n_kfs_), L(L_), skip(skip_), th(th_), best_idx(best_idx_), best_dist(best_dist_), reached(reached_), stats(stats_),
        n_stats(n_stats_) {}

  // ---- the key-frame source
  virtual bool has_lines(int k) const = 0;
  virtual void prepare_host() = 0;                // what host_pair needs whether or not anything is launched
  virtual size_t table_entry() const = 0;         // bytes of one key frame in the table at o_tab
  virtual void size_kfs(fj::Take&) {}             // only when something is launched: what the source stages behind the query
  virtual void fill_kfs(char* p) = 0;             // the table and what size_kfs took; p: the part's inputs in the pinned block
  virtual void launch_kfs(char* dev, const char* table, const FuseLines& FL, int2* rec, hipStream_t stream) = 0;
  virtual lf::Result host_pair(int k, int i) = 0;   // one pair on the host: pair_host() over the source's grid and constants

  lf::Result pair_host(const lf::KfGrid& G, const KfConst& c, int i) const {
    return lf::pair_host(c, G, L->start + 3 * (size_t)i, L->end + 3 * (size_t)i, L->normal + 3 * (size_t)i, L->max_dist[i], L->desc + 32 * (size_t)i,
                         th, 0, 0, gate);
  }

  size_t n_pairs() const { return (size_t)n_kfs * L->m; }

  void prepare() override {
    const size_t m = (size_t)L->m;
    prepare_host();
    // anything for the device?  a pair that is not skipped, and a key frame that has key lines
    bool any_lines = false;
    for (int k = 0; k < n_kfs && !any_lines; ++k) any_lines = has_lines(k);
    device = any_lines && fj::any_unskipped(skip, n_pairs()) && !on_host;
    if (!device) return;
    fj::Take take;
    o_tab = take(table_entry() * (size_t)n_kfs);
    o_start = take(sizeof(float) * 3 * m); o_end = take(sizeof(float) * 3 * m); o_nrm = take(sizeof(float) * 3 * m);
    o_maxd = take(sizeof(float) * m); o_desc = take(m * 32);
    o_skip = take(skip ? n_pairs() : 0);
    size_kfs(take);
    in_bytes = take.at;
    out_bytes = fj::up16(sizeof(int2) * n_pairs());
  }

  void fill(char* pinned) override {
    const size_t m = (size_t)L->m;
    char* p = pinned + in_at;
    memcpy(p + o_start, L->start, sizeof(float) * 3 * m);
    memcpy(p + o_end, L->end, sizeof(float) * 3 * m);
    memcpy(p + o_nrm, L->normal, sizeof(float) * 3 * m);
    memcpy(p + o_maxd, L->max_dist, sizeof(float) * m);
    memcpy(p + o_desc, L->desc, m * 32);
    if (skip) memcpy(p + o_skip, skip, n_pairs());
    fill_kfs(p);
  }

  int launch(char* dev, char* pinned, hipStream_t stream) override {
    const char* d = dev + in_at;
    const FuseLines FL{reinterpret_cast<const float*>(d + o_start), reinterpret_cast<const float*>(d + o_end),
                       reinterpret_cast<const float*>(d + o_nrm), reinterpret_cast<const float*>(d + o_maxd),
                       reinterpret_cast<const uint4*>(d + o_desc), skip ? reinterpret_cast<const uint8_t*>(d + o_skip) : nullptr,
                       L->m, (int)n_pairs()};
    launch_kfs(dev, d + o_tab, FL, reinterpret_cast<int2*>(pinned + out_at), stream);
    PLVS_KERNEL_CHECK();
    ++launches;
    return PLVS_OK;
  }

  void host_all() override {
    const int m = L->m;
    results.resize(n_pairs());
    for (int k = 0; k < n_kfs; ++k)
      for (int i = 0; i < m; ++i) {
        const size_t pair = (size_t)k * m + i;
        results[pair] = (skip && skip[pair]) ? lf::Result{-1, -1, lf::kSkipped} : host_pair(k, i);
      }
  }

  void collect(const char* pinned) override {
    const int m = L->m, K = n_kfs;
    const int2* rec = reinterpret_cast<const int2*>(pinned + out_at);
    results.resize(n_pairs());
    lf::Result* res_out = results.data();
    int host = 0;
    for (int k = 0; k < K; ++k)
      for (int i = 0; i < m; ++i) {
        const size_t pair = (size_t)k * m + i;
        const fj::Record r = fj::unpack(rec[pair]);
        lf::Result res{r.idx, r.dist, r.reached};
        if (r.ambiguous) {   // the level or theta is the host's to decide: the pair once more, by the host entry's code
          res = host_pair(k, i);
          ++host;
        }
        res_out[pair] = res;
      }
    st_host += host;
  }

  int refused() override {   // nothing is written when a pair asks for the full theta interval
    for (const lf::Result& r : results)
      if (r.reached == lf::kFullTheta) {
        plvs::set_error("invalid argument: %s", kFullThetaMessage);
        return PLVS_ERR_INVALID_ARG;
      }
    return PLVS_OK;
  }

  void post() override {
    int windows = 0;   // pairs that reached the window
    for (size_t p = 0; p < results.size(); ++p) {
      best_idx[p] = results[p].best_idx;
      best_dist[p] = results[p].best_dist;
      if (reached) reached[p] = (uint8_t)results[p].reached;
      if (results[p].reached >= lf::kEmptyWindow) ++windows;
    }
    if (!stats) return;
    stats[0] = st_host; stats[1] = windows; stats[2] = launches;
    if (n_stats == 4) stats[3] = fj::copy_in_stat(*this);
  }
};

// Key frames staged per call: the grids and constants built always (host_all reads them), a KfDev table, and behind the query every
// key frame's members, cell starts, descriptors and levels
struct StagedLines : LinePart {
  const plvs_line_fuse_keyframe* const kfs;
  std::vector<lf::Grid> grids;
  std::vector<KfDev> tab;

  StagedLines(const plvs_line_fuse_keyframe* kfs_, int n_kfs_, const plvs_fuse_lines* L_, const uint8_t* skip_, float th_, int32_t* best_idx_,
              int32_t* best_dist_, uint8_t* reached_, int32_t* stats_)
      : LinePart(n_kfs_, L_, skip_, th_, best_idx_, best_dist_, reached_, stats_, 3), kfs(kfs_) {}

  bool has_lines(int k) const override { return kfs[k].view.n > 0; }
  size_t table_entry() const override { return sizeof(KfDev); }

  void prepare_host() override {
    grids.resize((size_t)n_kfs);
    tab.resize((size_t)n_kfs);
    for (int k = 0; k < n_kfs; ++k) {
      tab[k].k = kf_const(kfs[k]);
      make_grid(kfs[k], tab[k].k, &grids[k]);
      tab[k].n_members = (int)grids[k].members.size();
      tab[k].pad = 0;
    }
  }

  void size_kfs(fj::Take& take) override {
    for (int k = 0; k < n_kfs; ++k) {
      KfDev& D = tab[k];
      D.o_mem = take(sizeof(Member) * (size_t)D.n_members);
      D.o_start = take(D.n_members ? sizeof(int) * grids[k].start.size() : 0);
      D.o_desc = take(D.n_members ? (size_t)kfs[k].view.n * 32 : 0);
      D.o_sf = take(sizeof(float) * (size_t)kfs[k].n_line_levels);
      D.o_sig = take(sizeof(float) * (size_t)kfs[k].n_line_levels);
    }
  }

  void fill_kfs(char* p) override {
    std::vector<KfDev> abs_tab = tab;   // the kernel reads a key frame's arrays at offsets from the BLOCK's start
    for (KfDev& D : abs_tab) { D.o_mem += in_at; D.o_start += in_at; D.o_desc += in_at; D.o_sf += in_at; D.o_sig += in_at; }
    memcpy(p + o_tab, abs_tab.data(), sizeof(KfDev) * (size_t)n_kfs);
    for (int k = 0; k < n_kfs; ++k) {
      const KfDev& D = tab[k];
      const plvs_line_fuse_keyframe& kf = kfs[k];
      if (D.n_members) {
        memcpy(p + D.o_mem, grids[k].members.data(), sizeof(Member) * (size_t)D.n_members);
        memcpy(p + D.o_start, grids[k].start.data(), sizeof(int) * grids[k].start.size());
        memcpy(p + D.o_desc, kf.view.descriptors, (size_t)kf.view.n * 32);
      }
      memcpy(p + D.o_sf, kf.view.line_scale_factors, sizeof(float) * (size_t)kf.n_line_levels);
      memcpy(p + D.o_sig, kf.view.line_inv_level_sigma2, sizeof(float) * (size_t)kf.n_line_levels);
    }
  }

  void launch_kfs(char* dev, const char* table, const FuseLines& FL, int2* rec, hipStream_t stream) override {
    hipLaunchKernelGGL(line_fuse_window_kernel, dim3(plvs::ceil_div(n_pairs(), 4)), dim3(256), 0, stream, dev,
                       reinterpret_cast<const KfDev*>(table), FL, th, rec);
  }

  lf::Result host_pair(int k, int i) override {
    const plvs_line_frame_view& v = kfs[k].view;
    return pair_host({grids[k].start.data(), grids[k].members.data(), v.descriptors, v.line_scale_factors, v.line_inv_level_sigma2}, tab[k].k, i);
  }
};

// ---------------------------------------------------------------------------------------------------- resident key frames
// Key frames resident in HBM (keyframe_handle.hpp): a KfRes table — pose, constants, pointers into the handles' allocations — and
// nothing else.  Nothing of a key frame is built, staged or copied.
struct ResidentLines : LinePart {
  const plvs_keyframe* const* const kfs;
  const plvs_keyframe_pose* const poses;          // the SE3 search's
  const plvs_keyframe_sim3_pose* const sim3;      // the Sim3 search's (one of the two is null)
  std::vector<KfConst> consts;   // per listed key frame: the handle's constants with the call's pose

  ResidentLines(const plvs_keyframe* const* kfs_, const plvs_keyframe_pose* poses_, const plvs_keyframe_sim3_pose* sim3_, int n_kfs_,
                const plvs_fuse_lines* L_, const uint8_t* skip_, float th_, int32_t* best_idx_, int32_t* best_dist_, uint8_t* reached_,
                int32_t* stats_)
      : LinePart(n_kfs_, L_, skip_, th_, best_idx_, best_dist_, reached_, stats_, 4), kfs(kfs_), poses(poses_), sim3(sim3_) {
    if (sim3) gate = lf::kGateSim3;
  }

  bool has_lines(int k) const override { return kfs[k]->ln.n > 0; }
  size_t table_entry() const override { return sizeof(KfRes); }

  void prepare_host() override {
    consts.resize((size_t)n_kfs);
    for (int k = 0; k < n_kfs; ++k) {
      KfConst& c = consts[k] = kfs[k]->ln.c;
      for (int i = 0; i < 9; ++i) c.R[i] = sim3 ? sim3[k].Rcw[i] : poses[k].Rcw[i];
      for (int i = 0; i < 3; ++i) {
        c.t[i] = sim3 ? sim3[k].tcw[i] : poses[k].tcw[i];
        c.Ow[i] = sim3 ? sim3[k].Ow_lines[i] : poses[k].Ow[i];
      }
    }
  }

  void fill_kfs(char* p) override {
    KfRes* tab = reinterpret_cast<KfRes*>(p + o_tab);
    for (int k = 0; k < n_kfs; ++k) tab[k] = KfRes{consts[k], arrays_at(kfs[k]->dev, kfs[k]->ln)};
  }

  void launch_kfs(char*, const char* table, const FuseLines& FL, int2* rec, hipStream_t stream) override {
    const KfRes* tab = reinterpret_cast<const KfRes*>(table);
    const dim3 grid(plvs::ceil_div(n_pairs(), 4));
    if (sim3) hipLaunchKernelGGL(line_fuse_window_resident_kernel<lf::kGateSim3>, grid, dim3(256), 0, stream, tab, FL, th, rec);
    else hipLaunchKernelGGL(line_fuse_window_resident_kernel<lf::kGateSE3>, grid, dim3(256), 0, stream, tab, FL, th, rec);
  }

  lf::Result host_pair(int k, int i) override {   // on the handle's host copy
    const KfArrays a = arrays_at(kfs[k]->host.data(), kfs[k]->ln);
    return pair_host({a.start, a.members, reinterpret_cast<const uint8_t*>(a.desc), a.sf, a.sig}, consts[k], i);
  }
};

}  // namespace

int plvs::kfhandle::check_line_keyframe(const plvs_line_fuse_keyframe& kf, bool need_pose) {
  PLVS_REQUIRE(kf.n_cameras == 1 && kf.camera_model == PLVS_CAMERA_PINHOLE,
               "single-camera pinhole key frames only (NlinesLeft == -1, bRight == false): the fisheye / two-camera branches stay with the reference");
  PLVS_REQUIRE(kf.K4 && kf.bounds4 && (!need_pose || (kf.Rcw && kf.tcw && kf.Ow)), "null pose / camera array");
  PLVS_REQUIRE(kf.n_line_levels >= 1 && kf.n_line_levels <= kMaxLevels && kf.n_line_levels == kf.view.n_levels && kf.view.line_scale_factors &&
                   kf.view.line_inv_level_sigma2,
               "line levels outside [1, 64], different from the view's, or null level arrays");
  PLVS_REQUIRE(kf.view.max_diag > 0.0f, "mnMaxDiag not positive");
  PLVS_REQUIRE(kf.view.n >= 0 && kf.view.n < (1 << kPosBits), "key line count outside [0, 2^23)");
  PLVS_REQUIRE((kf.view.u_right_start == nullptr) == (kf.view.u_right_end == nullptr), "one of mvuRightLineStart / End without the other");
  if (kf.view.n > 0) {
    PLVS_REQUIRE(kf.view.keylines_un && kf.view.descriptors, "null key frame array");
    for (int i = 0; i < kf.view.n; ++i)
      PLVS_REQUIRE(kf.view.keylines_un[i].octave >= 0 && kf.view.keylines_un[i].octave < kf.n_line_levels,
                   "octave of a key line outside the key frame's levels");
  }
  return PLVS_OK;
}

void plvs::kfhandle::stage_lines(const plvs_line_fuse_keyframe& kf, plvs_keyframe* h) {
  plvs_keyframe::Lines& s = h->ln;
  s.present = true;
  s.c = kf_const(kf, false);
  lf::Grid grid;
  make_grid(kf, s.c, &grid);
  s.n = kf.view.n;
  s.n_members = (int)grid.members.size();
  s.n_levels = kf.n_line_levels;
  s.o_mem = put(&h->host, grid.members.data(), sizeof(Member) * grid.members.size());
  s.o_start = put(&h->host, grid.start.data(), sizeof(int) * grid.start.size());
  s.o_desc = put(&h->host, kf.view.descriptors, (size_t)kf.view.n * 32);
  s.o_sf = put(&h->host, kf.view.line_scale_factors, sizeof(float) * (size_t)kf.n_line_levels);
  s.o_sig = put(&h->host, kf.view.line_inv_level_sigma2, sizeof(float) * (size_t)kf.n_line_levels);
}

int plvs::fusejob::make_line_part_kf(const plvs_keyframe* const* kfs, const plvs_keyframe_pose* poses, int n_kfs, const plvs_fuse_lines* L,
                                     const uint8_t* skip, float th, int32_t* best_idx, int32_t* best_dist, uint8_t* reached, int32_t* stats,
                                     bool host_entry, std::unique_ptr<Part>* out, const plvs_keyframe_sim3_pose* sim3) {
  out->reset();
  int rc = check_call(kfs, n_kfs, L, th, best_idx, best_dist);
  if (rc == PLVS_OK) rc = check_handles(kfs, sim3 ? static_cast<const void*>(sim3) : poses, n_kfs, 2, host_entry);
  if (rc != PLVS_OK) return rc;
  if (n_kfs > 0 && L->m > 0) out->reset(new ResidentLines(kfs, poses, sim3, n_kfs, L, skip, th, best_idx, best_dist, reached, stats));
  return PLVS_OK;
}

int plvs::fusejob::make_line_part(const plvs_line_fuse_keyframe* kfs, int n_kfs, const plvs_fuse_lines* L, const uint8_t* skip, float th,
                                  int32_t* best_idx, int32_t* best_dist, uint8_t* reached, int32_t* stats, std::unique_ptr<Part>* out) {
  out->reset();
  int rc = check_call(kfs, n_kfs, L, th, best_idx, best_dist);
  for (int k = 0; rc == PLVS_OK && k < n_kfs; ++k) rc = plvs::kfhandle::check_line_keyframe(kfs[k], true);
  if (rc != PLVS_OK) return rc;
  if (n_kfs > 0 && L->m > 0) out->reset(new StagedLines(kfs, n_kfs, L, skip, th, best_idx, best_dist, reached, stats));
  return PLVS_OK;
}

extern "C" {

int plvs_hip_line_fuse_search(const plvs_line_fuse_keyframe* kfs, int n_kfs, const plvs_fuse_lines* L, const uint8_t* skip, float th,
                              int32_t* best_idx, int32_t* best_dist, uint8_t* reached, int32_t* stats, void* stream) {
  std::unique_ptr<fj::Part> part;
  const int rc = plvs::fusejob::make_line_part(kfs, n_kfs, L, skip, th, best_idx, best_dist, reached, stats, &part);
  return rc != PLVS_OK ? rc : fj::run_single(part.get(), stats, 3, stream, false);
}

int plvs_hip_line_fuse_search_host(const plvs_line_fuse_keyframe* kfs, int n_kfs, const plvs_fuse_lines* L, const uint8_t* skip, float th,
                                   int32_t* best_idx, int32_t* best_dist, uint8_t* reached, int32_t* stats) {
  std::unique_ptr<fj::Part> part;
  const int rc = plvs::fusejob::make_line_part(kfs, n_kfs, L, skip, th, best_idx, best_dist, reached, stats, &part);
  return rc != PLVS_OK ? rc : fj::run_single(part.get(), stats, 3, nullptr, true);
}

}  // extern "C"
