// ORBmatcher::SearchByBoW over resident key frames (bow_search_pair.hpp): SearchByBoW(pKF1, pKF2[k]) as
// LoopClosing::DetectCommonRegionsFromBoW calls it per covisible (reference src/LoopClosing.cc:769-780), and SearchByBoW(pKF[k], F)
// as Tracking::Relocalization calls it per candidate (src/Tracking.cc:4907-4930) — one against K in one call: one reserve, one copy
// in (the table, the validity bytes, for the frame kind the frame's descriptors and vector; nothing of a key frame), one launch,
// one wait.  The whole greedy pass runs on the device; the rotation histogram and ComputeThreeMaxima (orb_window.hpp's
// three_maxima) run on the host per k after the wait.
//
// The kernel: one wave64 per (pair k, node a of the serial side), four jobs to a 256-thread workgroup, no barrier, no atomics, no
// LDS.  The wave finds its node in the lane side's ascending id list by binary search and leaves if it is absent.  A lane-side
// list of up to 64 members stays resident: lane l holds member l's descriptor (two uint4) and its open bit in registers.  A longer
// list is walked in passes of 64 per serial feature, its open bytes in the call's device scratch — position p is always lane
// p & 63's, so the byte is written and read by the same lane.  No length limit, nothing handed to the host.
// Per serial feature: every lane's key is dist << 23 | list position (kNoKey where closed); a wave minimum gives bestDist1 and the
// FIRST minimum in list order, a second one over the other lanes' best and the winner lane's runner-up gives bestDist2 (equal
// distances count as two, as `else if(dist<bestDist2)` does).  The winner's lane closes its member and posts the record.
#include <cstring>
#include <vector>

#include "bow_search_pair.hpp"
#include "common.hpp"
#include "fuse_jobs.hpp"
#include "keyframe_handle.hpp"
#include "orb_window.hpp"

namespace {

namespace bs = plvs::bowsearch;
namespace fj = plvs::fusejob;
using plvs::orbwin::kHistoLength;

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, m, 64));
  return v;
}

__device__ __forceinline__ uint32_t hamming(const uint4& qa, const uint4& qb, const uint4& ta, const uint4& tb) {
  return __popc(qa.x ^ ta.x) + __popc(qa.y ^ ta.y) + __popc(qa.z ^ ta.z) + __popc(qa.w ^ ta.w) +
         __popc(qb.x ^ tb.x) + __popc(qb.y ^ tb.y) + __popc(qb.z ^ tb.z) + __popc(qb.w ^ tb.w);
}

// grid (ceil(max serial nodes / 4), n pairs).  Every serial-side list position of every pair is written by exactly one wave.
template <bool kFrameKind>
__global__ __launch_bounds__(256) void bow_search_kernel(const bs::Pair* __restrict__ tab, float nn_ratio, int2* __restrict__ rec,
                                                         uint8_t* gates) {
  const int lane = threadIdx.x & 63;
  const bs::Side S = tab[blockIdx.y].s, L = tab[blockIdx.y].l;   // by value: the stores below cannot alias them
  const int rec_at = tab[blockIdx.y].rec_at, gate_at = tab[blockIdx.y].gate_at;
  const int a = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (a >= S.nnodes) return;
  const int s0 = __builtin_amdgcn_readfirstlane(S.off[a]), s1 = __builtin_amdgcn_readfirstlane(S.off[a + 1]);
  int2* R = rec + rec_at;                      // s0 <= p < s1 <= the pair's listed features: inside its records
  const uint32_t node = S.node_id[a];
  const int b = __builtin_amdgcn_readfirstlane(bs::lower_bound(L.node_id, L.nnodes, node));
  if (b == L.nnodes || L.node_id[b] != node) {
    for (int p = s0 + lane; p < s1; p += 64) R[p] = bs::not_evaluated();
    return;
  }
  const int l0 = __builtin_amdgcn_readfirstlane(L.off[b]), len = __builtin_amdgcn_readfirstlane(L.off[b + 1]) - l0;
  const uint32_t* lidx = L.idx + l0;           // q < len: inside the lane side's list
  if (len <= 64) {
    const bool have = lane < len;
    const uint32_t mine = have ? lidx[lane] : 0u;
    bool open = have && (!L.valid || L.valid[mine] != 0);
    uint4 ta = make_uint4(0, 0, 0, 0), tb = ta;
    if (have) { ta = L.desc[2 * (size_t)mine]; tb = L.desc[2 * (size_t)mine + 1]; }
    for (int p = s0; p < s1; ++p) {
      const uint32_t i1 = S.idx[p];
      if (!S.valid[i1]) {                      // wave-uniform
        if (lane == 0) R[p] = bs::not_evaluated();
        continue;
      }
      const uint4 qa = S.desc[2 * (size_t)i1], qb = S.desc[2 * (size_t)i1 + 1];
      const uint32_t key = open ? (hamming(qa, qb, ta, tb) << bs::kPosBits) | (uint32_t)lane : bs::kNoKey;
      const uint32_t m1 = wave_min(key);
      const uint32_t m2 = wave_min(key == m1 ? bs::kNoKey : key);
      const int d1 = (int)(m1 >> bs::kPosBits), d2 = (int)(m2 >> bs::kPosBits);
      const bool accept = bs::accepts<kFrameKind>(d1, d2, nn_ratio);
      const int writer = accept ? (int)(m1 & 63u) : 0;   // an accepted key is a member's: its position is below len <= 64
      if (lane == writer) {
        R[p] = bs::pack(accept ? (int)mine : -1, d1, d2);
        if (accept) open = false;
      }
    }
    return;
  }
  uint8_t* G = gates + gate_at + l0;           // len bytes, this job's alone
  for (int q = lane; q < len; q += 64) G[q] = L.valid ? L.valid[lidx[q]] != 0 : 1;
  for (int p = s0; p < s1; ++p) {
    const uint32_t i1 = S.idx[p];
    if (!S.valid[i1]) {
      if (lane == 0) R[p] = bs::not_evaluated();
      continue;
    }
    const uint4 qa = S.desc[2 * (size_t)i1], qb = S.desc[2 * (size_t)i1 + 1];
    uint32_t k1 = bs::kNoKey, k2 = bs::kNoKey;
    for (int q = lane; q < len; q += 64) {
      if (!G[q]) continue;
      const uint32_t j = lidx[q];
      const uint32_t key = (hamming(qa, qb, L.desc[2 * (size_t)j], L.desc[2 * (size_t)j + 1]) << bs::kPosBits) | (uint32_t)q;
      if (key < k1) { k2 = k1; k1 = key; }
      else if (key < k2) k2 = key;
    }
    const uint32_t m1 = wave_min(k1);
    const uint32_t m2 = wave_min(k1 == m1 ? k2 : k1);
    const int d1 = (int)(m1 >> bs::kPosBits), d2 = (int)(m2 >> bs::kPosBits);
    const bool accept = bs::accepts<kFrameKind>(d1, d2, nn_ratio);
    const int won = (int)(m1 & ((1u << bs::kPosBits) - 1u));   // read only if accepted: then a member's position, below len
    if (lane == (accept ? (won & 63) : 0)) {
      R[p] = bs::pack(accept ? (int)lidx[won] : -1, d1, d2);
      if (accept) G[won] = 0;
    }
  }
}

bs::Side handle_side(const plvs_keyframe& h, const char* block, const uint8_t* valid) {
  return bs::Side{reinterpret_cast<const uint32_t*>(block + h.bow.o_node), reinterpret_cast<const int32_t*>(block + h.bow.o_off),
                  reinterpret_cast<const uint32_t*>(block + h.bow.o_idx), reinterpret_cast<const uint4*>(block + h.pt.o_desc), valid,
                  h.bow.nnodes};
}
const float* handle_angle(const plvs_keyframe& h) { return reinterpret_cast<const float*>(h.host.data() + h.bow.o_angle); }

bool any_set(const uint8_t* v, int n) {
  for (int i = 0; i < n; ++i)
    if (v[i]) return true;
  return false;
}

// The call as a part of the staging block (fuse_jobs.hpp): [table | validity bytes | the frame's descriptors and vector] copied
// in one piece, [gate bytes] device scratch, [records] posted into the pinned side.
struct BowSearch : fj::Part {
  const plvs_keyframe* const kf1;
  const uint8_t* const valid1;
  const plvs_keyframe* const* const kfs;
  const uint8_t* const* const valid;
  const int n_kfs;
  const plvs_bow_frame* const F;
  const bool frame_kind;
  const float nn_ratio;
  const int check_orientation;
  int32_t* const match;
  int32_t* const match_dist;
  int32_t* const nmatches;
  int32_t* const stats;
  std::vector<int32_t> f_off;                 // the frame's offsets from 0
  std::vector<bs::Pair> host_tab;             // on host pointers: what the host twin and the collection read
  std::vector<int2> host_rec;
  std::vector<size_t> o_valid;
  size_t o_tab = 0, o_valid1 = 0, o_fdesc = 0, o_fnode = 0, o_foff = 0, o_fidx = 0;
  int n_rec = 0, n_gate = 0, max_serial_nodes = 0, f_listed = 0;
  bs::JobCounts jobs;

  BowSearch(const plvs_keyframe* kf1_, const uint8_t* valid1_, const plvs_keyframe* const* kfs_, const uint8_t* const* valid_, int n_kfs_,
            const plvs_bow_frame* F_, bool frame_kind_, float nn_ratio_, int check_orientation_, int32_t* match_, int32_t* match_dist_,
            int32_t* nmatches_, int32_t* stats_)
      : kf1(kf1_), valid1(valid1_), kfs(kfs_), valid(valid_), n_kfs(n_kfs_), F(F_), frame_kind(frame_kind_), nn_ratio(nn_ratio_),
        check_orientation(check_orientation_), match(match_), match_dist(match_dist_), nmatches(nmatches_), stats(stats_) {}

  int n_out() const { return frame_kind ? F->n : kf1->pt.n; }   // the outputs' row length

  bs::Side frame_side(const uint32_t* node_id, const int32_t* off, const uint32_t* idx, const void* desc) const {
    return bs::Side{node_id, off, idx, reinterpret_cast<const uint4*>(desc), nullptr, F->vec.nnodes};
  }

  void prepare() override {
    if (frame_kind) {
      f_off.assign((size_t)F->vec.nnodes + 1, 0);
      for (int a = 0; a <= F->vec.nnodes && F->vec.nnodes > 0; ++a) f_off[a] = F->vec.offset[a] - F->vec.offset[0];
      f_listed = f_off[F->vec.nnodes];
    }
    host_tab.resize((size_t)n_kfs);
    bool work = false;
    for (int k = 0; k < n_kfs; ++k) {
      bs::Pair& T = host_tab[k];
      const bs::Side mine = handle_side(*kfs[k], kfs[k]->host.data(), valid[k]);
      if (frame_kind) {
        T.s = mine;
        T.l = frame_side(F->vec.node_id, f_off.data(), F->vec.nnodes > 0 && f_listed > 0 ? F->vec.index + F->vec.offset[0] : nullptr, F->desc);
      } else {
        T.s = handle_side(*kf1, kf1->host.data(), valid1);
        T.l = mine;
      }
      T.rec_at = n_rec;
      T.gate_at = n_gate;
      n_rec += T.s.off[T.s.nnodes];
      n_gate += T.l.off[T.l.nnodes];
      max_serial_nodes = std::max(max_serial_nodes, T.s.nnodes);
      const bs::JobCounts c = bs::count_jobs(T.s, T.l);
      jobs.common += c.common;
      jobs.multi_pass += c.multi_pass;
      const plvs_keyframe& serial = frame_kind ? *kfs[k] : *kf1;
      work = work || (c.common > 0 && any_set(T.s.valid, serial.pt.n));
    }
    device = work && !on_host;
    if (!device) return;
    fj::Take take;
    o_tab = take(sizeof(bs::Pair) * (size_t)n_kfs);
    o_valid.resize((size_t)n_kfs);
    for (int k = 0; k < n_kfs; ++k) o_valid[k] = take((size_t)kfs[k]->pt.n);
    if (frame_kind) {
      o_fdesc = take((size_t)F->n * 32);
      o_fnode = take(sizeof(uint32_t) * (size_t)F->vec.nnodes);
      o_foff = take(sizeof(int32_t) * ((size_t)F->vec.nnodes + 1));
      o_fidx = take(sizeof(uint32_t) * (size_t)f_listed);
    } else {
      o_valid1 = take((size_t)kf1->pt.n);
    }
    in_bytes = take.at;
    scratch_bytes = fj::up16((size_t)n_gate);
    out_bytes = fj::up16(sizeof(int2) * (size_t)n_rec);
  }

  void fill(char* pinned) override {
    char* p = pinned + in_at;
    const char* d = plvs::thread_stage().dev + in_at;   // where the copy lands: the table points into it
    bs::Pair* tab = reinterpret_cast<bs::Pair*>(p + o_tab);
    for (int k = 0; k < n_kfs; ++k) memcpy(p + o_valid[k], valid[k], (size_t)kfs[k]->pt.n);
    if (frame_kind) {
      memcpy(p + o_fdesc, F->desc, (size_t)F->n * 32);
      memcpy(p + o_fnode, F->vec.node_id, sizeof(uint32_t) * (size_t)F->vec.nnodes);
      memcpy(p + o_foff, f_off.data(), sizeof(int32_t) * f_off.size());
      if (f_listed) memcpy(p + o_fidx, F->vec.index + F->vec.offset[0], sizeof(uint32_t) * (size_t)f_listed);
    } else {
      memcpy(p + o_valid1, valid1, (size_t)kf1->pt.n);
    }
    for (int k = 0; k < n_kfs; ++k) {
      const bs::Side mine = handle_side(*kfs[k], kfs[k]->dev, reinterpret_cast<const uint8_t*>(d + o_valid[k]));
      bs::Pair T;
      if (frame_kind) {
        T.s = mine;
        T.l = frame_side(reinterpret_cast<const uint32_t*>(d + o_fnode), reinterpret_cast<const int32_t*>(d + o_foff),
                         reinterpret_cast<const uint32_t*>(d + o_fidx), d + o_fdesc);
      } else {
        T.s = handle_side(*kf1, kf1->dev, reinterpret_cast<const uint8_t*>(d + o_valid1));
        T.l = mine;
      }
      T.rec_at = host_tab[k].rec_at;
      T.gate_at = host_tab[k].gate_at;
      tab[k] = T;
    }
  }

  int launch(char* dev, char* pinned, hipStream_t stream) override {
    const bs::Pair* tab = reinterpret_cast<const bs::Pair*>(dev + in_at + o_tab);
    int2* rec = reinterpret_cast<int2*>(pinned + out_at);
    uint8_t* gates = reinterpret_cast<uint8_t*>(dev + scratch_at);
    const dim3 grid(plvs::ceil_div((size_t)max_serial_nodes, 4), (unsigned)n_kfs);
    if (frame_kind) hipLaunchKernelGGL(bow_search_kernel<true>, grid, dim3(256), 0, stream, tab, nn_ratio, rec, gates);
    else hipLaunchKernelGGL(bow_search_kernel<false>, grid, dim3(256), 0, stream, tab, nn_ratio, rec, gates);
    PLVS_KERNEL_CHECK();
    ++launches;
    return PLVS_OK;
  }

  void host_all() override {
    host_rec.resize((size_t)n_rec);
    std::vector<uint8_t> open;
    for (int k = 0; k < n_kfs; ++k) {
      if (frame_kind) bs::pair_host<true>(host_tab[k], nn_ratio, host_rec.data() + host_tab[k].rec_at, &open);
      else bs::pair_host<false>(host_tab[k], nn_ratio, host_rec.data() + host_tab[k].rec_at, &open);
    }
  }
  void collect(const char* pinned) override {
    const int2* r = reinterpret_cast<const int2*>(pinned + out_at);
    host_rec.assign(r, r + n_rec);
  }

  // the records in the reference's order -> the outputs, the rotation histogram (:947-957, :419-434) and its cut (:976-994, :485-503)
  void post() override {
    const int row = n_out();
    const float factor = kHistoLength / 360.0f;   // USE_NEW_HISTOGRAM_FACTOR, :52
    std::vector<int> hist_item, hist_bin;
    for (size_t i = 0; i < (size_t)n_kfs * row; ++i) match[i] = match_dist[i] = -1;
    for (int k = 0; k < n_kfs; ++k) {
      const bs::Pair& T = host_tab[k];
      const int2* R = host_rec.data() + T.rec_at;
      int32_t* m = match + (size_t)k * row;
      int32_t* md = match_dist + (size_t)k * row;
      const float* angle_s = handle_angle(frame_kind ? *kfs[k] : *kf1);
      const float* angle_l = frame_kind ? F->angle : handle_angle(*kfs[k]);
      hist_item.clear();
      hist_bin.clear();
      int n = 0;
      for (int p = 0; p < T.s.off[T.s.nnodes]; ++p) {
        if (R[p].x < 0) continue;
        const int is = (int)T.s.idx[p], il = R[p].x;
        const int at = frame_kind ? il : is;       // vpMapPointMatches[bestIdxF] / vpMatches12[idx1]
        m[at] = frame_kind ? is : il;
        md[at] = R[p].y & 0xffff;
        ++n;
        if (check_orientation) {
          float rot = angle_s[is] - angle_l[il];
          if (rot < 0.0) rot += 360.0f;
          int bin = (int)std::round(rot * factor);
          if (bin == kHistoLength) bin = 0;
          hist_item.push_back(at);
          hist_bin.push_back(bin);
        }
      }
      if (check_orientation) {
        int count[kHistoLength] = {0};
        for (int b : hist_bin) ++count[b];
        int ind1, ind2, ind3;
        plvs::orbwin::three_maxima(count, kHistoLength, ind1, ind2, ind3);
        for (size_t h = 0; h < hist_bin.size(); ++h)
          if (hist_bin[h] != ind1 && hist_bin[h] != ind2 && hist_bin[h] != ind3) {
            m[hist_item[h]] = md[hist_item[h]] = -1;
            --n;
          }
      }
      if (nmatches) nmatches[k] = n;
    }
    if (!stats) return;
    stats[0] = launches; stats[1] = device ? 1 : 0; stats[2] = fj::copy_in_stat(*this);
    stats[3] = jobs.common; stats[4] = jobs.multi_pass; stats[5] = 0;
  }
};

// a NULL handle, a handle without a BoW side, for a device entry a host-only handle — all before any HIP call — then a handle of
// another device
int check_bow_handles(const std::vector<const plvs_keyframe*>& hs, bool host_entry) {
  for (const plvs_keyframe* h : hs) {
    PLVS_REQUIRE(h, "null key-frame handle");
    PLVS_REQUIRE(h->bow.present && h->pt.present, "a key-frame handle without a BoW side (plvs_hip_keyframe_create_bow makes one)");
  }
  if (host_entry) return PLVS_OK;
  for (const plvs_keyframe* h : hs)
    PLVS_REQUIRE(!(h->flags & PLVS_KEYFRAME_HOST_ONLY), "a PLVS_KEYFRAME_HOST_ONLY handle in a device entry (the _kf_host entries take it)");
  if (hs.empty()) return PLVS_OK;
  int device = -1;
  PLVS_HIP_TRY(hipGetDevice(&device));
  for (const plvs_keyframe* h : hs) PLVS_REQUIRE(h->device == device, "a key-frame handle created on another device than the current one");
  return PLVS_OK;
}

}  // namespace

int plvs::fusejob::make_bow_search_part(const plvs_keyframe* kf1, const uint8_t* valid1, const plvs_keyframe* const* kfs,
                                        const uint8_t* const* valid, int n_kfs, const plvs_bow_frame* F, bool frame_kind, float nn_ratio,
                                        int check_orientation, int32_t* match, int32_t* match_dist, int32_t* nmatches, int32_t* stats,
                                        bool host_entry, std::unique_ptr<Part>* out) {
  out->reset();
  PLVS_REQUIRE(n_kfs >= 0 && n_kfs <= 65535, "key-frame count outside [0, 65535]");
  PLVS_REQUIRE(match && match_dist, "null output");
  PLVS_REQUIRE(n_kfs == 0 || (kfs && valid), "null key frames / validity list");
  PLVS_REQUIRE(nn_ratio >= 0.0f, "nn_ratio negative or NaN");
  std::vector<const plvs_keyframe*> hs;
  if (!frame_kind) hs.push_back(kf1);
  for (int k = 0; k < n_kfs; ++k) hs.push_back(kfs[k]);
  int rc = check_bow_handles(hs, host_entry);
  if (rc != PLVS_OK) return rc;
  for (int k = 0; k < n_kfs; ++k) PLVS_REQUIRE(valid[k] || kfs[k]->pt.n == 0, "null validity array");
  if (frame_kind) {
    PLVS_REQUIRE(F && F->n >= 0 && F->n < (1 << bs::kPosBits), "null frame / key point count outside [0, 2^23)");
    PLVS_REQUIRE(F->n == 0 || (F->desc && F->angle), "null frame array");
    rc = bs::check_featvec(F->vec, F->n, nullptr, nullptr);
    if (rc != PLVS_OK) return rc;
  } else {
    PLVS_REQUIRE(valid1 || kf1->pt.n == 0, "null validity array");
  }
  long long rows = 0, recs = 0;
  for (int k = 0; k < n_kfs; ++k) {
    rows += frame_kind ? F->n : kf1->pt.n;
    recs += (frame_kind ? kfs[k] : kf1)->bow.listed;
  }
  PLVS_REQUIRE(rows <= (1ll << 30) && recs <= (1ll << 30), "more than 2^30 outputs");
  if (n_kfs > 0)
    out->reset(new BowSearch(kf1, valid1, kfs, valid, n_kfs, F, frame_kind, nn_ratio, check_orientation, match, match_dist, nmatches, stats));
  return PLVS_OK;
}

// ---- the handle's BoW side
int plvs::kfhandle::check_bow(const plvs_keyframe_bow& bow, int n, int* listed, int* longest) {
  const int rc = plvs::bowsearch::check_featvec(bow.vec, n, listed, longest);
  if (rc != PLVS_OK) return rc;
  PLVS_REQUIRE(bow.angle || n == 0, "null angle");
  return PLVS_OK;
}

void plvs::kfhandle::stage_bow(const plvs_keyframe_bow& bow, int listed, int longest, plvs_keyframe* h) {
  plvs_keyframe::Bow& s = h->bow;
  const size_t before = (h->host.size() + 15) & ~(size_t)15;
  const int nn = bow.vec.nnodes;
  std::vector<int32_t> off((size_t)nn + 1, 0);
  for (int a = 0; a <= nn && nn > 0; ++a) off[a] = bow.vec.offset[a] - bow.vec.offset[0];
  s.present = true;
  s.nnodes = nn;
  s.listed = listed;
  s.longest = longest;
  s.o_node = put(&h->host, bow.vec.node_id, sizeof(uint32_t) * (size_t)nn);
  s.o_off = put(&h->host, off.data(), sizeof(int32_t) * off.size());
  s.o_idx = put(&h->host, listed ? bow.vec.index + bow.vec.offset[0] : nullptr, sizeof(uint32_t) * (size_t)listed);
  s.o_angle = put(&h->host, bow.angle, sizeof(float) * (size_t)h->pt.n);
  s.bytes = h->host.size() - before;
}
