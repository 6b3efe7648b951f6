// TSDF integrate for the open_chisel back end (PointCloudMapChisel::InsertCloud
// -> Chisel::IntegratePointCloudWidthDepth, point-cloud part).
//
// Data layout in HBM (per handle):
//   voxel pool      four planes sdf / weight / kfid / rgbw, each
//                   max_chunks * 4096 dwords; chunk slot s owns words
//                   [s*4096, (s+1)*4096) of every plane (64 KiB per chunk).
//   chunk directory open-addressing hash (2*max_chunks, power of two) from the
//                   packed 3x21-bit chunk id to the pool slot, plus slot -> id.
//   per call        per voxel visit the update operands (w_u*u, w_u: 8 bytes) and the
//                   colour (4 bytes), written once grouped per tile and once in voxel
//                   order; per tile-local run of visits to one voxel a 20-byte descriptor.
//
// The reference integrates points strictly in order, and both the running
// weighted mean (f32) and the truncating u8 colour mean are order dependent.
// The device path keeps that order exactly:
//   1. ray_count   one thread per point walks its Amanatides-Woo ray and counts
//                  the voxels that take an update; first-touch chunks are
//                  inserted into the directory.
//   2. scan        exclusive scan of the counts = visit offsets (point order).
//   3. ray_tiles   the visit slots are cut into tiles of 4096; a workgroup re-walks the
//                  rays of its tile, keeps the visits in LDS, groups them by voxel (point
//                  order inside a group) and writes the update operands (w_u*u, w_u) and
//                  colours grouped that way, plus one descriptor per group ("run").
//   4. sort_runs   stable radix sort of the run descriptors by voxel key: per voxel its
//                  runs in tile (= point) order.  Runs, not visits, are sorted.
//   5. gather_runs copies the runs into voxel order -> per voxel its records contiguous
//                  and in point order; compacts voxel heads and updated chunks.
//   6. chain       one thread per voxel folds its records sequentially in registers (the
//                  f32 weighted mean; the truncating u8 colour mean on a second stream):
//                  each voxel is read and written once per call.
// Results are bit-identical to the sequential CPU loop.  This is the ordered mode (order_free = 0); the
// order-free mode (sdf / weight within a stated float tolerance, kfid and colour exact) is the single-walk
// pipeline of tsdf_walk.hpp.
#pragma once
#include "tsdf_chisel_handle.hpp"
#include "tsdf_tiles.hpp"

namespace {

// Stage 1: count the updating visits of each point and insert first-touch chunks.
// kNormals: the world-cloud-with-normals flavour (make_ray_normal / resolve_visit_normal), `normals` n x 3.
template <bool kNormals>
__global__ __launch_bounds__(256) void ray_count(
    Params P, const float* __restrict__ xyz, const float* __restrict__ normals, int npoints,
    const int32_t* __restrict__ offsets, int nclouds, const Pose* __restrict__ poses, Directory dir,
    Counters* __restrict__ ctr, uint32_t* __restrict__ counts) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npoints) return;
  const Pose pose = poses[cloud_of(offsets, nclouds, i)];
  Ray ray;
  RayN aux;
  uint32_t n = 0;
  bool walk = true;
  if (kNormals)
    make_ray_normal(P, pose, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], normals[3 * (size_t)i],
                    normals[3 * (size_t)i + 1], normals[3 * (size_t)i + 2], &ray, &aux);
  else
    walk = make_ray(P, pose, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], &ray);
  if (walk && !ray_in_coord_range(ray)) {
    // beyond the range in which the integer chunk addressing equals the reference's float
    // lookup: fail loudly instead of diverging
    atomicOr(&ctr->err, kErrCoordRange);
    walk = false;
  }
  // on a shard most rays cannot reach a chunk of this rank: skip their set-up and walk (with two
  // ranks nearly every ray still can, the test would only cost)
  if (walk && P.shard_count > 2 && !walk_may_touch_owned(P, ray)) walk = false;
  if (walk) {
    RayCursor cur;
    OwnerCache owner;
    ray_begin(ray, &cur);
    int vx, vy, vz;
    int lcx = 0, lcy = 0, lcz = 0;  // last chunk seen by this ray
    bool have_last = false;
    // one DDA step per trip for every lane (an early `continue` on rejected steps makes the compiler
    // nest a skip loop in which the lanes of a wave wait for each other's rejected stretches)
    while (ray_next(&cur, &vx, &vy, &vz)) {
      Visit v;
      const bool ok = kNormals ? resolve_visit_normal(P, aux, ray, vx, vy, vz, &v, &owner)
                               : resolve_visit(P, pose, ray, vx, vy, vz, &v, &owner);
      if (ok && (!have_last || v.cx != lcx || v.cy != lcy || v.cz != lcz)) {
        lcx = v.cx; lcy = v.cy; lcz = v.cz;
        have_last = true;
        dir_insert(dir, lcx, lcy, lcz, &ctr->num_chunks, &ctr->err);
      }
      n += ok ? 1u : 0u;
    }
  }
  counts[i] = n;
}

// ------------------------------------------------------------------ tiles
// Stage 3.  The visit slots of the call (point order, dense: offsets = scan of the counts)
// are cut into tiles of kTileSlots.  One workgroup per tile re-walks the rays of its points,
// keeps the tile's visits in LDS, groups them by voxel and writes
//   * the update operands (w_u*u, w_u) and the colour of every visit, grouped by voxel
//     and, inside a group, in point order (tile-local "runs"), fully coalesced;
//   * one descriptor per run: voxel key (slot*4096 + voxel), position, length and the
//     point of its last visit.
// Only the descriptors (one per run, not one per visit) go through the global sort.
//
// Grouping: an LDS hash table keyed by the voxel key gives every visit the table entry of
// its voxel; a stable LDS radix sort of (entry, slot) tags by entry (12 bits, two passes)
// makes the visits of a voxel contiguous and keeps them in slot (= point) order — its cost
// does not depend on how many visits a voxel collects.  The order of the groups inside
// a tile is irrelevant: a tile holds at most one run per voxel, and runs of different tiles
// keep their tile order through the stable global sort.
//
// Run descriptors are numbered across tiles by a decoupled look-back over tile_state (tile
// ids are tickets, so a tile only ever waits for tiles that already started).
struct TileOut {
  float2* vis;          // [V] per visit, in slot order: (u, point index as bits) — kept out of LDS so that
                        // three tiles fit a CU
  float2* rec_t;        // [V] operands, tile-grouped
  uint32_t* recc_t;     // [V] colours, tile-grouped
  uint32_t* dkey;       // run descriptors: voxel key,
  unsigned long long* dval;   // value array of the sort: position in rec_t | length << 32,
  uint32_t* last_pt;    // [V], sparse: at a run's position, the point of its last visit
};

template <bool kNormals>
__global__ __launch_bounds__(kTileThreads, 6) void ray_tiles(
    Params P, const float* __restrict__ xyz, const float* __restrict__ normals, const uint8_t* __restrict__ rgb, int npoints,
    const int32_t* __restrict__ offsets, int nclouds, const Pose* __restrict__ poses, Directory dir,
    Counters* __restrict__ ctr, const uint32_t* __restrict__ voff, uint32_t V,
    const uint32_t* __restrict__ tile_first, uint32_t ntiles, uint32_t* __restrict__ ticket,
    unsigned long long* __restrict__ tile_state, const uint32_t* __restrict__ rgbw, TileOut out) {
  __shared__ uint32_t skey[kTileSlots];     // voxel key of the visit in slot s
  __shared__ uint32_t bufA[kTileSlots];     // tags: group table entry << 12 | slot; sorted in place
  __shared__ uint32_t bufB[kTileSlots];     // the group hash table, then the sort's second buffer, then run heads
  __shared__ uint32_t wave_hist[kTileThreads / 64][kTileRadix];
  uint32_t* const gtab = bufB;              // representative slot of the voxel hashed to this entry
  __shared__ uint32_t wsum[kTileThreads / 64];
  __shared__ uint32_t sh_tile, sh_base;
  __shared__ unsigned long long ckey[kTileChunkCache];   // chunk id -> pool slot, the chunks this tile meets
  __shared__ int32_t cslot[kTileChunkCache];
  __shared__ int32_t cl_off[kTileCloudCache + 1];          // cloud offsets around the tile
  const int tid = threadIdx.x;

  if (tid == 0) {
    sh_tile = atomicAdd(ticket, 1u);
  }
#pragma unroll
  for (int k = 0; k < kTileItems; ++k) gtab[tid + k * kTileThreads] = kTileEmpty;
  if (tid < kTileChunkCache) {
    ckey[tid] = kEmptyKey;
    cslot[tid] = -2;
  }
  __syncthreads();
  const uint32_t t = sh_tile;
  const uint32_t slot0 = t * kTileSlots;
  const uint32_t n = min((uint32_t)kTileSlots, V - slot0);
  const uint32_t first = tile_first[t];
  const uint32_t last = (t + 1 < ntiles) ? tile_first[t + 1] : (uint32_t)(npoints - 1);

  // the clouds the tile's points belong to: offsets of up to kTileCloudCache of them in LDS
  const int cloud0 = cloud_of(offsets, nclouds, (int)first);
  const int ncl = min(nclouds - cloud0, kTileCloudCache);
  if (tid <= ncl) cl_off[tid] = offsets[cloud0 + tid];
  __syncthreads();

  // ---- phase 1a: the points of [first, last] that have visits in this tile, compacted (any order:
  // a visit's slot comes from voff).  On a shard most points of the range have none — their chunks
  // belong to other ranks, whole keyframes can look at chunks of other ranks only — and a wave
  // would otherwise walk 64 rays for the few lanes that do.  Stretches without visits are jumped
  // over by bisection on voff (uniform control flow).
  uint32_t* const tile_rays = bufA;   // free until phase 2; a tile holds <= kTileSlots such points
  if (tid == 0) sh_base = 0;
  __syncthreads();
  for (uint32_t base = first; base <= last;) {
    const uint32_t vb = voff[base];
    if (vb >= slot0 + n) break;                          // the rest belongs to later tiles
    const uint32_t end = min(base + (uint32_t)kTileThreads, last + 1);
    if (voff[end] == vb) {                               // nothing in [base, end)
      uint32_t lo = end, hi = last + 1;                  // voff[lo] == vb throughout
      if (voff[hi] == vb) break;
      while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (voff[mid] > vb) hi = mid; else lo = mid;
      }
      base = lo;                                         // point lo is the next one with visits
      continue;
    }
    const uint32_t i = base + tid;
    bool has = false;
    if (i < end) {
      const uint32_t o = voff[i], e = voff[i + 1];
      has = !(e == o || e <= slot0 || o >= slot0 + n);
    }
    const unsigned long long m = __ballot(has);
    uint32_t wbase = 0;
    if ((tid & 63) == 0 && m != 0ull) wbase = atomicAdd(&sh_base, (uint32_t)__popcll(m));
    wbase = __shfl(wbase, 0);
    if (has) tile_rays[wbase + __popcll(m & ((1ull << (tid & 63)) - 1ull))] = i;
    base = end;
  }
  __syncthreads();
  const uint32_t nrays = sh_base;
  __syncthreads();   // sh_base is reused by the look-back

  // ---- phase 1b: the visits of this tile, in slot (= point, then ray) order
  for (uint32_t r = tid; r < nrays; r += kTileThreads) {
    const uint32_t i = tile_rays[r];
    const uint32_t o = voff[i], e = voff[i + 1];
    const uint32_t n_lo = (o < slot0) ? slot0 - o : 0u;       // visits before it belong to the previous tile
    const uint32_t n_hi = min(e, slot0 + n) - o;              // visits from it on to the next one
    int cl = 0;
    while (cl + 1 < ncl && (int)i >= cl_off[cl + 1]) ++cl;
    if ((int)i >= cl_off[ncl]) cl = cloud_of(offsets, nclouds, (int)i) - cloud0;   // beyond the cached clouds
    const Pose pose = poses[cloud0 + cl];
    Ray ray;
    RayN aux;
    if (kNormals)
      make_ray_normal(P, pose, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], normals[3 * (size_t)i],
                      normals[3 * (size_t)i + 1], normals[3 * (size_t)i + 2], &ray, &aux);
    else if (!make_ray(P, pose, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], &ray))
      continue;
    RayCursor cur;
    OwnerCache owner;
    ray_begin(ray, &cur);
    int vx, vy, vz;
    int lcx = 0, lcy = 0, lcz = 0, lslot = -1;
    bool have_last = false;
    uint32_t nv = 0;
    while (nv < n_hi && ray_next(&cur, &vx, &vy, &vz)) {
      Visit v;
      const bool ok = kNormals ? resolve_visit_normal(P, aux, ray, vx, vy, vz, &v, &owner)
                               : resolve_visit(P, pose, ray, vx, vy, vz, &v, &owner);   // no early continue: see ray_count
      if (ok && nv >= n_lo) {
        if (!have_last || v.cx != lcx || v.cy != lcy || v.cz != lcz) {
          lcx = v.cx; lcy = v.cy; lcz = v.cz;
          have_last = true;
          lslot = tile_find_chunk(dir, ckey, cslot, lcx, lcy, lcz);
          if (lslot < 0) atomicOr(&ctr->err, kErrDirectoryMiss);
        }
        const uint32_t s = o + nv - slot0;
        skey[s] = (uint32_t)max(lslot, 0) * (uint32_t)kChunkVox + (uint32_t)v.vid;
        out.vis[slot0 + s] = make_float2(v.u, __uint_as_float(i));
      }
      nv += ok ? 1u : 0u;
    }
    if (nv < n_hi) atomicOr(&ctr->err, kErrDirectoryMiss);   // the count pass saw more visits: cannot happen
  }
  __syncthreads();

  // ---- phases 2-4: group the visits by voxel (LDS hash table), stable LDS radix sort of the
  // (group, slot) tags, run heads (tsdf_tiles.hpp)
  const uint32_t ngroups = tile_group_sort_heads(skey, bufA, bufB, wave_hist, wsum, n, tid);
  uint16_t* const hp = reinterpret_cast<uint16_t*>(bufB);   // positions of the runs; the sorted tags are in bufA
  // publish this tile's run count for the tiles behind it
  if (tid == 0 && t > 0) st_state(&tile_state[t], (1ull << 62) | ngroups);
  __syncthreads();   // hp complete

  // ---- phase 5: operands out, in sorted order
#pragma unroll
  for (int k = 0; k < kTileItems; ++k) {
    const uint32_t j = tid + k * kTileThreads;
    if (j < n) {
      const uint32_t s = bufA[j] & 0xFFFu;
      const float2 vv = out.vis[slot0 + s];
      const size_t p = __float_as_uint(vv.y);
      const float tr = kNormals ? 4 * P.resolution : truncation_of(P, xyz[3 * p + 2]);
      const float wu = P.weight / (2.0f * tr);
      out.rec_t[slot0 + j] = make_float2(wu * vv.x, wu);
      out.recc_t[slot0 + j] = colour_roundtrip(rgb[3 * p + 0]) | (colour_roundtrip(rgb[3 * p + 1]) << 8) |
                              (colour_roundtrip(rgb[3 * p + 2]) << 16);
    }
  }

  // the tile's place in the run numbering (decoupled look-back, wave 0)
  tile_lookback(t, ngroups, ntiles, tile_state, &sh_base, &ctr->num_desc, tid);
  __syncthreads();

  // ---- phase 6: run descriptors out
  const uint32_t dbase = sh_base;
  for (uint32_t g = tid; g < ngroups; g += kTileThreads) {
    const uint32_t p0 = hp[g], p1 = hp[g + 1];
    const uint32_t d = dbase + g;
    out.dkey[d] = skey[bufA[p0] & 0xFFFu];
    out.dval[d] = (unsigned long long)(slot0 + p0) | ((unsigned long long)(p1 - p0) << 32);
    out.last_pt[slot0 + p0] = __float_as_uint(out.vis[slot0 + (bufA[p1 - 1] & 0xFFFu)].y);
  }
}

// The truncating u8 colour mean of the ordered mode: one thread per voxel whose colour weight is below
// 254 folds its visits one by one through the sorted runs, exactly as the reference does, until the
// weight reaches 254 (at most 254 steps in the life of a voxel).
// kDivide: ColorVoxel::Integrate (a true division; the world-cloud-with-normals flavour) instead of IntegrateSimple.
template <bool kDivide>
__global__ __launch_bounds__(256) void fold_colours(
    const uint32_t* __restrict__ skeys, const unsigned long long* __restrict__ sval, uint32_t nd,
    const uint32_t* __restrict__ vj0, const uint32_t* __restrict__ recc_t, uint32_t* __restrict__ rgbw,
    const Counters* __restrict__ ctr) {
  // 1 / (1 + weight), the factor of ColorVoxel::IntegrateSimple, for every weight it can see
  __shared__ float inv_tab[256];
  inv_tab[threadIdx.x] = 1.f / (float)(1u + (uint32_t)threadIdx.x);
  __syncthreads();
  constexpr int kTurn = 16;   // visits per turn
  constexpr int kRuns = 8;    // run descriptors looked at per turn
  const uint32_t nvox = ctr->num_heads;
  for (uint32_t v0 = blockIdx.x * blockDim.x; v0 < nvox; v0 += gridDim.x * blockDim.x) {
    const uint32_t v = v0 + threadIdx.x;
    uint32_t key = 0, col = 254u << 24, jj = 0;
    if (v < nvox) {
      jj = vj0[v];
      key = skeys[jj];
      col = rgbw[key];
    }
    const bool fresh = v < nvox && (col >> 24) < 254u;
    // One flat loop for the whole wave.  A turn takes up to kTurn visits, across up to kRuns
    // consecutive runs of the voxel (runs are short: ~10 visits); the run descriptors of the next
    // turn are requested while the colours of this one are in flight — the fold is cheap, the
    // latency of a load per visit is not.
    bool active = fresh;
    uint32_t pos = 0;   // visits of run jj already folded
    unsigned long long d[kRuns];
    uint32_t dk[kRuns];
#pragma unroll
    for (int q = 0; q < kRuns; ++q) {
      const uint32_t jq = min(jj + q, nd - 1);
      d[q] = active ? sval[jq] : 0ull;
      dk[q] = active ? skeys[jq] : ~key;
    }
    while (__ballot(active) != 0ull) {
      // the runs at hand: which of them belong to the voxel, where each starts in the turn's
      // visit sequence (prefix of the remaining lengths)
      uint32_t start[kRuns + 1];   // visit index (within the turn's sequence) at which run q begins
      uint32_t nvalid = 0;          // leading runs of the voxel among the descriptors
      start[0] = 0;
#pragma unroll
      for (int q = 0; q < kRuns; ++q) {
        const bool mine = nvalid == (uint32_t)q && (jj + q < nd) && dk[q] == key;
        nvalid += mine ? 1u : 0u;
        const uint32_t len = mine ? (uint32_t)(d[q] >> 32) - (q == 0 ? pos : 0u) : 0u;
        start[q + 1] = start[q] + len;
      }
      const bool voxel_ends = nvalid < (uint32_t)kRuns;   // the voxel's runs end within the descriptors at hand
      const uint32_t avail = start[kRuns];
      const uint32_t taken = min(avail, (uint32_t)kTurn);
      // addresses of this turn's visits
      uint32_t addr[kTurn];
#pragma unroll
      for (int e = 0; e < kTurn; ++e) {
        uint32_t a0 = (uint32_t)d[0] + pos + (uint32_t)e;
#pragma unroll
        for (int q = 1; q < kRuns; ++q) a0 = ((uint32_t)e >= start[q]) ? (uint32_t)d[q] + ((uint32_t)e - start[q]) : a0;
        addr[e] = a0;
      }
      // where the turn stops: the run holding visit number `taken` (or past the last one)
      uint32_t run = 0;
#pragma unroll
      for (int q = 1; q <= kRuns; ++q) run += (taken >= start[q]) ? 1u : 0u;   // runs fully consumed
      const uint32_t p = (run < (uint32_t)kRuns) ? taken - start[run] + (run == 0 ? pos : 0u) : 0u;
      uint32_t c[kTurn];
#pragma unroll
      for (int e = 0; e < kTurn; ++e) c[e] = (active && (uint32_t)e < taken) ? recc_t[addr[e]] : 0u;
      // where the next turn starts, and its descriptors
      // (run / p after the loop: p may equal the count of run `run`; the skip at the top handles it)
      const uint32_t jj_next = jj + min(run, (uint32_t)kRuns);
      const uint32_t pos_next = (run < (uint32_t)kRuns) ? p : 0u;
      unsigned long long dn[kRuns];
      uint32_t dkn[kRuns];
#pragma unroll
      for (int q = 0; q < kRuns; ++q) {
        const uint32_t jq = min(jj_next + q, nd - 1);
        dn[q] = active ? sval[jq] : 0ull;
        dkn[q] = active && (jj_next + q < nd) ? skeys[jq] : ~key;
      }
      if (active) {
#pragma unroll
        for (int e = 0; e < kTurn; ++e) {
          const uint32_t cw = col >> 24;
          if ((uint32_t)e < taken && cw < 254u) {   // ColorVoxel::IntegrateSimple, visit by visit
            uint32_t red, green, blue;
            if (kDivide) {   // ColorVoxel::Integrate (ColorVoxel.h:68-89); Saturate cannot bind: a mean of bytes
              const float den = (float)(cw + 1u);
              red = (uint32_t)(uint8_t)((float)(cw * (col & 255u) + (c[e] & 255u)) / den);
              green = (uint32_t)(uint8_t)((float)(cw * ((col >> 8) & 255u) + ((c[e] >> 8) & 255u)) / den);
              blue = (uint32_t)(uint8_t)((float)(cw * ((col >> 16) & 255u) + ((c[e] >> 16) & 255u)) / den);
            } else {
              const float inv = inv_tab[cw];
              red = (uint32_t)(uint8_t)((float)(cw * (col & 255u) + (c[e] & 255u)) * inv);
              green = (uint32_t)(uint8_t)((float)(cw * ((col >> 8) & 255u) + ((c[e] >> 8) & 255u)) * inv);
              blue = (uint32_t)(uint8_t)((float)(cw * ((col >> 16) & 255u) + ((c[e] >> 16) & 255u)) * inv);
            }
            col = red | (green << 8) | (blue << 16) | ((cw + 1u) << 24);
          }
        }
        if ((col >> 24) >= 254u || (voxel_ends && taken == avail) || taken == 0) active = false;
      }
      jj = jj_next;
      pos = pos_next;
#pragma unroll
      for (int q = 0; q < kRuns; ++q) { d[q] = dn[q]; dk[q] = dkn[q]; }
    }
    if (fresh) rgbw[key] = col;
  }
}

// The order-dependent part: one thread per voxel run, 64 runs per wave, eight records per
// run and pass.  A single wave issues about one instruction every four cycles, and the
// longest run of the call is a serial chain, so the kernel is built to keep the
// instructions per step low and every wait off that chain:
//  * Loads: a lane walking its own run touches 64 different cache lines per load
//    instruction.  Here the wave fetches a pass cooperatively — four lanes read the eight
//    consecutive records (64 B) of one run, sixteen runs per load instruction — and hands
//    the records to their lanes through LDS (XOR-swizzled 16-byte units).  Four passes are
//    in flight in registers; the LDS hop is pipelined one pass deep (four buffers, no
//    barrier: one wave, and LDS operations of a wave execute in order).
//  * Arithmetic: w_k = w_{k-1} + wu_k does not depend on the running sdf, so the weights and
//    their reciprocals of the NEXT pass are computed beside the sdf recurrence of the
//    current pass; the recurrence itself is dist_update_rcp (mul, add, mul, fma, fma).
//    v_rcp_f32 plus one Newton step gives the correctly rounded reciprocal for every
//    binary32 significand on gfx950 (plvs_hip_selftest_rcp checks all 2^23 of them).
//  * A lane whose pass contains the end of its run (negative weight = last record), or an
//    operand outside the exact range of the reciprocal form, redoes that pass step by step.
//    Nothing is loaded there: the keyframe id of the voxel is written by gather_runs,
//    the longest run is reduced once per wave.
constexpr int kChainBatch = 8;
constexpr int kChainSets = 4;

__device__ __forceinline__ float rcp_rn(float b) {
  const float y0 = __builtin_amdgcn_rcpf(b);
  const float e = fmaf(-b, y0, 1.0f);
  return fmaf(e, y0, y0);
}

struct __attribute__((packed, aligned(8))) RecPair {   // two consecutive float2 records
  float x0, y0, x1, y1;
};

// 16-byte unit u (records 2u, 2u+1) of a run inside a staging buffer
__device__ __forceinline__ int stage_unit(int run, int u) { return run * 4 + ((u ^ (run >> 1)) & 3); }

__global__ __launch_bounds__(64) void chain_runs(
    const uint32_t* __restrict__ vj0, const uint32_t* __restrict__ skeys, const uint32_t* __restrict__ dst,
    uint32_t nrec, const float2* __restrict__ rec, Counters* __restrict__ ctr, float* __restrict__ sdf,
    float* __restrict__ weight) {
  __shared__ float4 stage[kChainSets][64 * 4];
  const int l = threadIdx.x;
  const uint32_t nheads = ctr->num_heads;
  const uint32_t last_pair = nrec - 1;   // the record buffer holds at least nrec + 1 records
  // the grid is an upper bound (the run count is only known on the device): surplus waves
  // leave at once, and a wave takes further groups of 64 runs if the grid was capped
  for (uint32_t group = blockIdx.x; group * 64u < nheads; group += gridDim.x) {
    const uint32_t h = group * 64u + (uint32_t)l;
    bool live = h < nheads;
    const uint32_t j0 = live ? vj0[h] : 0u;            // first run of the voxel
    const uint32_t r0 = live ? dst[j0] : 0u;           // its first record
    const size_t a = live ? (size_t)skeys[j0] : 0;     // slot*4096 + vid
    float s = live ? sdf[a] : 0.0f;
    float w = live ? weight[a] : 1.0f;
    uint32_t my_len = 0;
    // load i serves runs 16 i .. 16 i + 15; this lane fetches records 2q, 2q+1 (q = lane & 3)
    // of run 16 i + (lane >> 2)
    uint32_t base[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) base[i] = (uint32_t)__shfl((int)r0, 16 * i + (l >> 2)) + 2u * (uint32_t)(l & 3);
    const char* const rec_bytes = reinterpret_cast<const char*>(rec);

    RecPair G[kChainSets][4];
    auto fetch = [&](uint32_t pass, RecPair (&g)[4]) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        g[i] = *reinterpret_cast<const RecPair*>(rec_bytes + (min(base[i] + pass * kChainBatch, last_pair) << 3));
    };
    auto to_stage = [&](int buf, const RecPair (&g)[4]) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        stage[buf][stage_unit(16 * i + (l >> 2), l & 3)] = make_float4(g[i].x0, g[i].y0, g[i].x1, g[i].y1);
    };
    auto from_stage = [&](int buf, float4 (&R)[4]) {
#pragma unroll
      for (int u = 0; u < 4; ++u) R[u] = stage[buf][stage_unit(l, u)];
    };
    // weights, reciprocals and end markers of a pass, from the weight the run has before it
    struct Prepared {
      float x[kChainBatch], wn[kChainBatch], y[kChainBatch], wu[kChainBatch];
      bool plain;   // the pass holds the end of the run, or a weight outside the exact range
    };
    auto prepare = [&](const float4 (&R)[4], float w_in, Prepared& P) {
      uint32_t signs = 0;
      float wk = w_in;
#pragma unroll
      for (int k = 0; k < kChainBatch; ++k) {
        const float4 t = R[k >> 1];
        P.x[k] = (k & 1) ? t.z : t.x;
        P.wu[k] = (k & 1) ? t.w : t.y;
        signs |= __float_as_uint(P.wu[k]);
        wk = fabsf(P.wu[k]) + wk;
        P.wn[k] = wk;
        P.y[k] = rcp_rn(wk);
      }
      // the weights grow along the pass: the first and the last bound them all
      P.plain = ((signs >> 31) != 0) | !(P.wn[0] >= 0x1p-20f) | !(P.wn[kChainBatch - 1] <= 0x1p40f);
    };

    static_assert(kChainSets == 4, "the rotation below is written for four register sets / buffers");
    fetch(0, G[0]);
    fetch(1, G[1]);
    fetch(2, G[2]);
    fetch(3, G[3]);
    to_stage(0, G[0]);
    fetch(4, G[0]);
    to_stage(1, G[1]);
    fetch(5, G[1]);
    float4 R[4];
    Prepared cur, nxt;
    from_stage(0, R);
    prepare(R, w, cur);

    uint32_t pass = 0;
    // Pass p: records of pass p+2 go to LDS (and their registers are refilled with pass p+6),
    // pass p+1 is read from LDS and prepared, the recurrence of pass p runs.
#define PLVS_CHAIN_PASS(J, CUR, NXT)                                                                      \
  {                                                                                               \
    from_stage(((J) + 1) & 3, R);                                                                 \
    to_stage(((J) + 2) & 3, G[((J) + 2) & 3]);                                                    \
    fetch(pass + 2 + kChainSets, G[((J) + 2) & 3]);                                               \
    float s_fast = s, w_fast = w, amin = 0x1p0f, amax = 0x1p0f;                                   \
    _Pragma("unroll") for (int k = 0; k < kChainBatch; ++k)                                       \
        dist_update_rcp(s_fast, w_fast, CUR.x[k], CUR.wn[k], CUR.y[k], amin, amax);               \
    prepare(R, CUR.wn[kChainBatch - 1], NXT);                                                     \
    const bool redo = live && (CUR.plain || !(amin >= 0x1p-60f) || !(amax <= 0x1p60f));           \
    if (__ballot(redo) != 0ull && redo) {                                                         \
      bool fin = false;                                                                           \
      _Pragma("unroll") for (int k = 0; k < kChainBatch; ++k) {                                   \
        if (!fin) {                                                                               \
          float s2 = s, w2 = w, mn = 0x1p0f, mx = 0x1p0f;                                         \
          dist_update_rcp(s2, w2, CUR.x[k], CUR.wn[k], CUR.y[k], mn, mx);                         \
          if ((mn >= 0x1p-60f) && (mx <= 0x1p60f) && (CUR.wn[k] >= 0x1p-20f) &&                   \
              (CUR.wn[k] <= 0x1p40f)) {                                                           \
            s = s2;                                                                               \
            w = w2;                                                                               \
          } else {                                                                                \
            dist_update(s, w, CUR.x[k], fabsf(CUR.wu[k]));                                        \
          }                                                                                       \
          if (CUR.wu[k] < 0.0f) {                                                                 \
            fin = true;                                                                           \
            my_len = pass * kChainBatch + (uint32_t)k + 1u;                                       \
          }                                                                                       \
        }                                                                                         \
      }                                                                                           \
      if (fin) {                                                                                  \
        sdf[a] = s;                                                                               \
        weight[a] = w;                                                                            \
        live = false;                                                                             \
      }                                                                                           \
    } else {                                                                                      \
      s = s_fast;                                                                                 \
      w = w_fast;                                                                                 \
    }                                                                                             \
    ++pass;                                                                                       \
    if (__ballot(live) == 0ull) break;                                                            \
  }
    for (;;) {
      PLVS_CHAIN_PASS(0, cur, nxt)
      PLVS_CHAIN_PASS(1, nxt, cur)
      PLVS_CHAIN_PASS(2, cur, nxt)
      PLVS_CHAIN_PASS(3, nxt, cur)
    }
#undef PLVS_CHAIN_PASS
    // longest run of the call = the serial-latency floor of this stage (reported in the stats)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) my_len = max(my_len, (uint32_t)__shfl_xor((int)my_len, off));
    if (l == 0 && my_len > ctr->max_run) atomicMax(&ctr->max_run, my_len);
  }
}

}  // namespace

// ------------------------------------------------------------------ host side
// One call of the ordered pipeline: the caller's inputs, and what a stage learns for the stages behind it.
struct OrderedCall {
  const float* d_xyz;
  const float* d_normals;   // non-null: the world-cloud-with-normals flavour (Chisel::IntegrateWorldPointCloudWithNormals)
  const uint8_t* d_rgb;
  const uint32_t* d_kfid;
  int n, nclouds;
  uint32_t V = 0, ntiles = 0, D = 0;           // visits, tiles of kTileSlots visit slots, runs
  const uint32_t* skeys = nullptr;             // the sorted runs: voxel keys,
  const unsigned long long* sidx = nullptr;    //   position in rec_t | length << 32
  float ms[3] = {0.f, 0.f, 0.f};               // stages 0-2, read before their closing events are recorded again
};

static int ordered_fail(plvs_tsdf_chisel* h) {
  plvs::set_error("tsdf_chisel integrate: internal directory miss (err=%u)", h->h_ctr->err);
  return poisoned(h);
}

// Offsets and poses on the device, the per-call counters zeroed (num_chunks stays).
static int ordered_begin(plvs_tsdf_chisel* h, const OrderedCall& c, const int32_t* offsets, const float* d_Twc, hipStream_t s) {
  PLVS_HIP_TRY(h->counts.reserve((size_t)c.n + 1));
  PLVS_HIP_TRY(h->scratch.reserve(scan_scratch_words((size_t)c.n)));
  PLVS_HIP_TRY(hipMemcpyAsync(h->offsets.p, offsets, ((size_t)c.nclouds + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(pose_prep, dim3(ceil_div((size_t)c.nclouds, 64)), dim3(64), 0, s, d_Twc, c.nclouds, h->poses.p);
  PLVS_HIP_TRY(hipMemsetAsync(&h->d_ctr->total_visits, 0, sizeof(uint32_t), s));
  PLVS_HIP_TRY(hipMemsetAsync(&h->d_ctr->err, 0, 5 * sizeof(uint32_t), s));
  h->stage_set = 0;
  return PLVS_OK;
}

// Stages 1 and 2: the visits of every point, their offsets; the call's visits and new chunks read back.
static int ordered_count(plvs_tsdf_chisel* h, OrderedCall& c, hipStream_t s) {
  PLVS_HIP_TRY(stage_mark(h, 0, s));
  const auto kernel = c.d_normals ? ray_count<true> : ray_count<false>;
  hipLaunchKernelGGL(kernel, dim3(ceil_div((size_t)c.n, 256)), dim3(256), 0, s, h->P, c.d_xyz, c.d_normals, c.n, h->offsets.p,
                     c.nclouds, h->poses.p, h->dir, h->d_ctr, h->counts.p);
  PLVS_KERNEL_CHECK();
  PLVS_HIP_TRY(stage_mark(h, 1, s));
  // counts -> visit offsets (n + 1 entries: the total closes the list)
  PLVS_HIP_TRY(exclusive_scan_u32(h->counts.p, h->counts.p, (size_t)c.n, &h->d_ctr->total_visits, h->scratch.p, s));
  PLVS_HIP_TRY(hipMemcpyAsync(h->counts.p + c.n, &h->d_ctr->total_visits, sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
  PLVS_HIP_TRY(stage_mark(h, 2, s));
  int rc = read_counters(h, s);
  if (rc != PLVS_OK) return rc;
  const uint32_t err = h->h_ctr->err;
  if (err) {
    plvs::set_error("tsdf_chisel integrate: %s%s", (err & kErrPoolFull) ? "chunk pool full (raise max_chunks) " : "",
                    (err & kErrCoordRange) ? "voxel coordinates beyond +-2^20 (outside the supported map extent) " : "");
    return poisoned(h);
  }
  c.V = h->h_ctr->total_visits;
  const int chunks_before = h->num_chunks;
  h->num_chunks = h->h_ctr->num_chunks;
  h->stats.visits = c.V;
  h->stats.new_chunks = h->num_chunks - chunks_before;
  return PLVS_OK;
}

// What V visits need; the times of stages 0 and 1, which are complete (the counter read synchronised).
static int ordered_reserve(plvs_tsdf_chisel* h, OrderedCall& c) {
  const uint32_t V = c.V;
  c.ntiles = ceil_div(V, kTileSlots);
  PLVS_HIP_TRY(h->dkey0.reserve(V));
  PLVS_HIP_TRY(h->tile_first.reserve(c.ntiles));
  PLVS_HIP_TRY(h->tile_state.reserve((size_t)c.ntiles + 1));
  PLVS_HIP_TRY(h->updated.reserve((size_t)h->num_chunks + 1));
  PLVS_HIP_TRY(h->rec_t.reserve(V));
  PLVS_HIP_TRY(h->recc_t.reserve(V));
  PLVS_HIP_TRY(h->rec.reserve((size_t)V + 2));   // chain_runs reads record pairs
  PLVS_HIP_TRY(h->didx0.reserve(V));
  PLVS_HIP_TRY(h->last_pt.reserve(V));
  PLVS_HIP_TRY(h->block_first.reserve(ceil_div(V, kGatherSpan)));
  if (h->profiling) {
    PLVS_HIP_TRY(stage_elapsed(&c.ms[0], h->ev[0], h->ev[1]));
    PLVS_HIP_TRY(stage_elapsed(&c.ms[1], h->ev[1], h->ev[2]));
  }
  return PLVS_OK;
}

// Stage 3: the tiles; the number of runs read back (it sizes the sort).
static int ordered_tiles(plvs_tsdf_chisel* h, OrderedCall& c, hipStream_t s) {
  PLVS_HIP_TRY(stage_mark(h, 2, s));   // (again: the first record stands in front of a host read)
  PLVS_HIP_TRY(hipMemsetAsync(h->tile_state.p, 0, ((size_t)c.ntiles + 1) * sizeof(unsigned long long), s));
  hipLaunchKernelGGL(mark_tiles, dim3(ceil_div((size_t)c.n, 256)), dim3(256), 0, s, h->counts.p, c.n, h->tile_first.p);
  // per-visit (u, point): in the buffer the gather fills later
  const TileOut out{h->rec.p, h->rec_t.p, h->recc_t.p, h->dkey0.p, h->didx0.p, h->last_pt.p};
  const auto kernel = c.d_normals ? ray_tiles<true> : ray_tiles<false>;
  hipLaunchKernelGGL(kernel, dim3(c.ntiles), dim3(kTileThreads), 0, s, h->P, c.d_xyz, c.d_normals, c.d_rgb, c.n, h->offsets.p,
                     c.nclouds, h->poses.p, h->dir, h->d_ctr, h->counts.p, c.V, h->tile_first.p, c.ntiles,
                     reinterpret_cast<uint32_t*>(h->tile_state.p), h->tile_state.p + 1, h->rgbw, out);
  PLVS_KERNEL_CHECK();
  PLVS_HIP_TRY(stage_mark(h, 3, s));
  int rc = read_counters(h, s);
  if (rc != PLVS_OK) return rc;
  if (h->h_ctr->err) return ordered_fail(h);
  c.D = h->h_ctr->num_desc;
  if (h->profiling) PLVS_HIP_TRY(stage_elapsed(&c.ms[2], h->ev[2], h->ev[3]));
  return PLVS_OK;
}

// Stage 4: the run descriptors by voxel key.
static int ordered_sort(plvs_tsdf_chisel* h, OrderedCall& c, hipStream_t s) {
  const uint32_t D = c.D;
  PLVS_HIP_TRY(h->dkey1.reserve(D));
  PLVS_HIP_TRY(h->scratch.reserve(radix_scratch_words(D)));
  PLVS_HIP_TRY(h->didx1.reserve(D));
  PLVS_HIP_TRY(h->run_cnt.reserve(D));
  PLVS_HIP_TRY(h->run_dst.reserve(D));
  PLVS_HIP_TRY(stage_mark(h, 3, s));   // (again, as for event 2)
  bool second = false;
  PLVS_HIP_TRY(radix_sort_pairs_u64(h->dkey0.p, h->didx0.p, h->dkey1.p, h->didx1.p, D, 0, voxel_key_bits(h->num_chunks),
                                    h->scratch.p, s, &second));
  c.skeys = second ? h->dkey1.p : h->dkey0.p;
  c.sidx = second ? h->didx1.p : h->didx0.p;
  PLVS_HIP_TRY(stage_mark(h, 4, s));
  return PLVS_OK;
}

// Stage 5: voxel heads and the gather into voxel order; beside it, on the side stream, the colours.
static int ordered_gather_and_fold(plvs_tsdf_chisel* h, const OrderedCall& c, hipStream_t s) {
  const uint32_t D = c.D, V = c.V;
  PLVS_HIP_TRY(h->heads.reserve(D));
  hipLaunchKernelGGL(voxel_heads, dim3(ceil_div(D, 256 * kHeadTiles)), dim3(256), 0, s, c.skeys, D, h->heads.p, h->updated.p,
                     h->d_ctr);
  // The colour fold (truncating u8 mean, exact: fold_colours) reads the tile-ordered colours through
  // the sorted runs and touches only rgbw, so it runs on a second stream beside the gather; the
  // distance chain then has the machine to itself.
  PLVS_HIP_TRY(hipEventRecord(h->ev_fork, s));
  PLVS_HIP_TRY(hipStreamWaitEvent(h->side, h->ev_fork, 0));
  const auto fold = c.d_normals ? fold_colours<true> : fold_colours<false>;
  hipLaunchKernelGGL(fold, dim3(std::min<size_t>(ceil_div(D, 256), 1024)), dim3(256), 0, h->side, c.skeys, c.sidx, D,
                     h->heads.p, h->recc_t.p, h->rgbw, h->d_ctr);
  PLVS_HIP_TRY(hipEventRecord(h->ev_join, h->side));
  hipLaunchKernelGGL(run_counts, dim3(ceil_div(D, 256)), dim3(256), 0, s, c.sidx, D, h->run_cnt.p);
  PLVS_HIP_TRY(exclusive_scan_u32(h->run_cnt.p, h->run_dst.p, D, nullptr, h->scratch.p, s));
  const uint32_t nblocks = ceil_div(V, kGatherSpan);
  hipLaunchKernelGGL(mark_blocks, dim3(ceil_div(D, 256)), dim3(256), 0, s, h->run_dst.p, D, V, h->block_first.p);
  hipLaunchKernelGGL(gather_runs, dim3(nblocks), dim3(kGatherThreads), 0, s, c.skeys, c.sidx, D, h->last_pt.p, h->run_dst.p,
                     h->block_first.p, nblocks, V, h->rec_t.p, h->recc_t.p, h->rec.p, (uint32_t*)nullptr, c.d_kfid, h->kfid);
  PLVS_KERNEL_CHECK();
  PLVS_HIP_TRY(stage_mark(h, 5, s));
  return PLVS_OK;
}

// Stage 6: the distance chain; the colours join behind it.
static int ordered_chain(plvs_tsdf_chisel* h, const OrderedCall& c, hipStream_t s) {
  // one thread per voxel; the grid is an upper bound of the voxel count, surplus waves exit
  // on the device-side count
  hipLaunchKernelGGL(chain_runs, dim3(std::min<size_t>(ceil_div(c.D, 64), 16384)), dim3(64), 0, s, h->heads.p, c.skeys,
                     h->run_dst.p, c.V, h->rec.p, h->d_ctr, h->sdf, h->weight);
  PLVS_HIP_TRY(hipStreamWaitEvent(s, h->ev_join, 0));
  PLVS_KERNEL_CHECK();
  PLVS_HIP_TRY(stage_mark(h, 6, s));
  return PLVS_OK;
}

// The finished call: its counters, the stage times, the stats.
static int ordered_finish(plvs_tsdf_chisel* h, const OrderedCall& c, hipStream_t s) {
  int rc = read_counters(h, s);
  if (rc != PLVS_OK) return rc;
  if (h->profiling) {
    for (int i = 0; i < 3; ++i) h->stage_ms[i] += c.ms[i];
    if ((rc = add_stage_times(h, 3, kNumStages - 3)) != PLVS_OK) return rc;
    h->prof_calls++;
  }
  if (h->h_ctr->err) return ordered_fail(h);
  h->stats.updated_chunks = (int32_t)h->h_ctr->num_updated;
  h->stats.voxels = (int32_t)h->h_ctr->num_heads;
  h->stats.max_run = (int32_t)h->h_ctr->max_run;
  h->last_updated = h->h_ctr->num_updated;
  return PLVS_OK;
}

// n > 0 points of nclouds clouds (offsets checked, h->offsets and h->poses reserved by the caller).
static int integrate_ordered(plvs_tsdf_chisel* h, const float* d_xyz, const uint8_t* d_rgb, const uint32_t* d_kfid, int n,
                             int nclouds, const int32_t* offsets, const float* d_Twc, hipStream_t s, const float* d_normals) {
  OrderedCall c{d_xyz, d_normals, d_rgb, d_kfid, n, nclouds};
  int rc = ordered_begin(h, c, offsets, d_Twc, s);
  if (rc == PLVS_OK) rc = ordered_count(h, c, s);
  if (rc != PLVS_OK || c.V == 0) return rc;
  if (c.V >= (1u << 29)) {
    plvs::set_error("tsdf_chisel integrate: %u voxel visits in one call exceed the 2^29 limit (split the batch)", c.V);
    return PLVS_ERR_CAPACITY;
  }
  if ((rc = ordered_reserve(h, c)) != PLVS_OK) return rc;
  if ((rc = ordered_tiles(h, c, s)) != PLVS_OK) return rc;
  if ((rc = ordered_sort(h, c, s)) != PLVS_OK) return rc;
  if ((rc = ordered_gather_and_fold(h, c, s)) != PLVS_OK) return rc;
  if ((rc = ordered_chain(h, c, s)) != PLVS_OK) return rc;
  return ordered_finish(h, c, s);
}
