// One more C entry point over the reference's open_chisel library, in a library of its own
// (oracle/ref/Makefile -> oracle/_ref/libchisel_set_chunk_ref.so, linked against libchisel_full_ref.so, whose handle
// it takes): one chunk's voxels written through the reference's own setters — DistVoxel::SetSDF / SetWeight / SetKfid,
// ColorVoxel::SetRed .. SetWeight; the chunk is created (ChunkManager::CreateChunk) when the map lacks it.  The tests
// seed voxel states with it that no integrate would reach (tests/chisel_scan_edge_scenario.py,
// tests/test_oracle_pinned_chisel_map.py).  Calls only.  chisel_full_ref_wrap.cpp is included for the handle's layout.
// TEST INFRASTRUCTURE ONLY: nothing under plvs_amd/ may call into this file.
#include "chisel_full_ref_wrap.cpp"

extern "C" void ref_chisel_set_chunk(void* p, int cx, int cy, int cz, const float* sdf, const float* weight,
                                     const uint32_t* kfid, const uint32_t* rgbw) {
  chisel::ChunkManager& cm = static_cast<FullRef*>(p)->map->GetMutableChunkManager();
  const chisel::ChunkID id(cx, cy, cz);
  if (!cm.HasChunk(id)) cm.CreateChunk(id);
  chisel::ChunkPtr chunk = cm.GetChunk(id);
  for (int i = 0; i < 4096; ++i) {
    chisel::DistVoxel& d = chunk->GetDistVoxelMutable(i);
    d.SetSDF(sdf[i]);
    d.SetWeight(weight[i]);
    d.SetKfid(kfid[i]);
    chisel::ColorVoxel& c = chunk->GetColorVoxelMutable(i);
    c.SetRed((uint8_t)(rgbw[i] & 255u));
    c.SetGreen((uint8_t)((rgbw[i] >> 8) & 255u));
    c.SetBlue((uint8_t)((rgbw[i] >> 16) & 255u));
    c.SetWeight((uint8_t)(rgbw[i] >> 24));
  }
}
