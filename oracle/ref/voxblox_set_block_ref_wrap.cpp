// One more C entry point over the reference's voxblox, in a library of its own (oracle/ref/Makefile ->
// oracle/_ref/libvoxblox_set_block_ref.so, linked against libvoxblox_ref.so, whose map handle it takes, so that the
// libraries built before it stay what they were): one block's voxels written through the reference's own Layer / Block /
// TsdfVoxel — Layer::allocateBlockPtrByIndex (which returns the block the map already has), Block::getVoxelByLinearIndex,
// the voxel's members, and the two flags an integrate sets.  No counterpart in the reference; calls only.  The tests
// seed voxel states with it that no integrate would reach (tests/mesh_crafted_scenario.py, tests/test_oracle_pinned.py).
// voxblox_integrator_ref_wrap.cpp is included for the handle's layout.
// TEST INFRASTRUCTURE ONLY: nothing under plvs_amd/ may call into this file.
#include "voxblox_integrator_ref_wrap.cpp"

extern "C" void ref_voxblox_set_block(void* h, int bx, int by, int bz, const float* distance, const float* weight,
                                      const uint32_t* rgba) {
  voxblox::Block<voxblox::TsdfVoxel>::Ptr b =
      static_cast<RefMap*>(h)->layer->allocateBlockPtrByIndex(voxblox::BlockIndex(bx, by, bz));
  for (size_t i = 0; i < b->num_voxels(); ++i) {
    voxblox::TsdfVoxel& v = b->getVoxelByLinearIndex(i);
    v.distance = distance[i];
    v.weight = weight[i];
    v.color = voxblox::Color((uint8_t)(rgba[i] & 255u), (uint8_t)((rgba[i] >> 8) & 255u), (uint8_t)((rgba[i] >> 16) & 255u),
                             (uint8_t)(rgba[i] >> 24));
  }
  b->has_data() = true;
  b->updated() = true;
}
