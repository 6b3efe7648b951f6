// One more C entry point over the reference's open_chisel library, in a library of its own
// (oracle/ref/Makefile -> oracle/_ref/libchisel_mesh_ids_ref.so, linked against libchisel_full_ref.so, whose handle it
// takes, so that the libraries built before it stay what they were): the meshes of a given list of chunks.
// Chisel::UpdateMeshes (Chisel.cpp:57-65) is ChunkManager::RecomputeMeshes(meshesToUpdate), and only an integrate or a
// deform fills that private set: chunks written with ref_chisel_set_chunk are meshed by handing RecomputeMeshes the
// ids directly (n x 3).  ref_chisel_full_mesh_chunk then reads each mesh (tests/mesh_crafted_scenario.py,
// tests/test_oracle_pinned_chisel_map.py).  Calls only.  chisel_full_ref_wrap.cpp is included for the handle's layout.
// TEST INFRASTRUCTURE ONLY: nothing under plvs_amd/ may call into this file.
#include "chisel_full_ref_wrap.cpp"

extern "C" void ref_chisel_recompute_meshes(void* p, const int32_t* ids, int n) {
  chisel::ChunkSet todo;
  for (int i = 0; i < n; ++i) todo[chisel::ChunkID(ids[3 * i], ids[3 * i + 1], ids[3 * i + 2])] = true;
  static_cast<FullRef*>(p)->map->GetMutableChunkManager().RecomputeMeshes(todo);
}
