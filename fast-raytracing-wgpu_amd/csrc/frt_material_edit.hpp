// frt_material_edit.hpp — device side of frt_renderer_set_instance_materials: the material id of an instance is one word of its
// 64-byte instance record and one word (q[25], SceneBuilder::write_shade_tri) of the 128-byte shading record of each of its triangles. One kernel
// stores those words; nothing is read back, no triangle slot and no box changes. The host specification is SceneBuilder::set_instance_materials
// (frt_scene.cpp). The other material, light and texture edits are plain copies into the replica's tables and need no kernel.
#pragma once
#include "frt_trace.hpp"
#include <hip/hip_runtime.h>

namespace frt {

// One edited instance, 16 B, built on the host (an instance appears at most once: the host keeps the last of several values) and copied up with the others.
struct MaterialEditInstance {
    uint32_t first_tri;     // its first flattened triangle id
    uint32_t work_begin;    // prefix sum of tri_count over the records before this one
    uint32_t id;            // instance index
    uint32_t mat_id;        // its new material
};
static_assert(sizeof(MaterialEditInstance) == 16, "MaterialEditInstance layout");

struct MaterialEditArgs {
    const MaterialEditInstance* rec; uint32_t nrec, work;   // records and their summed tri_count
    uint32_t num_instances;                                 // of the replica (SceneView has no count of them)
};

// One launch on `stream`; nothing when there is no record.
hipError_t launch_instance_materials(const SceneView& sc, const MaterialEditArgs& a, hipStream_t stream);

} // namespace frt
