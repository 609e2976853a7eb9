// frt_refit.hpp — device side of frt_renderer_set_instance_transforms: re-transform the moved instances' triangles into the
// triangle slots, then refit the pair and quad trees level by level, deepest first. The host specification is SceneBuilder::set_instance_transforms
// (frt_scene.cpp) and SceneBuilder::refit (frt_bvh.cpp); the results are bit-identical (same f32 operations, no contraction, exact min / max).
#pragma once
#include "frt_trace.hpp"
#include <hip/hip_runtime.h>

namespace frt {

// One moved instance, 208 B, built on the host and copied up in one piece with the others.
struct MovedInstance {
    uint32_t id;            // instance index
    uint32_t first_tri;     // its first flattened triangle id
    uint32_t tri_count;
    uint32_t index_offset;  // of its mesh in SceneView::indices
    uint32_t pos_offset;    // of its mesh's first vertex in the object-space positions
    uint32_t work_begin;    // prefix sum of tri_count over the records before this one
    uint32_t light;         // light index to overwrite with `light_rec`, or 0xFFFFFFFF
    uint32_t pad;
    float m[12];            // columns 0..3 of the 4x4, xyz each: m[3c + r]
    InstanceView dev;       // the new device instance record (w2o, flip)
    LightView light_rec;
};
static_assert(sizeof(MovedInstance) == 208, "MovedInstance layout");

struct RefitArgs {
    const MovedInstance* rec; uint32_t nrec, work;   // records and their summed tri_count
    const float4* pos;                               // object-space positions of every mesh, xyzw
    const uint32_t* slot_of;                         // flattened triangle id -> triangle slot
    unsigned int* ext;                               // max |coordinate| over all triangle bounds, as f32 bits (one word)
};

// Transform + record scatter, then the scene-box reduction (ext zeroed first), all on `stream`.
hipError_t launch_instance_transform(const SceneView& sc, const RefitArgs& a, hipStream_t stream);
// The scene-box reduction alone (what launch_instance_transform ends with): `ext` zeroed, then max |coordinate| over every triangle slot.
hipError_t launch_scene_extent(const SceneView& sc, unsigned int* ext, hipStream_t stream);
// One refit level: pair nodes [p0, p1) and quad nodes [q0, q1) (each range one level of its tree, every deeper level already refit).
hipError_t launch_refit_level(const SceneView& sc, const unsigned int* ext, uint32_t p0, uint32_t p1, uint32_t q0, uint32_t q1, hipStream_t stream);

} // namespace frt
