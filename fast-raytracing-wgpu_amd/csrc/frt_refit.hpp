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

// The device functions the kernels that write triangle slots share (frt_refit.hip, frt_deform.hip, frt_instance_edit.hip). Contract flags: no
// contraction, no hand-written fma, so every operation is world_triangle's (frt_scene.cpp), in its order.
// Vertex k of a triangle under the 3x4 `m` (columns 0..3, xyz each: m[3c + r]): w[k] = ((c0*x + c1*y) + c2*z) + c3.
__device__ inline void instance_world_vertices(const float* m, const float4 p[3], float w[3][3]) {
    for (int k = 0; k < 3; ++k)
        for (int c = 0; c < 3; ++c) w[k][c] = ((m[c] * p[k].x + m[3 + c] * p[k].y) + m[6 + c] * p[k].z) + m[9 + c];
}
// The whole triangle slot (build_gpu_layout): (v0, id bits) (e1 = v1 - v0, instance bits) (e2 = v2 - v0, 0).
__device__ inline void store_tri_slot(float4* t, const float w[3][3], uint32_t id, uint32_t inst) {
    t[0] = make_float4(w[0][0], w[0][1], w[0][2], __uint_as_float(id));
    t[1] = make_float4(w[1][0] - w[0][0], w[1][1] - w[0][1], w[1][2] - w[0][2], __uint_as_float(inst));
    t[2] = make_float4(w[2][0] - w[0][0], w[2][1] - w[0][1], w[2][2] - w[0][2], 0.0f);
}

// Transform + record scatter, then the scene-box reduction (ext zeroed first), all on `stream`.
hipError_t launch_instance_transform(const SceneView& sc, const RefitArgs& a, hipStream_t stream);
// The scene-box reduction alone (what launch_instance_transform ends with): `ext` zeroed, then max |coordinate| over every triangle slot.
hipError_t launch_scene_extent(const SceneView& sc, unsigned int* ext, hipStream_t stream);
// One refit level: pair nodes [p0, p1) and quad nodes [q0, q1) (each range one level of its tree, every deeper level already refit).
hipError_t launch_refit_level(const SceneView& sc, const unsigned int* ext, uint32_t p0, uint32_t p1, uint32_t q0, uint32_t q1, hipStream_t stream);

} // namespace frt
