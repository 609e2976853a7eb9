// frt_deform.hpp — device side of frt_renderer_set_mesh_vertices ("Deforming meshes"): after the new object-space positions (and
// attributes) of one mesh have been copied into the replica, re-transform the triangles of every instance of that mesh into their slots and, when
// attributes were given, write their shading records again. The scene-extent pass and the level-by-level refit of frt_refit.hpp follow unchanged.
// The host specification is SceneBuilder::set_mesh_vertices (frt_scene.cpp); the results are bit-identical: the same f32 operations in the same
// order, no contraction, and vertex normals decoded once per vertex on the host by the function build_gpu_layout uses.
#pragma once
#include "frt_refit.hpp"

namespace frt {

// One instance of the deformed mesh, 64 B, built on the host and copied up with the others.
struct DeformInstance {
    uint32_t id;            // instance index
    uint32_t first_tri;     // its first flattened triangle id
    uint32_t tri_count;
    uint32_t work_begin;    // prefix sum of tri_count over the records before this one
    float m[12];            // columns 0..3 of the instance's current 4x4, xyz each: m[3c + r]
};
static_assert(sizeof(DeformInstance) == 64, "DeformInstance layout");

struct DeformArgs {
    const DeformInstance* rec; uint32_t nrec, work;   // records and their summed tri_count
    uint32_t index_offset;                            // of the mesh in SceneView::indices
    uint32_t pos_offset;                              // of the mesh's first vertex in `pos`
    uint32_t attr_offset;                             // of the mesh's first vertex in SceneView::attributes
    const float4* pos;                                // object-space positions of every mesh, xyzw (already the new ones)
    const float4* normals;                            // decoded normal of every vertex of the mesh (xyz, 0), or null: shading records stay
    const uint32_t* slot_of;                          // flattened triangle id -> triangle slot
};

// The triangle (and shading record) rewrite on `stream`. Launches nothing when there is no work.
hipError_t launch_mesh_deform(const SceneView& sc, const DeformArgs& a, hipStream_t stream);

} // namespace frt
