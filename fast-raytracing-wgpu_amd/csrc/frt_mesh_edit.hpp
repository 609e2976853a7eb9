// frt_mesh_edit.hpp — device side of frt_renderer_add_meshes: the vertices and indices of the new meshes go from the call's staging
// block into the replica's pools (object-space positions, attributes, decoded normals, indices) and their mesh-info records are written. The host
// specification is SceneBuilder::add_mesh (frt_scene.cpp): the pools hold, element for element, what the builder's arrays hold, and the decoded
// normals what decoded_vertex_normal (frt_bvh.cpp) gives: the same function, frt_shade.hpp's decode_octahedral_normal, compiled for the device under
// the library's contract flags. New materials, lights and texture layers are plain staged copies and need no kernel.
#pragma once
#include "frt_scene.hpp"      // MeshAppend
#include "frt_trace.hpp"
#include <hip/hip_runtime.h>

namespace frt {

struct MeshAppendArgs {
    const MeshAppend* rec; uint32_t nrec;             // one record per new mesh, sorted by vert_begin and index_begin (prefix sums)
    uint32_t nverts, nidx;                            // the call's vertices and indices: the launch covers nverts + nidx work items
    const float4* pos;                                // staged: xyzw per vertex, in record order
    const float4* attrs;                              // staged: two float4 per vertex, (normal.xy, uv.xy) (tangent.xyzw)
    const uint32_t* idx;                              // staged: the meshes' indices (mesh-relative, copied unchanged)
    float4* out_pos; float4* out_attrs; float4* out_normals; uint32_t* out_idx; MeshInfoView* out_infos;      // the replica's pools
    uint32_t mesh_base;                               // id of the first new mesh
    uint32_t cap_verts, cap_indices, cap_meshes;      // room in the pools: nothing is written at or beyond them
};

// One launch on `stream`; nothing when there is no record.
hipError_t launch_mesh_append(const MeshAppendArgs& a, hipStream_t stream);

} // namespace frt
