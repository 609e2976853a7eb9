// frt_instance_edit.hpp — device side of frt_renderer_add_instances / _remove_instances: the triangles, shading records, instance
// records and id -> slot table of the replica with instances appended or taken out, written OUT OF PLACE into buffers that enter the replica together
// with the tree the rebuild (frt_rebuild.hpp) then makes over them. The host specification is SceneBuilder::add_instances / remove_instances
// (frt_scene.cpp): the new buffers hold, id for id, what flatten() and build_gpu_layout make of the resulting instance list, bit for bit — the
// transform and the shading record are the device functions of frt_refit.hpp and frt_deform.hpp, and w2o / flip come from the host, in double.
// In the new triangle buffer flattened triangle id i lies in slot i (the rebuild sorts the slots anyway), except that an append keeps the old slots
// where they were: the old buffers are copied and the new triangles follow them.
#pragma once
#include "frt_deform.hpp"

namespace frt {

// One appended instance, 144 B, built on the host and copied up with the others.
struct AppendInstance {
    uint32_t id;            // its (new) instance index
    uint32_t first_tri;     // its first flattened triangle id
    uint32_t tri_count;
    uint32_t work_begin;    // prefix sum of tri_count over the records before this one
    uint32_t index_offset;  // of its mesh in SceneView::indices
    uint32_t pos_offset;    // of its mesh's first vertex in the object-space positions
    uint32_t attr_offset;   // of its mesh's first vertex in SceneView::attributes and in the decoded normals
    uint32_t pad;
    float m[12];            // columns 0..3 of the 4x4, xyz each: m[3c + r]
    InstanceView dev;       // its device instance record
};
static_assert(sizeof(AppendInstance) == 144, "AppendInstance layout");

// The buffers an edit writes; each has room for the new counts.
struct InstanceEditTarget { float4* tris; uint32_t* slot_of; float4* shade_tris; InstanceView* instances; };

struct AppendArgs {
    const AppendInstance* rec; uint32_t nrec, work;   // records and their summed tri_count
    const float4* pos;                                // object-space positions of every mesh, xyzw
    const float4* normals;                            // decoded normal of every vertex of the scene (xyz, 0), indexed as SceneView::attributes
    uint32_t num_tris, num_instances;                 // of the scene AFTER the call: nothing is written at or beyond them
    InstanceEditTarget out;
};

// One removed instance, 16 B; the records are sorted by instance id. Positions are in the NEW numbering: what survives in front of the range.
struct RemovedRange {
    uint32_t new_tri;       // flattened triangles that survive in front of this instance's
    uint32_t tris_through;  // triangles removed up to and including this instance's
    uint32_t new_inst;      // instances that survive in front of it
    uint32_t pad;
};

struct RemoveArgs {
    const RemovedRange* rng; uint32_t nrng;
    const uint32_t* slot_of;                          // the replica's id -> slot table (old ids)
    uint32_t old_tris, old_instances;                 // of the replica as it is
    uint32_t num_tris, num_instances;                 // after the call
    InstanceEditTarget out;
};

// Triangles [first new id, num_tris) and instance records of the appended instances into `a.out`; `sc` gives the indices and attributes.
hipError_t launch_instances_append(const SceneView& sc, const AppendArgs& a, hipStream_t stream);
// Every surviving triangle (slot, shading record) and instance record of `sc` into `a.out` under its new id.
hipError_t launch_instances_remove(const SceneView& sc, const RemoveArgs& a, hipStream_t stream);

} // namespace frt
