// frt_refit_device.hpp — device side of frt_renderer_set_instance_transforms_ex with FRT_TRANSFORM_DEVICE ("Transforms from device
// memory"): the ids and matrices of a call are device memory, so everything the host form does before its kernel runs — the checks, the choice of the
// last record of an id given twice, the inverse in double, the records of the instances and of their linked lights — is done by kernels, from small
// per-instance tables the renderer keeps on the device. The result is the host form's, bit for bit (frt_instance_record.hpp restates its arithmetic);
// the scene-extent pass and the level-by-level refit of frt_refit.hpp follow unchanged.
#pragma once
#include "frt_refit.hpp"

namespace frt {

// What the host holds per instance (RefitState::inst and what it looks up with it) and a matrix does not change, 48 B.
struct InstanceConst {
    uint32_t first_tri, tri_count;   // its flattened triangles
    uint32_t index_offset;           // of its mesh in SceneView::indices
    uint32_t pos_offset;             // of its mesh's first vertex in the object-space positions
    uint32_t mesh_id, mat_id;
    uint32_t light;                  // the light registered with it, or 0xFFFFFFFF
    uint32_t light_kind;             // 0 quad, 1 sphere
    float emission[4];               // of that light
};
static_assert(sizeof(InstanceConst) == 48, "InstanceConst layout");

// `reject`: [0] the flag of this call, zeroed on the stream in front of the validation launch; [1] the calls rejected so far (as DeformInput::reject).
struct TransformInput {
    const uint32_t* ids; const float4* mats; uint32_t n;   // the caller's: [n] and [4 n] (column-major 4x4, one column per float4)
    uint32_t num_inst;
    const InstanceConst* consts;     // [num_inst]
    float4* m;                       // [4 num_inst]: the current matrix of every instance (the truth once a device call has been made)
    uint32_t* last;                  // [num_inst]: 1 + the last record of this call that names the instance, 0: it does not move
    uint32_t* reject;
    const float4* pos;               // object-space positions of every mesh, xyzw
    const uint32_t* slot_of;         // flattened triangle id -> triangle slot
    uint32_t cap_verts, cap_indices; // capacities of the vertex and index pools
};

// On `stream`, in this order: the flag and `last` zeroed; validation (one thread per record: an id out of range, a non-finite entry or a 3x3 whose
// determinant is zero raises the flag; otherwise the record enters `last` by atomicMax); records (one thread per record: returns at once under a raised
// flag — its first thread then counts the rejection — and otherwise, if its record is the last of its instance, stores the matrix, the instance record
// and the light record); triangles (one thread per triangle of the SCENE: a triangle whose instance moved is transformed into its slot). A bad id is
// never used as an index by any of them.
hipError_t launch_device_transforms(const SceneView& sc, const TransformInput& a, hipStream_t stream);

} // namespace frt
